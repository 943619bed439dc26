"""Several target columns in one secure solve (include/linreg_gc_targets.h) on the MI355X: the co-located solver, the two
roles apart, and phase 1 with k target columns (the rectangular X^T Y kernel) against the oracle and numpy."""
import numpy as np
import pytest

from helpers import oracle_solve, split_shares

pytestmark = pytest.mark.gpu


def _targets_system(oracle, rng, n, d, k, w, p):
    X = rng.standard_normal((n, d)); X /= np.abs(X).max(axis=0)
    Xq = oracle.quantize(X, p, n, w)
    A0, bs = None, []
    for t in range(k):
        y = X @ rng.random(d) + 0.1 * rng.standard_normal(n)
        A, b = oracle.aggregate(Xq, oracle.quantize(y, p, n, w), n, d, p, w)
        A0 = A if A0 is None else A0
        bs.append(b)
    return A0, bs


@pytest.mark.parametrize("alg,w,p", [("cgd", 64, 56), ("cholesky", 32, 28), ("ldlt", 64, 56)])
def test_solver_targets_match_oracle_and_single_solves(lgc, oracle, alg, w, p):
    rng = np.random.default_rng(40 + w + len(alg))
    d, n, k, iters, lam = 12, 80, 4, 5, 0.001
    A, bs = _targets_system(oracle, rng, n, d, k, w, p)
    shares = split_shares(rng, A, np.concatenate(bs), 2, w)
    sysm = lgc.make_system(d, w, p, alg, iters, lam, 2, 1, 1, 0)
    s = lgc.Solver(sysm, seed=bytes(range(16)), targets=k)
    assert lgc.lib().lgc_solver_num_targets(s._h) == k
    s.set_shares(shares)
    s.run()
    beta = s.beta()
    inputs = s.inputs()
    s.close()
    assert beta.shape == (k, d)
    T = d * (d + 1) // 2
    for t in range(k):
        exp, a, bb = oracle_solve(oracle, A, bs[t], d, w, p, alg, iters, lam, 1)
        assert beta[t].tolist() == exp.tolist(), t
        assert inputs[T + t * d:T + (t + 1) * d].tolist() == bb.tolist()
        # the same target solved on its own on the GPU
        one = lgc.Solver(sysm, seed=bytes(range(16)))
        one.set_shares(split_shares(rng, A, bs[t], 2, w))
        one.run()
        assert one.beta().tolist() == beta[t].tolist(), t
        one.close()
    assert inputs[:T].tolist() == a.tolist()


def test_parties_apart_with_three_targets(lgc, oracle):
    rng = np.random.default_rng(7)
    w, p, d, n, k, P = 64, 56, 6, 50, 3, 2
    A, bs = _targets_system(oracle, rng, n, d, k, w, p)
    shares = split_shares(rng, A, np.concatenate(bs), P, w)
    sysm = lgc.make_system(d, w, p, "cholesky", 0, 0.001, P, 1, 0, 0)
    small = 1 << 20
    G = lgc.Party(sysm, lgc.GARBLER, seed=bytes(range(5, 21)), max_launch_table_bytes=small, targets=k)
    E = lgc.Party(sysm, lgc.EVALUATOR, max_launch_table_bytes=small, targets=k)
    assert G.input_bits == (d * (d + 1) // 2 + k * d) * w
    assert lgc.lib().lgc_party_num_targets(E._h) == k
    assert G.program_fingerprint() == E.program_fingerprint()
    two = lgc.Party(sysm, lgc.EVALUATOR, max_launch_table_bytes=small, targets=2)
    assert two.program_fingerprint() != E.program_fingerprint()
    two.close()
    for s in range(P):
        E.set_input_labels(s, G.encode_inputs(s, shares[s]))
    for i in range(G.num_launches):
        E.evaluate(i, G.garble(i))
    beta, _, _ = E.finish(G.decode_bits())
    G.close(); E.close()
    assert beta.shape == (k, d)
    for t in range(k):
        exp, _, _ = oracle_solve(oracle, A, bs[t], d, w, p, "cholesky", 0, 0.001, 1)
        assert beta[t].tolist() == exp.tolist(), t


@pytest.mark.parametrize("n,d,c0,c1,k,w,p", [
    (1003, 140, 3, 133, 1, 64, 56), (1003, 140, 0, 140, 5, 64, 56), (257, 70, 5, 70, 70, 32, 28), (4099, 90, 20, 85, 70, 64, 54),
])
def test_phase1_local_targets_against_numpy(lgc, oracle, n, d, c0, c1, k, w, p):
    rng = np.random.default_rng(n + k)
    X = rng.standard_normal((n, d)); X /= np.abs(X).max(axis=0)
    Y = X[:, :min(d, 8)] @ rng.random((min(d, 8), k)) + 0.1 * rng.standard_normal((n, k))
    Xq = oracle.quantize(X, p, n, w).reshape(n, d)
    Yq = np.stack([oracle.quantize(Y[:, t].copy(), p, n, w) for t in range(k)], axis=1)
    m = np.uint64((1 << w) - 1) if w < 64 else np.uint64(0xFFFFFFFFFFFFFFFF)
    ph = lgc.Phase1(Xq, Yq, w, p, targets=k)
    A, B = ph.local_targets(c0, c1)
    with np.errstate(over="ignore"):
        Bx = (Xq[:, c0:c1].astype(np.uint64).T @ Yq.astype(np.uint64)).T & m      # X[:, c0:c1]^T Y mod 2^w, k x own
    assert B.shape == (k, c1 - c0)
    assert np.array_equal(B, Bx)
    ref = lgc.Phase1(Xq, Yq[:, 0].copy(), w, p)                                  # a single-target handle, same data
    assert np.array_equal(A, ref.local(c0, c1))
    ref.close()
    # column d + t is target t for the TI arithmetic
    V = rng.integers(0, 2 ** 63, size=(3, n), dtype=np.uint64)
    cols = [d, d + k // 2, d + k - 1]
    got = ph.dot(V, cols=cols)
    with np.errstate(over="ignore"):
        exp = [int((V[q] * Yq[:, c - d].astype(np.uint64)).sum(dtype=np.uint64) & m) for q, c in enumerate(cols)]
    assert got.tolist() == exp
    with pytest.raises(lgc.LgcError):
        ph.dot(V[:1], cols=[d + k])                                              # past the last target
    ph.close()
