"""bin/linreg --scan=M --scan_se on the MI355X: five processes (CSP, Evaluator, three data providers) scan M = 3 candidate
columns against c = 2 shared covariates, n = 40 rows, in TI mode and with --use_ot.  The input format gives every provider a
contiguous run of columns and y to the last one, so the candidates cannot all lie with a provider that holds neither covariates
nor y: here provider 3 holds the two covariates, provider 4 two candidates and nothing else, provider 5 the last candidate and
y -- every kind of block of lgc_p1_local_scan occurs (no own covariate without y, no own covariate with y) and the pairs of two
candidates of different providers are the ones every side skips.  Every printed coefficient is the last coefficient of a plain
`cholesky` run on the file [C, g_m] with the same arguments."""
import os
import re
import subprocess

import numpy as np
import pytest

from helpers import free_ports

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "linreg-mpc_amd", "host")
P, N, C_, M = 56, 40, 2, 3
ARGS = ["cholesky", "0", "0.001"]
NUM = "-?[0-9]+\\.[0-9]+"


def _write(path, X, y, firsts):
    n, d = X.shape
    ports = free_ports(len(firsts) + 2)
    lines = ["%d %d %d" % (n, d, len(firsts)), "127.0.0.1:%d" % ports[0], "127.0.0.1:%d" % ports[1]]
    lines += ["127.0.0.1:%d %d" % (ports[2 + k], f) for k, f in enumerate(firsts)]
    lines += ["%d %d" % (n, d)] + [" ".join(repr(float(v)) for v in row) for row in X] + ["%d" % n, " ".join(repr(float(v)) for v in y), ""]
    open(path, "w").write("\n".join(lines))
    return path


def _run(path, nproviders, extra):
    exe = os.path.join(HOST, "bin", "linreg")
    procs = [subprocess.Popen([exe, path, str(P), str(k)] + ARGS + extra + ["--table_ring"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
             for k in range(1, nproviders + 3)]
    try:
        outs = [q.communicate(timeout=240) for q in procs]
    finally:
        for q in procs:
            if q.poll() is None:
                q.kill()
    assert all(q.returncode == 0 for q in procs), [e.decode()[-400:] for _, e in outs]
    return outs[1][0].decode().rstrip("\n").splitlines()


@pytest.fixture(scope="module")
def data():
    subprocess.check_call(["make", "-C", HOST], stdout=subprocess.DEVNULL)
    rng = np.random.default_rng(40)
    X = rng.standard_normal((N, C_ + M))
    X = (X - X.mean(axis=0)) / X.std(axis=0)
    y = X @ np.array([0.5, -0.3, 0.4, 0.0, -0.2]) + 0.4 * rng.standard_normal(N)
    y = (y - y.mean()) / y.std()
    return np.round(X, 9), np.round(y, 9)


@pytest.mark.parametrize("mode", [[], ["--use_ot"]], ids=["ti", "ot"])
def test_scan_equals_the_plain_runs(tmp_path, data, mode):
    X, y = data
    scan = _run(_write(str(tmp_path / "scan.in"), X, y, [0, 2, 4]), 3, mode + ["--scan=%d" % M, "--scan_se"])
    res = [l for l in scan if l.startswith("Result:")]
    assert len(res) == 1 and scan[-2] == res[0] and scan[-1].startswith("Standard errors: ")
    assert "A = " not in "\n".join(scan)                          # nothing but the candidates' coefficients is revealed
    beta = re.findall(NUM, res[0])
    assert len(beta) == M
    for m in range(M):
        Z = np.column_stack([X[:, :C_], X[:, C_ + m]])
        plain = _run(_write(str(tmp_path / ("plain%d.in" % m)), Z, y, [0, 1, 2]), 3, mode)
        last = [l for l in plain if l.startswith("Result:")]
        assert len(last) == 1 and re.findall(NUM, last[0])[-1] == beta[m], (m, last, res)
    se = [float(v) for v in re.findall(NUM, scan[-1])]
    assert len(se) == M and all(v > 0 for v in se)
    assert scan[-1] == "Standard errors: " + "".join("%20.15f " % v for v in se)       # formatted as --inference prints its own
    # and they are the least-squares quantities.  The coefficients: against the ridge solution of the normalised system (lambda
    # counts in units of the system divided by D), to phase 1's quantisation.  The standard errors: against plain OLS, which
    # the scan's differ from by the ridge term -- lambda D = 0.003 on a unit diagonal moves v_m by 0.3 % and e_m, which
    # overstates the residual by lambda |beta|^2 (linreg_gc_scan.h), by about as much: within 1 %, bound 2 %
    for m in range(M):
        Z = np.column_stack([X[:, :C_], X[:, C_ + m]])
        D = C_ + 1
        b = np.linalg.solve(Z.T @ Z / N + 0.001 * D * np.eye(D), Z.T @ y / N)
        assert abs(float(beta[m]) - b[-1]) < 1e-6
        r = y - Z @ np.linalg.solve(Z.T @ Z, Z.T @ y)
        assert abs(se[m] / np.sqrt(float(r @ r) / (N - D) * np.linalg.inv(Z.T @ Z)[-1, -1]) - 1) < 2e-2
