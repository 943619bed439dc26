"""The matrix-triple mode of phase 1 (include/linreg_gc_p1_matrix.h) on the MI355X: the initializer, provider A and provider B
run in one process through the Python binding.  E, F, T and both shares equal the model of tests/ti_matrix_model.py word for
word at both widths, and the shares sum to the block lgc_p1_local forms over a column range holding both sets.  Shapes sit at
the kernel's edges: the 64-column tile, the 16-row slab, the 256-row split threshold, a ragged last chunk."""
import ctypes as C

import numpy as np
import pytest

import ti_matrix_model as tm
from test_ti_matrix_cpu import SEEDS, data

pytestmark = pytest.mark.gpu

P = {64: 56, 32: 24}
SHAPES = [(1, 1, 1), (15, 1, 2), (16, 65, 1), (17, 3, 64), (255, 64, 65), (512, 63, 64), (513, 65, 130), (1031, 2, 129)]


def three_roles(lgc, ph, Xq, yq, cols_a, cols_b, w):
    """(what the library computed, what the model computed) for one instance on the rows ph holds"""
    a, b = len(cols_a), len(cols_b)
    sa, sb, ss = SEEDS
    got = {"T": lgc.ti_matrix_generate(sa, sb, ss, ph.n, a, b, w), "E": ph.matrix_mask(cols_a, sa), "F": ph.matrix_mask(cols_b, sb)}
    got["share_a"] = ph.matrix_share_a(a, sa, ss, got["F"], b)
    got["share_b"] = ph.matrix_share_b(cols_b, got["E"], a, got["T"])
    want = tm.run(tm.columns(Xq, yq, cols_a), tm.columns(Xq, yq, cols_b), sa, sb, ss, w)
    return got, want


def check(got, want, w):
    wire = np.uint32 if w == 32 else np.uint64
    for k in ("E", "F", "T"):
        assert got[k].dtype == wire, k                                        # wire form: W-bit words
    for k in ("E", "F", "T", "share_a", "share_b"):
        g = got[k].astype(np.uint64)
        assert g.shape == want[k].shape, k
        assert not (g >> np.uint64(w - 1) >> np.uint64(1)).any(), k           # W = 32: no bit above 31
        assert np.array_equal(g, want[k]), k


def total(got, w):
    with np.errstate(over="ignore"):
        return (got["share_a"] + got["share_b"]) & np.uint64(tm.mask(w))


def local_block(ph, d, cols_a, cols_b, with_y):
    """<column cols_a[i], column cols_b[j]> from lgc_p1_local over all d columns (and y)"""
    r = ph.local(0, d, with_y=with_y)
    A, bvec = r if with_y else (r, None)
    idx = lambda i, j: max(i, j) * (max(i, j) + 1) // 2 + min(i, j)
    return np.array([[bvec[j] if i == d else A[idx(i, j)] for j in cols_b] for i in cols_a], dtype=np.uint64)


@pytest.mark.parametrize("w", [32, 64])
@pytest.mark.parametrize("n,a,b", SHAPES)
def test_three_roles_equal_the_model(lgc, n, a, b, w):
    rng = np.random.default_rng(100000 * w + 1000 * n + a)
    d = a + b
    Xq, _ = data(rng, n, d, w)
    cols_b, cols_a = list(range(b)), list(range(b, d))           # A holds the higher columns
    ph = lgc.Phase1(Xq, None, w, P[w])
    got, want = three_roles(lgc, ph, Xq, None, cols_a, cols_b, w)
    check(got, want, w)
    assert np.array_equal(total(got, w), local_block(ph, d, cols_a, cols_b, False))
    assert np.array_equal(total(got, w), tm.gram_block(tm.columns(Xq, None, cols_a), tm.columns(Xq, None, cols_b), w))
    ph.close()


@pytest.mark.parametrize("w", [32, 64])
def test_unsorted_column_lists(lgc, w):
    rng = np.random.default_rng(7 + w)
    n, d = 100, 12
    Xq, _ = data(rng, n, d, w)
    cols_a, cols_b = [9, 3, 11], [7, 0, 5, 2]
    ph = lgc.Phase1(Xq, None, w, P[w])
    got, want = three_roles(lgc, ph, Xq, None, cols_a, cols_b, w)
    check(got, want, w)
    assert np.array_equal(total(got, w), local_block(ph, d, cols_a, cols_b, False))
    ph.close()


@pytest.mark.parametrize("w", [32, 64])
def test_y_among_the_columns_of_a(lgc, w):
    rng = np.random.default_rng(11 + w)
    n, d = 70, 7
    Xq, yq = data(rng, n, d, w)
    cols_a, cols_b = [5, 6, d], [0, 1, 2, 3]
    ph = lgc.Phase1(Xq, yq, w, P[w])
    got, want = three_roles(lgc, ph, Xq, yq, cols_a, cols_b, w)
    check(got, want, w)
    assert np.array_equal(total(got, w), local_block(ph, d, cols_a, cols_b, True))
    ph.close()


@pytest.mark.parametrize("w", [32, 64])
def test_row_window(lgc, w):
    """set_rows(5, 300) of n = 400: the window starts and ends off a slab boundary; every word is what an object created from
    those rows gives, and what the model gives on them"""
    rng = np.random.default_rng(13 + w)
    n, d, r0, r1 = 400, 9, 5, 300
    Xq, yq = data(rng, n, d, w)
    cols_a, cols_b = [6, 7, 8, d], [0, 1, 2, 3, 4]
    ph, cut = lgc.Phase1(Xq, yq, w, P[w]), lgc.Phase1(Xq[r0:r1], yq[r0:r1], w, P[w])
    ph.set_rows(r0, r1)
    got, want = three_roles(lgc, ph, Xq[r0:r1], yq[r0:r1], cols_a, cols_b, w)
    other, _ = three_roles(lgc, cut, Xq[r0:r1], yq[r0:r1], cols_a, cols_b, w)
    check(got, want, w)
    assert all(np.array_equal(got[k], other[k]) for k in got)
    assert np.array_equal(total(got, w), local_block(ph, d, cols_a, cols_b, True))
    ph.set_rows(0, n)
    whole, want_all = three_roles(lgc, ph, Xq, yq, cols_a, cols_b, w)
    check(whole, want_all, w)
    ph.close(); cut.close()


@pytest.mark.parametrize("w", [32, 64])
def test_device_io(lgc, w):
    """lgc_p1_set_device_io: the blocks E and F are device memory on both ends; the words are the host path's"""
    L = lgc.lib()
    for f, args in (("lgc_dev_alloc", [C.c_int, C.c_size_t, C.POINTER(C.c_void_p), C.c_void_p]), ("lgc_dev_upload", [C.c_void_p, C.c_void_p, C.c_size_t]),
                    ("lgc_dev_download", [C.c_void_p, C.c_void_p, C.c_size_t])):
        getattr(L, f).argtypes = args; getattr(L, f).restype = C.c_int
    L.lgc_dev_free.argtypes = [C.c_void_p]; L.lgc_dev_free.restype = None
    rng = np.random.default_rng(17 + w)
    n, d = 300, 70
    Xq, yq = data(rng, n, d, w)
    cols_a, cols_b = list(range(60, d)) + [d], list(range(0, 66))             # a = 11, b = 66: two tiles on B's side
    a, b = len(cols_a), len(cols_b)
    sa, sb, ss = SEEDS
    ph = lgc.Phase1(Xq, yq, w, P[w])
    host, want = three_roles(lgc, ph, Xq, yq, cols_a, cols_b, w)
    check(host, want, w)
    wire = np.uint32 if w == 32 else np.uint64
    dE, dF = C.c_void_p(), C.c_void_p()
    assert L.lgc_dev_alloc(0, n * a * (w // 8), C.byref(dE), None) == 0 and L.lgc_dev_alloc(0, n * b * (w // 8), C.byref(dF), None) == 0
    ph.set_device_io(True)
    ph.matrix_mask(cols_a, sa, out_ptr=dE.value)
    ph.matrix_mask(cols_b, sb, out_ptr=dF.value)
    E, F = np.zeros((n, a), dtype=wire), np.zeros((n, b), dtype=wire)
    assert L.lgc_dev_download(E.ctypes.data_as(C.c_void_p), dE, E.nbytes) == 0 and L.lgc_dev_download(F.ctypes.data_as(C.c_void_p), dF, F.nbytes) == 0
    got = {"E": E, "F": F, "T": host["T"], "share_a": ph.matrix_share_a(a, sa, ss, dF.value, b), "share_b": ph.matrix_share_b(cols_b, dE.value, a, host["T"])}
    ph.set_device_io(False)
    check(got, want, w)
    L.lgc_dev_free(dE); L.lgc_dev_free(dF)
    ph.close()


def test_refusals_on_a_handle(lgc):
    """a column index past d, column d when y is not set: LGC_EINVAL; an empty block writes nothing"""
    rng = np.random.default_rng(19)
    Xq, yq = data(rng, 20, 4, 64)
    ph, phy = lgc.Phase1(Xq, None, 64, 56), lgc.Phase1(Xq, yq, 64, 56)
    E = np.zeros((20, 2), dtype=np.uint64)
    for h, cols, want in ((ph, [0, 5], "out of range"), (phy, [0, 5], "out of range"), (ph, [0, 4], "y is not set")):
        with pytest.raises(lgc.LgcError) as e:
            h.matrix_mask(cols, SEEDS[0])
        assert e.value.code == -1 and want in str(e.value)
        with pytest.raises(lgc.LgcError) as e:
            h.matrix_share_b(cols, E, 2, np.zeros((2, 2), dtype=np.uint64))
        assert e.value.code == -1 and want in str(e.value)
    assert phy.matrix_mask([0, 4], SEEDS[0]).shape == (20, 2)
    assert ph.matrix_mask([], SEEDS[0]).shape == (20, 0)
    assert ph.matrix_share_a(0, SEEDS[0], SEEDS[2], np.zeros((20, 3), dtype=np.uint64), 3).shape == (0, 3)
    ph.close(); phy.close()


@pytest.mark.parametrize("w", [32, 64])
def test_gram_and_rect_kernels_after_the_generalised_tile_body(lgc, w):
    """p1_gram_folds_kernel and p1_rect_kernel pass X on both sides of the generalised body: their words on a (300, 70) input
    (two tiles a side, a split, a ragged slab) are numpy's"""
    rng = np.random.default_rng(23 + w)
    n, d, k = 300, 70, 3
    Xq, _ = data(rng, n, d, w)
    Yq = rng.integers(-(1 << (w - 1)), 1 << (w - 1), size=(n, k), dtype=np.int64)
    U, V = Xq.view(np.uint64), Yq.view(np.uint64)
    m = np.uint64(tm.mask(w))
    with np.errstate(over="ignore"):
        G, B = (U.T @ U) & m, (V.T @ U) & m
    ph = lgc.Phase1(Xq, Yq[:, 0], w, P[w])
    A, bvec = ph.local(0, d, with_y=True)
    off = [(i, j) for i in range(d) for j in range(i)]
    assert [int(A[i * (i + 1) // 2 + j]) for i, j in off] == [int(G[i, j]) for i, j in off]
    assert np.array_equal(bvec, B[0])
    ph.close()
    pt = lgc.Phase1(Xq, Yq, w, P[w], targets=k)
    _, Bt = pt.local_targets(0, d)
    assert np.array_equal(Bt, B)
    pt.close()
