"""The per-pair and per-batch share kernels of the trusted-initializer protocol (p1_mask_kernel, p1_mask1_kernel, p1_dot_kernel,
p1_dot1_kernel, p1_ti_a_kernel, p1_ti_a_batch_kernel and p1_block_sum of csrc/phase1.hip, behind lgc_p1_mask, lgc_p1_dot,
lgc_p1_ti_a and lgc_p1_ti_a_batch) on the MI355X, word for word against tests/p1_model.py.  X is full-range (sign-extended from 32
bits at w = 32) and every vector is full-range below 2^w, so every sum wraps; d = 2 with a y column, and column d (y) is among the
columns of every case.  The row counts are the edges of the launch rules: the single-pair kernels run min(ceil(n / 1024), 64)
workgroups of 1024 threads, the batch kernels min(ceil(n / 256), 64) of 256 per pair, the pairs in grid.y."""
import ctypes as C
import functools

import numpy as np
import pytest

import p1_model

pytestmark = pytest.mark.gpu

WIDTHS = [(64, 56), (32, 28)]
D = 2                       # columns 0 and 1 of X, y is column 2
MAX_PAIRS = 65535           # of one launch: grid.y
EINVAL = -1

# 63, 64, 65: a ragged wave in p1_block_sum; 1023, 1024, 1025: the last size of one workgroup, the first of two;
# 65536, 65537, 66561: the last single trip of the grid-stride loop, a second trip of one element, of a workgroup and one element
SINGLE_ROWS = [1, 63, 64, 65, 1023, 1024, 1025, 65536, 65537, 66561]
# 255, 256, 257: one and two workgroups per pair; 16384, 16385: the last single trip, a second trip of one element
BATCH_ROWS = [1, 255, 256, 257, 16384, 16385]
BATCH_PAIRS = [2, 17]
DEVIO_ROWS = [257, 16385]


def _words(rng, shape, w):
    return rng.integers(0, (1 << w) - 1, shape, dtype=np.uint64, endpoint=True)


@functools.lru_cache(maxsize=None)
def _case(n, npairs, w):
    """inputs and the model's words, once per process.  X: (n, 3) with y as column 2; cols starts at y and walks all three with
    period 4, so that pair 65535, the first of a second launch or trip over the pairs, has another column than pair 0"""
    rng = np.random.default_rng([n, npairs, w])
    X = rng.integers(-(1 << (w - 1)), 1 << (w - 1), (n, D + 1), dtype=np.int64)
    cols = np.array([D, 0, 1, 0], dtype=np.uint32)[np.arange(npairs) % 4]
    c = _with_model(X, cols, _words(rng, (npairs, n), w), _words(rng, (npairs, n), w), _words(rng, npairs, w), w)
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


def _with_model(X, cols, V, Y, sub, w):
    """the inputs and what p1_model makes of them: V is the vector of mask and the A of dot (party b's message `in` of ti_a),
    Y the B of dot (the initializer's y of ti_a)"""
    ti_mask, ti_share = p1_model.ti_a(X, cols, Y, V, sub, w)
    return dict(X=X, cols=cols, V=V, Y=Y, sub=sub, w=w,
                pos=p1_model.mask(X, cols, V, +1, w), neg=p1_model.mask(X, cols, V, -1, w),
                dot_b=p1_model.dot(V, Y, sub, w), dot_b0=p1_model.dot(V, Y, None, w),
                dot_c=p1_model.dot(V, p1_model.columns(X, cols), sub, w), ti_mask=ti_mask, ti_share=ti_share)


def _window(c, r0, r1):
    """the case of rows [r0, r1) of c: the model on X[r0:r1] and the same rows of every vector"""
    return _with_model(c["X"][r0:r1], c["cols"], np.ascontiguousarray(c["V"][:, r0:r1]), np.ascontiguousarray(c["Y"][:, r0:r1]),
                       c["sub"], c["w"])


def _handle(lgc, c, p):
    return lgc.Phase1(c["X"][:, :D], c["X"][:, D], c["w"], p)


def _check_single(h, c):
    """one pair per call: p1_mask1_kernel, p1_dot1_kernel, p1_ti_a_kernel"""
    for q, col in enumerate(c["cols"].tolist()):
        V, Y, sub = c["V"][q:q + 1], c["Y"][q:q + 1], c["sub"][q:q + 1]
        assert np.array_equal(h.mask([col], V, +1), c["pos"][q:q + 1])
        assert np.array_equal(h.mask([col], V, -1), c["neg"][q:q + 1])
        assert np.array_equal(h.dot(V, B=Y, sub=sub), c["dot_b"][q:q + 1])
        assert np.array_equal(h.dot(V, B=Y), c["dot_b0"][q:q + 1])
        assert np.array_equal(h.dot(V, cols=[col], sub=sub), c["dot_c"][q:q + 1])
        m, s = h.ti_a(col, Y[0], V[0], sub[0])
        assert np.array_equal(m, c["ti_mask"][q]) and int(s) == int(c["ti_share"][q])


def _check_batch(h, c):
    """all pairs in one call: p1_mask_kernel, p1_dot_kernel, p1_ti_a_batch_kernel; and p1_ti_a_kernel row by row"""
    cols, V, Y, sub = c["cols"], c["V"], c["Y"], c["sub"]
    assert np.array_equal(h.mask(cols, V, +1), c["pos"])
    assert np.array_equal(h.mask(cols, V, -1), c["neg"])
    assert np.array_equal(h.dot(V, B=Y, sub=sub), c["dot_b"])
    assert np.array_equal(h.dot(V, B=Y), c["dot_b0"])
    assert np.array_equal(h.dot(V, cols=cols, sub=sub), c["dot_c"])
    m, s = h.ti_a_batch(cols, Y, V, sub)
    assert np.array_equal(m, c["ti_mask"]) and np.array_equal(s, c["ti_share"])
    for q, col in enumerate(cols.tolist()):
        m1, s1 = h.ti_a(col, Y[q], V[q], sub[q])
        assert np.array_equal(m1, m[q]) and int(s1) == int(s[q])


class _Dev:
    """device buffers of lgc_dev_alloc, as the same-node rings of the host program pass them"""

    def __init__(self, lgc):
        self.L = L = lgc.lib()
        for f, a in (("lgc_dev_alloc", [C.c_int, C.c_size_t, C.POINTER(C.c_void_p), C.c_void_p]),
                     ("lgc_dev_upload", [C.c_void_p, C.c_void_p, C.c_size_t]), ("lgc_dev_download", [C.c_void_p, C.c_void_p, C.c_size_t])):
            getattr(L, f).argtypes = a; getattr(L, f).restype = C.c_int
        L.lgc_dev_free.argtypes = [C.c_void_p]; L.lgc_dev_free.restype = None
        self.ptrs = []

    def upload(self, a):
        a = np.ascontiguousarray(a, dtype=np.uint64)
        ptr = C.c_void_p()
        assert self.L.lgc_dev_alloc(0, a.nbytes, C.byref(ptr), None) == 0
        self.ptrs.append(ptr)
        assert self.L.lgc_dev_upload(ptr, a.ctypes.data_as(C.c_void_p), a.nbytes) == 0
        return ptr

    def ones(self, shape):
        """a result buffer with every bit set: a word the kernel leaves, or leaves untruncated, shows"""
        return self.upload(np.full(shape, ~np.uint64(0), dtype=np.uint64))

    def download(self, ptr, shape):
        out = np.zeros(shape, dtype=np.uint64)
        assert self.L.lgc_dev_download(out.ctypes.data_as(C.c_void_p), ptr, out.nbytes) == 0
        return out

    def close(self):
        for ptr in self.ptrs:
            self.L.lgc_dev_free(ptr)
        self.ptrs = []


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _devio_mask(h, dev, c, sign):
    shape = c["V"].shape
    dV, dOut = dev.upload(c["V"]), dev.ones(shape)
    assert dev.L.lgc_p1_mask(h._h, _vp(c["cols"]), shape[0], dV, sign, dOut) == 0
    out = dev.download(dOut, shape)
    if c["w"] == 32:
        assert not (out >> np.uint64(32)).any()              # what a peer that maps the buffer reads
    return out


def _devio_ti_a_batch(h, dev, c):
    shape = c["V"].shape
    dY, dIn, dOut = dev.upload(c["Y"]), dev.upload(c["V"]), dev.ones(shape)
    shares = np.zeros(shape[0], dtype=np.uint64)
    assert dev.L.lgc_p1_ti_a_batch(h._h, _vp(c["cols"]), shape[0], dY, dIn, _vp(c["sub"]), dOut, _vp(shares)) == 0
    out = dev.download(dOut, shape)
    if c["w"] == 32:
        assert not (out >> np.uint64(32)).any() and not (shares >> np.uint64(32)).any()
    return out, shares


def _check_devio(h, dev, c):
    """vectors in device memory (set_device_io): the same three calls, the sums still returned to the host"""
    npairs = len(c["cols"])
    assert np.array_equal(_devio_mask(h, dev, c, +1), c["pos"])
    assert np.array_equal(_devio_mask(h, dev, c, -1), c["neg"])
    dA, dB = dev.upload(c["V"]), dev.upload(c["Y"])
    for B, cols, sub, exp in ((dB, None, c["sub"], "dot_b"), (dB, None, None, "dot_b0"), (None, c["cols"], c["sub"], "dot_c")):
        out = np.full(npairs, ~np.uint64(0), dtype=np.uint64)
        assert dev.L.lgc_p1_dot(h._h, dA, B, None if cols is None else _vp(cols), npairs, None if sub is None else _vp(sub), _vp(out)) == 0
        assert np.array_equal(out, c[exp])
    m, s = _devio_ti_a_batch(h, dev, c)
    assert np.array_equal(m, c["ti_mask"]) and np.array_equal(s, c["ti_share"])


@pytest.mark.parametrize("w,p", WIDTHS)
@pytest.mark.parametrize("n", SINGLE_ROWS)
def test_single_pair_calls(lgc, n, w, p):
    c = _case(n, 3, w)
    h = _handle(lgc, c, p)
    _check_single(h, c)
    h.close()


@pytest.mark.parametrize("w,p", WIDTHS)
@pytest.mark.parametrize("npairs", BATCH_PAIRS)
@pytest.mark.parametrize("n", BATCH_ROWS)
def test_batch_calls(lgc, n, npairs, w, p):
    c = _case(n, npairs, w)
    h = _handle(lgc, c, p)
    _check_batch(h, c)
    h.close()


@pytest.mark.parametrize("w,p", WIDTHS)
@pytest.mark.parametrize("n", DEVIO_ROWS)
def test_device_io_calls(lgc, n, w, p):
    c = _case(n, 3, w)
    h = _handle(lgc, c, p)
    dev = _Dev(lgc)
    h.set_device_io(True)
    _check_devio(h, dev, c)
    dev.close()
    h.close()


@pytest.mark.parametrize("w,p", WIDTHS)
def test_device_io_mask_launches_65536_pairs_in_two_chunks(lgc, w, p):
    """the second launch of the 65535-pair loop takes the last pair: its column from dcols + 65535, its words from V + 65535 n"""
    c = _case(3, MAX_PAIRS + 1, w)
    assert c["cols"][-1] != c["cols"][0]
    h = _handle(lgc, c, p)
    dev = _Dev(lgc)
    h.set_device_io(True)
    for sign, exp in ((+1, "pos"), (-1, "neg")):
        out = _devio_mask(h, dev, c, sign)
        assert np.array_equal(out[-1], c[exp][-1])
        assert np.array_equal(out, c[exp])
    dev.close()
    h.close()


@pytest.mark.parametrize("w,p", WIDTHS)
def test_ti_a_batch_strides_grid_y_over_65536_pairs(lgc, w, p):
    """65535 workgroup rows for 65536 pairs: row 0 takes pair 65535 in a second trip of the q += gridDim.y loop, on the host path
    and with device I/O"""
    c = _case(2, MAX_PAIRS + 1, w)
    h = _handle(lgc, c, p)
    m, s = h.ti_a_batch(c["cols"], c["Y"], c["V"], c["sub"])
    assert np.array_equal(m[-1], c["ti_mask"][-1]) and int(s[-1]) == int(c["ti_share"][-1])
    assert np.array_equal(m, c["ti_mask"]) and np.array_equal(s, c["ti_share"])
    dev = _Dev(lgc)
    h.set_device_io(True)
    m, s = _devio_ti_a_batch(h, dev, c)
    assert np.array_equal(m, c["ti_mask"]) and np.array_equal(s, c["ti_share"])
    dev.close()
    h.close()


@pytest.mark.parametrize("w,p", WIDTHS)
def test_65535_pairs_is_the_most_of_one_call(lgc, w, p):
    """mask and dot on the host path, dot with device I/O, and the initializer's lgc_ti_generate put the pair in grid.y of a single
    launch: 65535 pairs give the model's words, 65536 are refused with LGC_EINVAL before any device call, the limit named in
    lgc_last_error() and the output untouched"""
    big = _case(1, MAX_PAIRS + 1, w)
    c = {k: (v[:MAX_PAIRS] if isinstance(v, np.ndarray) else v) for k, v in big.items() if k != "X"}
    h = _handle(lgc, big, p)
    assert np.array_equal(h.mask(c["cols"], c["V"], -1), c["neg"])
    assert np.array_equal(h.dot(c["V"], B=c["Y"], sub=c["sub"]), c["dot_b"])
    assert np.array_equal(h.dot(c["V"], cols=c["cols"], sub=c["sub"]), c["dot_c"])

    L, npairs = lgc.lib(), MAX_PAIRS + 1
    mark = np.uint64(0x5a5a5a5a5a5a5a5a)

    def refused(rc, out):
        msg = L.lgc_last_error().decode()
        return rc == EINVAL and "too many pairs" in msg and str(MAX_PAIRS) in msg and (out == mark).all()
    out = np.full((npairs, 1), mark, dtype=np.uint64)
    assert refused(L.lgc_p1_mask(h._h, _vp(big["cols"]), npairs, _vp(big["V"]), +1, _vp(out)), out)
    for B, cols in ((_vp(big["Y"]), None), (None, _vp(big["cols"]))):
        out = np.full(npairs, mark, dtype=np.uint64)
        assert refused(L.lgc_p1_dot(h._h, _vp(big["V"]), B, cols, npairs, _vp(big["sub"]), _vp(out)), out)
    with pytest.raises(lgc.LgcError) as e:
        h.mask(big["cols"], big["V"], +1)
    assert e.value.code == EINVAL and "too many pairs" in str(e.value)
    with pytest.raises(lgc.LgcError) as e:
        lgc.ti_generate(bytes(range(16)), 0, npairs, 1, w)
    assert e.value.code == EINVAL and "too many pairs" in str(e.value) and str(MAX_PAIRS) in str(e.value)

    dev = _Dev(lgc)
    h.set_device_io(True)
    dA, dB = dev.upload(big["V"]), dev.upload(big["Y"])
    out = np.full(npairs, mark, dtype=np.uint64)
    assert refused(L.lgc_p1_dot(h._h, dA, dB, None, npairs, _vp(big["sub"]), _vp(out)), out)
    out = np.full(npairs, mark, dtype=np.uint64)
    assert refused(L.lgc_p1_dot(h._h, dA, None, _vp(big["cols"]), npairs, _vp(big["sub"]), _vp(out)), out)
    dev.close()
    h.close()


@pytest.mark.parametrize("w,p", WIDTHS)
def test_row_window(lgc, w, p):
    """after set_rows(r0, r1) with r0 > 0 every call acts on rows [r0, r1): one case of each group, the model on X[r0:r1].
    1063 rows: two workgroups of the single-pair kernels, five per pair of the batch kernels"""
    n, r0, r1 = 1100, 37, 1100
    for npairs, check in ((3, _check_single), (17, _check_batch)):
        c = _case(n, npairs, w)
        h = _handle(lgc, c, p)
        h.set_rows(r0, r1)
        check(h, _window(c, r0, r1))
        h.close()
    c = _case(n, 3, w)
    h = _handle(lgc, c, p)
    h.set_rows(r0, r1)
    dev = _Dev(lgc)
    h.set_device_io(True)
    _check_devio(h, dev, _window(c, r0, r1))
    dev.close()
    h.close()
