"""shared helpers for the parity tests"""
import numpy as np


def edge_operands(rng, w, n):
    """operand pairs (a, b) as uint64 arrays: the 14 edge values of a w-bit word pairwise (196 pairs), then n random pairs of
    mixed magnitudes and both signs"""
    m = (1 << w) - 1
    edge = [0, 1, 2, 3, m, m - 1, 1 << (w - 1), (1 << (w - 1)) - 1, (1 << (w - 1)) + 1, 5, 0x5555555555555555 & m,
            0xAAAAAAAAAAAAAAAA & m, 1 << (w // 2), (1 << (w // 2)) - 1]
    a = [x for x in edge for _ in edge]
    b = [y for _ in edge for y in edge]
    r = rng.integers(0, 1 << 63, size=(2, n), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(2, n), dtype=np.uint64)
    # mixed magnitudes: shift random values right by random amounts, keep signs varied
    sh = rng.integers(0, w, size=(2, n)).astype(np.uint64)
    r = (r & np.uint64(m)) >> sh
    neg = rng.integers(0, 2, size=(2, n)).astype(bool)
    r = np.where(neg, (~r + np.uint64(1)) & np.uint64(m), r)
    a = np.concatenate([np.array(a, dtype=np.uint64), r[0]])
    b = np.concatenate([np.array(b, dtype=np.uint64), r[1]])
    return a, b


def synth_system(oracle, rng, n, d, w, p, lam=0.001, sigma=0.1):
    """experiments/generate_tests.py:159-169 distribution, quantised and aggregated
    by the oracle.  Returns (A_total, b_total) as uint64 (T and d entries)."""
    X = rng.standard_normal((n, d)); X /= np.abs(X).max(axis=0)
    beta = rng.random(d)
    y = X @ beta + sigma * rng.standard_normal(n)
    Xq = oracle.quantize(X, p, n, w); yq = oracle.quantize(y, p, n, w)
    A, b = oracle.aggregate(Xq, yq, n, d, p, w)
    return A, b


def split_shares(rng, A, b, nshares, w):
    """additive shares mod 2^w of the (T + d) vector; share-major (nshares, T + d)"""
    tot = np.concatenate([A, b]).astype(np.uint64)
    m = np.uint64((1 << w) - 1) if w < 64 else np.uint64(0xFFFFFFFFFFFFFFFF)
    sh = rng.integers(0, 2 ** 63, size=(nshares, tot.size), dtype=np.uint64) * np.uint64(2) + \
        rng.integers(0, 2, size=(nshares, tot.size), dtype=np.uint64)
    sh &= m
    with np.errstate(over="ignore"):
        sh[0] = (tot - sh[1:].sum(axis=0, dtype=np.uint64)) & m
    return sh


def oracle_solve(oracle, A, b, d, w, p, alg, iters, lam, normalize, trace=False):
    a = oracle.sum_shares(np.asarray(A, dtype=np.uint64)[None, :], w)
    bb = oracle.sum_shares(np.asarray(b, dtype=np.uint64)[None, :], w)
    if normalize:
        a, bb = oracle.circuit_input(a, bb, d, lam, p, w)
    if alg == "cgd":
        return oracle.cgd(a, bb, d, p, w, iters, trace=trace), a, bb
    if alg == "cholesky":
        return oracle.cholesky(a, bb, d, p, w), a, bb
    return oracle.ldlt(a, bb, d, p, w), a, bb


def sx(v, w):
    v = np.asarray(v, dtype=np.uint64)
    if w == 32:
        return v.astype(np.uint32).astype(np.int32).astype(np.int64)
    return v.astype(np.int64)


def openssl_gate_hash(labels, tweaks):
    """The fixed-key AES gate hash H(x, t) = AES_k(sigma(x) ^ t) ^ sigma(x) ^ t, sigma(xL || xR) = (xL ^ xR) || xL, written
    here from its definition over OpenSSL's AES-128 (libcrypto through ctypes): shares no line with the product's T-table AES
    or with oracle/gc_cpu.cpp (which is compiled from the product's headers), so agreement is an independent check of both.
    labels (n, 16) uint8, tweaks (n,) uint64 in the low half.  Key: FIPS-197 Appendix B (the build's fixed public key)."""
    import ctypes
    import ctypes.util
    import numpy as np
    crypto = ctypes.CDLL(ctypes.util.find_library("crypto") or "libcrypto.so.3")
    key = bytes.fromhex("2b7e151628aed2a6abf7158809cf4f3c")
    sched = ctypes.create_string_buffer(256)                           # AES_KEY
    assert crypto.AES_set_encrypt_key(key, 128, sched) == 0
    x = np.ascontiguousarray(labels, dtype=np.uint8).reshape(-1, 16)
    out = np.zeros_like(x)
    inb, outb = ctypes.create_string_buffer(16), ctypes.create_string_buffer(16)
    for i in range(len(x)):
        # the label is a little-endian 128-bit number: xL = its HIGH half (bytes 8..15), xR = its low half (bytes 0..7);
        # sigma(x) = (xL ^ xR) || xL has xL ^ xR in the high half and xL in the low half; the 64-bit tweak goes into the low half
        xl, xr = x[i, 8:], x[i, :8]
        k = np.concatenate([xl, xl ^ xr])
        tw = np.frombuffer(int(tweaks[i]).to_bytes(8, "little"), dtype=np.uint8)
        k[:8] ^= tw
        ctypes.memmove(inb, k.tobytes(), 16)
        crypto.AES_encrypt(inb, outb, sched)
        out[i] = np.frombuffer(outb.raw, dtype=np.uint8) ^ k
    return out


GATE_HASH_KEY = bytes.fromhex("2b7e151628aed2a6abf7158809cf4f3c")    # FIPS-197 Appendix B (the build's fixed public key)
_crypto = None


def _libcrypto():
    """OpenSSL's libcrypto with the EVP prototypes set (pointers are 64-bit: the default int return would cut them)"""
    global _crypto
    if _crypto is None:
        import ctypes as C
        import ctypes.util
        L = C.CDLL(ctypes.util.find_library("crypto") or "libcrypto.so.3")
        vp, ci = C.c_void_p, C.c_int
        L.EVP_CIPHER_CTX_new.restype = vp; L.EVP_CIPHER_CTX_new.argtypes = []
        L.EVP_CIPHER_CTX_free.restype = None; L.EVP_CIPHER_CTX_free.argtypes = [vp]
        L.EVP_aes_128_ecb.restype = vp; L.EVP_aes_128_ecb.argtypes = []
        L.EVP_EncryptInit_ex.restype = ci; L.EVP_EncryptInit_ex.argtypes = [vp, vp, vp, C.c_char_p, C.c_char_p]
        L.EVP_CIPHER_CTX_set_padding.restype = ci; L.EVP_CIPHER_CTX_set_padding.argtypes = [vp, ci]
        L.EVP_EncryptUpdate.restype = ci; L.EVP_EncryptUpdate.argtypes = [vp, vp, C.POINTER(ci), vp, ci]
        _crypto = L
    return _crypto


def _evp_aes128_blocks(key, blocks):
    """AES-128 of every 16-byte row of `blocks` under `key`: EVP_aes_128_ecb, padding off, ONE EVP_EncryptUpdate call"""
    import ctypes as C
    L = _libcrypto()
    blocks = np.ascontiguousarray(blocks, dtype=np.uint8).reshape(-1, 16)
    out = np.empty_like(blocks)
    if not len(blocks):
        return out
    assert blocks.nbytes < 2 ** 31                                     # EVP_EncryptUpdate takes an int length
    ctx = L.EVP_CIPHER_CTX_new()
    assert ctx
    try:
        assert L.EVP_EncryptInit_ex(ctx, L.EVP_aes_128_ecb(), None, bytes(key), None) == 1
        assert L.EVP_CIPHER_CTX_set_padding(ctx, 0) == 1
        n = C.c_int(0)
        assert L.EVP_EncryptUpdate(ctx, out.ctypes.data_as(C.c_void_p), C.byref(n), blocks.ctypes.data_as(C.c_void_p), blocks.nbytes) == 1
        assert n.value == blocks.nbytes
    finally:
        L.EVP_CIPHER_CTX_free(ctx)
    return out


def openssl_aes_ctr(key, first_block, nblocks):
    """AES-128-CTR keystream, block c = AES_key(c as a little-endian 128-bit number), c = first_block .. first_block + nblocks - 1:
    the counters are built in numpy (low 64 bits first_block + b, high 64 bits zero) and encrypted in one EVP call.
    Returns nblocks * 16 bytes (uint8)."""
    ctrs = np.zeros((nblocks, 2), dtype="<u8")
    ctrs[:, 0] = np.uint64(first_block) + np.arange(nblocks, dtype=np.uint64)
    return _evp_aes128_blocks(key, ctrs.view(np.uint8)).reshape(-1)


def openssl_gate_hash_fast(labels, tweaks):
    """openssl_gate_hash, vectorised: sigma(x) ^ t for every row in numpy, one EVP call, one xor.  Same definition, same key."""
    x = np.ascontiguousarray(labels, dtype=np.uint8).reshape(-1, 16)
    xl, xr = x[:, 8:], x[:, :8]                                        # xL = the HIGH half of the little-endian number
    k = np.concatenate([xl, xl ^ xr], axis=1)                          # sigma(x): xL in the low half, xL ^ xR in the high half
    tw = np.ascontiguousarray(tweaks, dtype="<u8").reshape(-1, 1)
    assert len(tw) == len(x)
    k[:, :8] ^= tw.view(np.uint8)                                      # the 64-bit tweak goes into the low half
    return _evp_aes128_blocks(GATE_HASH_KEY, k) ^ k


def iknp_restatement(seeds0, seeds1, delta, cbits_packed, m, ctr0):
    """The IKNP extension of m OTs restated over OpenSSL and numpy (nothing of the product or of oracle/gc_cpu.cpp): column
    PRG = AES-128-CTR under each base-OT seed from block ctr0, u_j = G(k0_j) ^ G(k1_j) ^ c, the sender's
    q_j = G(k_{delta_j}) ^ delta_j u_j, and the 128 x m bit-matrix transpose through unpackbits / packbits (LSB first in
    both directions).  cbits_packed: the m choice bits packed LSB-first (shorter is zero-padded).
    Returns (U (128, m128 * 16) uint8, rows_t (m, 16), rows_q (m, 16))."""
    seeds0 = np.asarray(seeds0, dtype=np.uint8).reshape(128, 16); seeds1 = np.asarray(seeds1, dtype=np.uint8).reshape(128, 16)
    delta = np.frombuffer(bytes(delta), dtype=np.uint8)
    dbits = np.unpackbits(delta, bitorder="little")
    seeds_s = np.where(dbits[:, None] == 1, seeds1, seeds0)            # what the base OTs give the sender
    m128 = (m + 127) // 128
    packed = np.ascontiguousarray(cbits_packed).view(np.uint8).ravel()
    cb = np.zeros(m128 * 16, dtype=np.uint8)
    cb[:len(packed)] = packed
    T = np.stack([openssl_aes_ctr(seeds0[j], ctr0, m128) for j in range(128)])              # receiver's columns t_j = G(k0_j)
    G1 = np.stack([openssl_aes_ctr(seeds1[j], ctr0, m128) for j in range(128)])
    U = T ^ G1 ^ cb[None, :]                                                                # u_j = G(k0_j) ^ G(k1_j) ^ c
    Gs = np.stack([openssl_aes_ctr(seeds_s[j], ctr0, m128) for j in range(128)])            # sender: it holds k_{delta_j}
    Q = Gs ^ (U * dbits[:, None])                                                           # q_j ( = t_j ^ delta_j c )
    # bit-matrix transpose: row i holds bit i of every column, column j at bit j
    rows_t = np.packbits(np.unpackbits(T, axis=1, bitorder="little")[:, :m].T, axis=1, bitorder="little")   # (m, 16)
    rows_q = np.packbits(np.unpackbits(Q, axis=1, bitorder="little")[:, :m].T, axis=1, bitorder="little")
    return U, rows_t, rows_q


def iknp_labels_restatement(rows_t, rows_q, delta, choice, m0, m1, tweak0):
    """1-of-2 OT of 16-byte messages on given rows: e0_i = m0_i ^ H(i, q_i), e1_i = m1_i ^ H(i, q_i ^ D), the receiver's
    out_i = e_{c_i} ^ H(i, t_i); tweak of OT i is tweak0 + i.  Returns (e0, e1, out), each (m, 16) uint8."""
    delta = np.frombuffer(bytes(delta), dtype=np.uint8)
    choice = np.asarray(choice, dtype=np.uint8)
    m = len(choice)
    tweaks = np.uint64(tweak0) + np.arange(m, dtype=np.uint64)
    e0 = np.asarray(m0, dtype=np.uint8).reshape(m, 16) ^ openssl_gate_hash_fast(rows_q[:m], tweaks)
    e1 = np.asarray(m1, dtype=np.uint8).reshape(m, 16) ^ openssl_gate_hash_fast(rows_q[:m] ^ delta[None, :], tweaks)
    out = np.where(choice[:, None] == 1, e1, e0) ^ openssl_gate_hash_fast(rows_t[:m], tweaks)
    return e0, e1, out


def iknp_gilboa_restatement(rows_t, rows_q, delta, a, b, w, tweak0):
    """Gilboa inner products on given rows, from the definition in include/linreg_gc.h and ot.hip's header: OT
    i = (q n + k) w + bit, x0 = H(i, q_i), h1 = H(i, q_i ^ D) (low w bits), y_i = x0 + (b[q][k] << bit) - h1; the sender's
    share of pair q is -sum x0, the receiver's sum H(i, t_i) + c_i y_i with c_i = bit `bit` of a[q][k]; all mod 2^w, in
    numpy uint64 (which wraps mod 2^64).  Returns (y (m,), share_sender (npairs,), share_receiver (npairs,))."""
    delta = np.frombuffer(bytes(delta), dtype=np.uint8)
    a = np.ascontiguousarray(a, dtype=np.uint64); b = np.ascontiguousarray(b, dtype=np.uint64)
    npairs, n = a.shape
    m = npairs * n * w
    mask = np.uint64((1 << w) - 1)
    tweaks = np.uint64(tweak0) + np.arange(m, dtype=np.uint64)
    low = lambda h: np.ascontiguousarray(h[:, :8]).view("<u8").reshape(-1).astype(np.uint64) & mask     # low w bits of a hash
    x0 = low(openssl_gate_hash_fast(rows_q[:m], tweaks))
    h1 = low(openssl_gate_hash_fast(rows_q[:m] ^ delta[None, :], tweaks))
    ht = low(openssl_gate_hash_fast(rows_t[:m], tweaks))
    bit = np.tile(np.arange(w, dtype=np.uint64), npairs * n)
    with np.errstate(over="ignore"):
        y = (x0 + ((np.repeat(b.ravel(), w) << bit) & mask) - h1) & mask
        c = (np.repeat(a.ravel(), w) >> bit) & np.uint64(1)
        ss = (np.uint64(0) - x0.reshape(npairs, n * w).sum(axis=1, dtype=np.uint64)) & mask
        sr = (ht + c * y).reshape(npairs, n * w).sum(axis=1, dtype=np.uint64) & mask
    return y, ss, sr


def free_ports(k):
    """k listening ports BELOW the kernel's ephemeral range (ip_local_port_range, 32768-60999 here): a port from bind(0)
    lies inside that range, and while its party is not listening yet a peer's connect() attempt can be given the same number as
    its SOURCE port -- the attempt then connects to itself (TCP simultaneous open) or the party's bind fails, and the run hangs
    (one such hang in ~600 runs of the GPU suite)"""
    import socket, random
    lo = 12000
    try:
        hi = min(30000, int(open("/proc/sys/net/ipv4/ip_local_port_range").read().split()[0]) - 1)
    except (OSError, ValueError):
        hi = 30000
    ports, rnd = [], random.SystemRandom()
    while len(ports) < k:
        p = rnd.randrange(lo, hi)
        if p in ports:
            continue
        s_ = socket.socket()
        try:
            s_.bind(("127.0.0.1", p))
            ports.append(p)
        except OSError:
            pass
        finally:
            s_.close()
    return ports
