"""Record corpora for the per-op tests (test_ops_cpu.py, test_gpu_ops.py): every op valid at a width, on the edge operands of
helpers.edge_operands and the special cases of each op, as a linreg_gc.RecordProgram whose last launch reveals every word
(slot i = word i)."""
import numpy as np

import word_model as wm
from helpers import edge_operands

OP = wm.OP


class Corpus:
    """Sections add input words (`inp`), scratch words (`out`) and launches of records (`launch`).  Input words must be the
    first words after word 0, so a corpus is built twice: the first pass counts the inputs, the second places the scratch
    words after them.  `kind` of a launch: "gen", "mac" (OP_MAC / OP_MAC2) or "mack"."""

    def __init__(self, w, p, n_inputs=None):
        self.w, self.p = w, p
        self.inputs = []
        self.next_out = (n_inputs or 0) + 1
        self.launches = []        # (kind, records)
        self.desc = {}            # word -> what wrote it

    def inp(self, vals):
        """input words holding vals (consecutive); returns the first id"""
        first = 1 + len(self.inputs)
        self.inputs.extend(int(v) & wm.mask(self.w) for v in vals)
        return first

    def out(self, n=1):
        first = self.next_out
        self.next_out += n
        return first

    def launch(self, kind, recs, descs=None):
        self.launches.append((kind, [tuple(int(x) for x in r) for r in recs]))
        for r, d in zip(recs, descs or [None] * len(recs)):
            name = wm.OPS[int(r[0])]
            self.desc.setdefault(int(r[2]), "%s %s" % (name, d or "rec=%s" % (tuple(int(x) for x in r),)))

    def program(self, linreg_gc, modes, reveal_mode="auto"):
        """the RecordProgram: modes(kind) -> (garbler kernel, evaluator kernel) of a launch of that kind"""
        n_words = self.next_out
        recs, sizes, mg, me = [], [], [], []
        for kind, rs in self.launches:
            recs += rs
            sizes.append(len(rs))
            g, e = modes(kind)
            mg.append(g)
            me.append(e)
        recs += [(OP["REVEAL"], 1, i, i, 0, 0, 1, 1) for i in range(n_words)]
        sizes.append(n_words)
        mg.append(reveal_mode)
        me.append(reveal_mode)
        return linreg_gc.RecordProgram(self.w, self.p, recs, sizes, mg, me, n_inputs=len(self.inputs), n_words=n_words,
                                       n_reveal=n_words)

    def records(self):
        out = [r for _, rs in self.launches for r in rs]
        return out + [(OP["REVEAL"], 1, i, i, 0, 0, 1, 1) for i in range(self.next_out)]

    def words0(self):
        """the word file before the first launch: 0, the inputs, zeros"""
        return [0] + self.inputs + [0] * (self.next_out - 1 - len(self.inputs))


def _h(v):
    return "0x%x" % int(v)


def build(w, p, seed=0, n_rand=40, sections=None):
    """the corpus of every op at (w, p); sections: names to keep (None = all)"""
    def once(n_inputs):
        C = Corpus(w, p, n_inputs)
        for k, (name, fn) in enumerate(SECTIONS):
            if sections is None or name in sections:
                if (name in ONLY64_SECTIONS and w != 64) or (name in ONLY32_SECTIONS and w != 32):
                    continue
                fn(C, np.random.default_rng([seed, w, p, k]), n_rand)
        return C
    return once(len(once(None).inputs))


M32 = 0xFFFFFFFF


def _pairs(C, rng, n_rand):
    a, b = edge_operands(rng, C.w, n_rand)
    return [int(x) for x in a], [int(y) for y in b]


def sec_binary(C, rng, n_rand):
    a, b = _pairs(C, rng, n_rand)
    n = len(a)
    ia, ib = C.inp(a), C.inp(b)
    for name in ("ADD", "SUB", "MUL", "DIV", "EQ"):
        o = C.out(n)
        C.launch("gen", [(OP[name], 1, o + i, ia + i, ib + i, 0, 1, 1) for i in range(n)],
                 ["a=%s b=%s" % (_h(a[i]), _h(b[i])) for i in range(n)])
    # DIV: x / 0, 0 / 0 and INT_MIN / -1 through word 0 and explicit operands
    m = wm.mask(C.w)
    sp = C.inp([5, 1 << (C.w - 1), m, 0, (1 << (C.w - 1)) - 1])
    o = C.out(5)
    C.launch("gen", [(OP["DIV"], 1, o, sp, 0, 0, 1, 1), (OP["DIV"], 1, o + 1, 0, 0, 0, 1, 1),
                     (OP["DIV"], 1, o + 2, sp + 1, sp + 2, 0, 1, 1), (OP["DIV"], 1, o + 3, sp + 3, sp + 3, 0, 1, 1),
                     (OP["DIV"], 1, o + 4, sp + 4, sp + 2, 0, 1, 1)],
             ["5/word0", "word0/word0", "INT_MIN/-1", "0/0", "INT_MAX/-1"])
    # MULSUB: c - a b
    c = [int(x) for x in edge_operands(rng, C.w, 0)[0][::7]]
    k = min(len(c), n)
    ic = C.inp(c[:k])
    o = C.out(k)
    C.launch("gen", [(OP["MULSUB"], 1, o + i, ia + i, ib + i, ic + i, 1, 1) for i in range(k)],
             ["a=%s b=%s c=%s" % (_h(a[i]), _h(b[i]), _h(c[i])) for i in range(k)])
    # EQ on pairs that differ only in the top bit, and equal pairs
    t = [int(x) for x in rng.integers(0, 1 << 62, size=16, dtype=np.uint64)]
    ea = C.inp([v & m for v in t] + [v & m for v in t])
    eb = C.inp([(v ^ (1 << (C.w - 1))) & m for v in t] + [v & m for v in t])
    o = C.out(32)
    C.launch("gen", [(OP["EQ"], 1, o + i, ea + i, eb + i, 0, 1, 1) for i in range(32)],
             ["a=%s b=%s" % (_h(t[i % 16] & m), _h((t[i % 16] ^ (1 << (C.w - 1))) & m if i < 16 else t[i % 16] & m)) for i in range(32)])


def sec_unary(C, rng, n_rand):
    a, _ = _pairs(C, rng, n_rand)
    a = a[::14] + a[196:]        # the 14 edge values once, then the random ones
    n = len(a)
    ia = C.inp(a)
    for name in ("ABS", "SQRT", "COPY"):
        o = C.out(n)
        C.launch("gen", [(OP[name], 1, o + i, ia + i, 0, 0, 1, 1) for i in range(n)], ["a=%s" % _h(v) for v in a])
    # IDIVC by public constants
    for c in (1, 2, 3, 500, 1 << 7, (1 << 31) - 1):
        o = C.out(n)
        l = 0
        while (1 << l) < c:
            l += 1
        mm = ((1 << (C.w - 1 + l)) // c + 1) if c > 1 else 0
        C.launch("gen", [(OP["IDIVC"], 1, o + i, ia + i, mm & M32, c, l, (mm >> 32) & M32) for i in range(n)],
                 ["a=%s c=%d" % (_h(v), c) for v in a])
    # CONST, and ops whose operands are word 0 or a constant made in the launch before
    consts = [0, 1, wm.mask(C.w), 1 << (C.w - 1), 0x123456789ABCDEF0 & wm.mask(C.w)]
    o = C.out(len(consts))
    C.launch("gen", [(OP["CONST"], 1, o + i, v & M32, (v >> 32) & M32, 0, 1, 1) for i, v in enumerate(consts)],
             ["value=%s" % _h(v) for v in consts])
    q = C.out(4)
    C.launch("gen", [(OP["ADD"], 1, q, o + 4, 0, 0, 1, 1), (OP["MUL"], 1, q + 1, o + 2, o + 4, 0, 1, 1),
                     (OP["SUB"], 1, q + 2, 0, o + 3, 0, 1, 1), (OP["MUL"], 1, q + 3, 0, o + 2, 0, 1, 1)],
             ["const+word0", "const*const", "word0-const", "word0*const"])


def sec_sums(C, rng, n_rand):
    w = C.w
    v = [int(x) for x in edge_operands(rng, w, 64)[0][::3]]
    iv = C.inp(v)
    n = len(v)
    recs, descs = [], []
    ic = C.inp([v[5]])
    for cnt in (1, 2, 5, 64):
        for sa, start in ((1, 0), (3, 1), (-1, n - 1), (-2, n - 2)):
            if start + (cnt - 1) * sa >= n or start + (cnt - 1) * sa < 0:
                continue
            for op in ("SUM", "SUBSUM", "ABSSUM"):
                for c in ((0, 1, w - 1) if op == "ABSSUM" else (ic,)):
                    o = C.out()
                    recs.append((OP[op], cnt, o, iv + start, 0, c, sa, 1))
                    descs.append("cnt=%d sa=%d c=%d" % (cnt, sa, c))
    C.launch("gen", recs, descs)
    # MAX: signed / unsigned (b = 1), cnt up to 64
    recs, descs = [], []
    for cnt in (1, 2, 7, 64):
        for sa, start in ((1, 0), (-1, n - 1)):
            for ub in (0, 1):
                o = C.out()
                recs.append((OP["MAX"], cnt, o, iv + start, ub, 0, sa, 1))
                descs.append("cnt=%d sa=%d b=%d" % (cnt, sa, ub))
    C.launch("gen", recs, descs)


def sec_side(C, rng, n_rand):
    """the 64-bit side outputs: MUL / MULSUB / DIV with their hdiff, |v| and mirror words, HDIFF, DIVB"""
    a, b = _pairs(C, rng, n_rand)
    a, b = a[::5], b[::5]
    n = len(a)
    ia, ib, ic = C.inp(a), C.inp(b), C.inp(b[::-1])
    o = C.out(2 * n)
    C.launch("gen", [(OP["MUL"], 2, o + i, ia + i, ib + i, 0, n, 1) for i in range(n)], ["a=%s b=%s cnt=2" % (_h(a[i]), _h(b[i])) for i in range(n)])
    for cnt in (2, 3):
        o = C.out(2 * n)
        C.launch("gen", [(OP["MULSUB"], cnt, o + i, ia + i, ib + i, ic + i, n, 1) for i in range(n)],
                 ["a=%s b=%s c=%s cnt=%d" % (_h(a[i]), _h(b[i]), _h(b[n - 1 - i]), cnt) for i in range(n)])
    o, mir = C.out(2 * n), C.out(n)
    C.launch("gen", [(OP["DIV"], 2, o + i, ia + i, ib + i, mir + i, n, 1) for i in range(n)], ["a=%s b=%s cnt=2 mirror" % (_h(a[i]), _h(b[i])) for i in range(n)])
    o = C.out(n)
    C.launch("gen", [(OP["HDIFF"], 1, o + i, ia + i, 0, 0, 1, 1) for i in range(n)], ["a=%s" % _h(v) for v in a])
    # DIVB: the program guarantees |a| <= |b|
    mag = lambda v: abs(wm.s(v, 64))
    pa, pb = zip(*[(x, y) if mag(x) <= mag(y) else (y, x) for x, y in zip(a, b)])
    ja, jb = C.inp(pa), C.inp(pb)
    o = C.out(n)
    C.launch("gen", [(OP["DIVB"], 1, o + i, ja + i, jb + i, 0, 1, 1) for i in range(n)], ["a=%s b=%s" % (_h(pa[i]), _h(pb[i])) for i in range(n)])


def sec_ip(C, rng, n_rand):
    w = C.w
    v = [int(x) for x in edge_operands(rng, w, 40)[0][::4]]
    n = len(v)
    iv = C.inp(v)
    accs, recs, descs = [], [], []
    for cnt, sa, start in ((1, 1, 0), (3, 1, 2), (8, -1, n - 1), (20, 2, 1)):
        o = C.out(4)
        accs.append(o)
        recs.append((OP["IPMAC"], cnt, o, iv + start, iv + n - 1 - start, 0, sa, -sa))
        descs.append("cnt=%d sa=%d" % (cnt, sa))
    C.launch("gen", recs, descs)
    m = C.out(4)
    C.launch("gen", [(OP["IPMERGE"], 2, m, accs[0], 0, 0, 1, 1)], ["cnt=2"])
    o = C.out(3)
    C.launch("gen", [(OP["IPFIN"], 1, o, accs[3], 0, 0, 1, 1), (OP["IPFIN"], 2, o + 1, accs[2], 0, 0, 1, 1),
                     (OP["IPFIN"], 1, o + 2, m, 0, 0, 1, 1)], ["cnt=1", "cnt=2", "of IPMERGE"])


def sec_lasso(C, rng, n_rand):
    w, p = C.w, C.p
    mdl = wm.Model(None, w, p)
    # STEPEXP: row-sum magnitudes of every bit length, lambda values, c = ceil(log2 d)
    ms = [0, 1, 2, 3, (1 << (w - 1)) - 1, 1 << (w - 1), wm.mask(w)] + \
        [int(x) >> int(k) for x, k in zip(rng.integers(0, 1 << 62, 8, dtype=np.uint64), rng.integers(0, 62, 8))]
    ms = [x & wm.mask(w) for x in ms]
    lam = [int(x) & ((1 << (w - 2)) - 1) for x in rng.integers(0, 1 << 62, len(ms), dtype=np.uint64)]
    im, il = C.inp(ms), C.inp(lam)
    recs, descs = [], []
    for c in (0, 1, 9, min(p + 2, w - 2)):
        for i in range(len(ms)):
            o = C.out(3)
            recs.append((OP["STEPEXP"], 1, o, im + i, il + i, c, 1, 1))
            descs.append("m=%s lambda=%s c=%d" % (_h(ms[i]), _h(lam[i]), c))
    C.launch("gen", recs, descs)
    # PROX: shift words of steps 2^(p - l) both ways, theta >= 0 with -theta, momentum constants; x_i, y_i updated in place
    a, b = _pairs(C, rng, n_rand)
    recs, descs = [], []
    for i, ell in enumerate((0, max(p - 3, 0), p, p + 1, p + 7, 2 * w)):
        theta = [0, 1, int(rng.integers(0, 1 << (w - 2))), (1 << (w - 1)) - 1][i % 4]
        E = C.inp([mdl.step_word(ell), theta, wm.u(-theta, w)])
        for j, coef in enumerate((0, 1, (1 << p) - 1, int(rng.integers(0, 1 << max(p, 1))))):
            k = (7 * i + 13 * j) % len(a)
            g = C.inp([a[k], b[k]])                                        # (M y)_i, b_i
            x = C.inp([b[(k + 1) % len(b)], a[(k + 3) % len(a)]])            # x_i, y_i
            sb = (C.out() - (x + 1)) if (w == 64 and j % 2) else 0          # hdiff(y_i') in a word of its own
            recs.append((OP["PROX"], (coef >> 32) & M32, x, g, coef & M32, E, 1, sb))
            descs.append("g=(%s - %s) x=%s y=%s ell=%d theta=%s coef=%s" % (_h(a[k]), _h(b[k]), _h(b[(k + 1) % len(b)]),
                                                                         _h(a[(k + 3) % len(a)]), ell, _h(theta), _h(coef)))
    C.launch("gen", recs, descs)


def _mac_vector(C, rng):
    v = [int(x) for x in edge_operands(rng, C.w, 520)[0][::13]]
    v += [int(x) for x in edge_operands(rng, C.w, 600)[1][196:]]
    return v, C.inp(v)


MAC_SHAPES = ((1, 1, 1), (2, 1, -1), (3, -1, 2), (17, -2, -3), (500, 1, -1))


def _mac_recs(C, op, v, iv, delta=0):
    n = len(v)
    recs, descs = [], []
    for cnt, sa, sb in MAC_SHAPES:
        cnt = min(cnt, 250) if op == "MAC2" else cnt      # (2 cnt products)
        span = (2 * cnt if op == "MAC2" else cnt) - 1
        a0 = iv + (0 if sa > 0 else -sa * span)
        b0 = iv + (n - 1 - sb * span if sb > 0 else n - 1)
        assert iv <= a0 + span * sa < iv + n and iv <= b0 + span * sb < iv + n and b0 < iv + n and a0 < iv + n
        o = C.out(4 if op == "MAC2" else 2)
        recs.append((OP[op], cnt, o, a0, b0, delta, sa, sb))
        descs.append("cnt=%d sa=%d sb=%d" % (cnt, sa, sb))
    return recs, descs


def sec_mac(C, rng, n_rand):
    v, iv = _mac_vector(C, rng)
    C.launch("mac", *_mac_recs(C, "MAC", v, iv))


def sec_mac2(C, rng, n_rand):
    v, iv = _mac_vector(C, rng)
    C.launch("mac", *_mac_recs(C, "MAC2", v, iv))


def sec_mack(C, rng, n_rand):
    v, iv = _mac_vector(C, rng)
    hd = C.out(len(v))
    C.launch("gen", [(OP["HDIFF"], 1, hd + i, iv + i, 0, 0, 1, 1) for i in range(len(v))], ["a=%s" % _h(x) for x in v])
    C.launch("mack", *_mac_recs(C, "MACK", v, iv, hd - iv))


SECTIONS = [("binary", sec_binary), ("unary", sec_unary), ("sums", sec_sums), ("side", sec_side), ("ip", sec_ip),
            ("lasso", sec_lasso), ("mac", sec_mac), ("mac2", sec_mac2), ("mack", sec_mack)]
ONLY64_SECTIONS = {"side", "mack"}
ONLY32_SECTIONS = {"mac2"}


def plain_words(gccpu, prog, C):
    """the decode slots of `prog` (C's program) on the plaintext machine of the CPU checker"""
    words = np.zeros(prog.info.n_words, dtype=np.uint64)
    words[:len(C.inputs) + 1] = [0] + C.inputs
    dec = np.zeros(prog.info.n_reveal + 1, dtype=np.uint64)
    gccpu.plain_run(prog.records(), prog.info.n_records, C.w, C.p, words, dec)
    return [int(v) & wm.mask(C.w) for v in dec[:prog.info.n_reveal]]


def model_words(oracle, C):
    """the decode slots by the integer model, with its carry-save and opaque words"""
    _, dec, cs, opaque = wm.run(oracle, C.records(), C.words0(), C.w, C.p, C.next_out)
    return dec, cs, opaque


def mismatches(C, got, want, cs=(), opaque=(), limit=8):
    """messages for the slots where got differs from want; cs: carry-save pairs (x, x + 1) compared as their sum mod 2^w,
    opaque: slots not compared"""
    out = []
    m = wm.mask(C.w)
    skip = set(opaque) | {x + 1 for x in cs}
    for i in range(len(want)):
        if i in skip:
            continue
        g, e = (got[i] + got[i + 1]) & m if i in cs else got[i], want[i]
        if g != e:
            out.append("word %d (%s): got 0x%x, expected 0x%x" % (i, C.desc.get(i, "input"), g, e))
            if len(out) >= limit:
                break
    return out
