"""An independent integer model of the garbled word machine's record ops (gc_exec.h), in Python integers.

Written from the op definitions, not from the circuits: mul, div, sqrt and the compare come from the semantic oracle
(orc.py, a restatement of the reference), the lasso pieces from lasso_model.py.  Words are unsigned w-bit integers.

Records are (op, cnt, dst, a, b, c, sa, sb) tuples.  `run` interprets a list of them on a word file.  A multiply-accumulate
leaves its result in carry-save form, two words whose split is the circuit's own; the model stores the sum in the first
word and 0 in the second, and `cs_pairs` tells a comparison which words to add before it compares.  The four words of an
inner-product accumulator (OP_IPMAC / OP_IPMERGE) have no model of their own: the model keeps the exact sum aside and
checks it through the OP_IPFIN that consumes it; `opaque` lists those words.
"""
import lasso_model as lm

OPS = ["NOP", "MAC", "SUM", "SUBSUM", "IPMAC", "IPFIN", "IPMERGE", "MUL", "MULSUB", "ADD", "SUB", "ABS", "MAX", "DIV", "SQRT",
       "IDIVC", "CONST", "COPY", "REVEAL", "MAC2", "MACK", "HDIFF", "EQ", "DIVB", "ABSSUM", "STEPEXP", "PROX"]
OP = {n: i for i, n in enumerate(OPS)}
ONLY64 = {OP["MACK"], OP["HDIFF"], OP["DIVB"]}
ONLY32 = {OP["MAC2"]}


def mask(w):
    return (1 << w) - 1


def s(v, w):
    """the signed value of a w-bit word"""
    return lm.wrap(int(v), w)


def u(v, w):
    """a signed or unsigned integer as a w-bit word"""
    return int(v) & mask(w)


class Model:
    def __init__(self, oracle, w, p):
        self.orc, self.w, self.p = oracle, w, p

    # ---- word ops on signed values, results as words
    def mul(self, a, b):
        return u(self.orc.mul(s(a, self.w), s(b, self.w), self.p, self.w), self.w)

    def div(self, a, b):
        return u(self.orc.div(s(a, self.w), s(b, self.w), self.p, self.w), self.w)

    def sqrt(self, a):
        return u(self.orc.sqrt(s(a, self.w), self.p, self.w), self.w)

    def gt(self, a, b):
        """Circ::gt: signed at w = 32, unsigned at w = 64 (obig_cmp)"""
        return self.orc.cmp(s(a, self.w), s(b, self.w), self.w) > 0

    def add(self, a, b):
        return u(a + b, self.w)

    def sub(self, a, b):
        return u(a - b, self.w)

    def abs(self, a):
        return u(abs(s(a, self.w)), self.w)

    @staticmethod
    def hdiff(v):
        """|hi32 - lo32| in lanes 0..31, [hi32 < lo32] in lane 32"""
        hi, lo = (v >> 32) & 0xFFFFFFFF, v & 0xFFFFFFFF
        return abs(hi - lo) | ((1 << 32) if hi < lo else 0)

    def tdiv(self, a, c):
        """tdiv(a, c) for a public c >= 1: truncation toward zero"""
        x = s(a, self.w)
        q = abs(x) // c
        return u(-q if x < 0 else q, self.w)

    def ip_final(self, total):
        """wrap_w(sum >> p) of an exact sum of products"""
        return u(total >> self.p, self.w)

    def step_word(self, ell):
        """the shift word of a step 2^(p - ell) as Circ::stepexp forms it: L in lanes 0.., min(R, w - 1) in lanes 8.."""
        L, R = max(self.p - ell, 0), min(max(ell - self.p, 0), self.w - 1)
        return L | (R << 8)

    def step_shift(self, v, E):
        """v shifted by the shift word E: left by its L (mod 2^w), then arithmetically right by its R"""
        lg = 6 if self.w == 64 else 5
        L, R = E & ((1 << lg) - 1), (E >> 8) & ((1 << lg) - 1)
        return u(s(v << L, self.w) >> R, self.w)

    # ---- one record
    def exec(self, r, W, dec, acc, cs, opaque):
        op, cnt, dst, a, b, c, sa, sb = [int(x) for x in r]
        w, M32 = self.w, 0xFFFFFFFF
        at = lambda base, k, st: (base + k * st) & M32
        name = OPS[op]
        if name in ("MAC", "MACK"):
            tot = sum(s(self.mul(W[at(a, k, sa)], W[at(b, k, sb)]), w) for k in range(cnt))
            W[dst], W[dst + 1] = u(tot, w), 0
            cs.add(dst)
        elif name == "MAC2":
            for h in range(2):
                tot = sum(s(self.mul(W[at(a, h * cnt + k, sa)], W[at(b, h * cnt + k, sb)]), w) for k in range(cnt))
                W[dst + 2 * h], W[dst + 2 * h + 1] = u(tot, w), 0
                cs.add(dst + 2 * h)
        elif name == "HDIFF":
            W[dst] = self.hdiff(W[a])
        elif name == "EQ":
            W[dst] = int(W[a] == W[b])
        elif name in ("SUM", "SUBSUM"):
            v = u(sum(W[at(a, k, sa)] for k in range(cnt)), w)
            W[dst] = self.sub(W[c], v) if name == "SUBSUM" else v
        elif name == "IPMAC":
            acc[dst] = sum(s(W[at(a, k, sa)], w) * s(W[at(b, k, sb)], w) for k in range(cnt))
            for i in range(4):
                W[dst + i] = 0
                opaque.add(dst + i)
        elif name in ("IPFIN", "IPMERGE"):
            tot = sum(acc[a + 4 * k] for k in range(cnt))
            if name == "IPFIN":
                W[dst] = self.ip_final(tot)
            else:
                acc[dst] = tot
                for i in range(4):
                    W[dst + i] = 0
                    opaque.add(dst + i)
        elif name == "MUL":
            W[dst] = self.mul(W[a], W[b])
            if cnt == 2:
                W[(dst + sa) & M32] = self.hdiff(W[dst])
        elif name == "MULSUB":
            W[dst] = self.sub(W[c], self.mul(W[a], W[b]))
            if cnt == 2:
                W[(dst + sa) & M32] = self.abs(W[dst])
            elif cnt == 3:
                W[(dst + sa) & M32] = self.hdiff(W[dst])
        elif name == "ADD":
            W[dst] = self.add(W[a], W[b])
        elif name == "SUB":
            W[dst] = self.sub(W[a], W[b])
        elif name == "ABS":
            W[dst] = self.abs(W[a])
        elif name == "MAX":
            vals = [W[at(a, k, sa)] for k in range(cnt)]
            m = vals[0]
            for v in vals[1:]:
                if (v > m) if b else self.gt(v, m):
                    m = v
            W[dst] = m
        elif name in ("DIV", "DIVB"):
            W[dst] = self.div(W[a], W[b])
            if name == "DIV" and c:
                W[c] = W[dst]
            if name == "DIV" and cnt == 2:
                W[(dst + sa) & M32] = self.hdiff(W[dst])
        elif name == "SQRT":
            W[dst] = self.sqrt(W[a])
        elif name == "IDIVC":
            W[dst] = self.tdiv(W[a], c)
        elif name == "CONST":
            W[dst] = u(a | (b << 32), w)
        elif name == "COPY":
            W[dst] = W[a]
        elif name == "REVEAL":
            dec[dst] = W[a]
        elif name == "ABSSUM":
            W[dst] = u(sum(abs(s(W[at(a, k, sa)], w)) >> c for k in range(cnt)), w)
        elif name == "STEPEXP":
            ell = c + W[a].bit_length()
            theta = u(lm.step(s(W[b], w), ell, w, self.p), w)
            W[dst], W[dst + 1], W[dst + 2] = self.step_word(ell), theta, u(-s(theta, w), w)
        elif name == "PROX":
            yi = (dst + sa) & M32
            g = self.sub(W[a], W[(a + sa) & M32])
            z = self.sub(W[yi], self.step_shift(g, W[c]))
            assert W[c + 2] == u(-s(W[c + 1], w), w) and s(W[c + 1], w) >= 0, "PROX needs theta >= 0 and -theta"
            xn = u(lm.soft(s(z, w), s(W[c + 1], w), w), w)
            dx = self.sub(xn, W[dst])
            coef = b | (cnt << 32)
            yn = self.add(xn, u(s(dx, w) * coef >> self.p, w))
            W[dst], W[yi] = xn, yn
            if sb:
                W[(yi + sb) & M32] = self.hdiff(yn)
        elif name == "NOP":
            pass
        else:
            raise ValueError("no model for op %d" % op)


def run(oracle, records, words, w, p, n_reveal):
    """interpret `records` on a copy of `words` (unsigned w-bit ints); returns (words, decode slots, cs_pairs, opaque)"""
    m = Model(oracle, w, p)
    W = [int(v) & mask(w) for v in words]
    dec = [0] * n_reveal
    acc, cs, opaque = {}, set(), set()
    for r in records:
        m.exec(r, W, dec, acc, cs, opaque)
        # a word written by a later record is no longer carry-save or opaque
        op, dst = int(r[0]), int(r[2])
        if OPS[op] not in ("MAC", "MACK", "MAC2", "IPMAC", "IPMERGE", "REVEAL"):
            cs.discard(dst)
            opaque.discard(dst)
    return W, dec, cs, opaque
