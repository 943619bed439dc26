"""Closed-form count of the AES lookup instructions (ds_read_b32, per wave) of the OP_MACK launches of a program: 160 per
hash everywhere but in the partial-product rows of the 32 x 32 arrays, where operand a's hashes cost 133 (160 in rows 0
and 1 of an array and in a row that follows a multiple of 512 gate steps: gc_aes.h row_hash) and operand b's 135 (hash_lu).
Host only.  usage: mack_lookup_count.py [d [iters [width [precision]]]]   (default: the benchmark's solve, 500 15 64 56)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "linreg-mpc_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import linreg_gc as lgc   # noqa: E402
from word_model import OP   # noqa: E402  (the op numbers of gc_exec.h)


def main():
    a = [int(x) for x in sys.argv[1:]]
    d, iters, w, p = (a + [500, 15, 64, 56][len(a):])[:4]
    sysm = lgc.make_system(d, w, p, "cgd", iters, 0.0, 2, 0, 0, 0)      # the benchmark's system
    prog = lgc.Program(sysm)
    raw = np.frombuffer(prog.records(), dtype=np.uint8).reshape(-1, 40)
    op = raw[:, 0:4].copy().view(np.uint32).reshape(-1)
    cnt = raw[:, 4:8].copy().view(np.uint32).reshape(-1)
    step0 = raw[:, 32:40].copy().view(np.uint64).reshape(-1).astype(object)
    seen = {}
    for i, L in enumerate(prog.launches()):
        f, n = L["first_rec"], L["nrec"]
        if n == 0 or not (op[f:f + n] == OP["MACK"]).all():
            continue
        pairs = (cnt[f:f + n].astype(np.int64) + 1) // 2
        per_pair, rem = divmod(int(L["steps"]), int(pairs.sum()))
        assert rem == 0 and per_pair >= 3 * 63, (i, per_pair, rem)
        starts = np.concatenate([int(step0[f + k]) + per_pair * np.arange(pairs[k]) for k in range(n)])
        starts = (starts[:, None] + 63 * np.arange(3)[None, :]).reshape(-1)
        fills = 2 + ((starts + 61) // 512 != (starts + 1) // 512)
        rows_saved = int((32 - fills).sum())
        for role, nh in (("garbler", 2), ("evaluator", 1)):
            parent = int(L["steps"]) * 2 * nh * 160
            saved = nh * (27 * rows_saved + 25 * 32 * len(starts))
            key = (role, int(L["steps"]), parent, saved)
            seen.setdefault(key, []).append(i)
    for (role, steps, parent, saved), ls in sorted(seen.items(), key=lambda kv: kv[1][0]):
        print("%-9s launches %s: %d steps, %d lookups at 160 per hash, %d saved (%.2f %%) -> %d"
              % (role, ls if len(ls) < 4 else "%d..%d (%d)" % (ls[0], ls[-1], len(ls)), steps, parent, saved,
                 100.0 * saved / parent, parent - saved))


if __name__ == "__main__":
    main()
