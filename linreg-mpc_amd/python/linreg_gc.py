"""ctypes binding of the product C ABI (include/linreg_gc.h, liblinreg_gc.so).

This is plumbing above the C ABI; all compute happens in the HIP library.
There is no CPU fallback: `Solver` raises `LgcError` (LGC_ENODEVICE) when no
MI355X is visible, and importing fails loudly when the library is not built.
"""
import ctypes as C
import functools
import os
import types

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LGC_LIB") or os.path.join(os.path.dirname(_HERE), "csrc", "liblinreg_gc.so")

ALG = {"cholesky": 0, "ldlt": 1, "cgd": 2, "dimcheck": 3,   # dimcheck: the two parties' dimension comparison (src/linear.oc:109-114), not a solver
       "lasso": 4}                                          # lasso / elastic net (include/linreg_gc_lasso.h): needs l1=


class LgcError(RuntimeError):
    def __init__(self, code, msg):
        RuntimeError.__init__(self, "lgc error %d: %s" % (code, msg))
        self.code = code


class System(C.Structure):
    """counterpart of linear_system_t (reference src/linear.h:16-26)"""
    _fields_ = [("d", C.c_size_t), ("width", C.c_int), ("precision", C.c_int), ("algorithm", C.c_int),
                ("num_iterations", C.c_int), ("lam", C.c_double), ("nshares", C.c_size_t),
                ("normalize", C.c_int), ("reveal_inputs", C.c_int), ("trace", C.c_int)]


class Stats(C.Structure):
    _fields_ = [("and_gates", C.c_uint64), ("gate_steps", C.c_uint64), ("table_bytes", C.c_uint64),
                ("launches", C.c_uint64), ("seconds_total", C.c_double), ("seconds_garble", C.c_double),
                ("seconds_eval", C.c_double), ("seconds_mac_garble", C.c_double), ("seconds_mac_eval", C.c_double),
                ("mac_gates", C.c_uint64), ("mac_launches", C.c_uint64)]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class Record(C.Structure):
    _fields_ = [("op", C.c_uint32), ("cnt", C.c_uint32), ("dst", C.c_uint32), ("a", C.c_uint32),
                ("b", C.c_uint32), ("c", C.c_uint32), ("sa", C.c_int32), ("sb", C.c_int32), ("step0", C.c_uint64)]


class LassoOpts(C.Structure):
    """struct lgc_lasso_opts (include/linreg_gc_lasso_opts.h)"""
    _fields_ = [("l1_count", C.c_size_t), ("l1", C.c_void_p), ("l1_mode", C.c_int), ("penalty_factors", C.c_void_p),
                ("lower", C.c_void_p), ("upper", C.c_void_p)]


class Launch(C.Structure):
    _fields_ = [("first_rec", C.c_uint32), ("nrec", C.c_uint32), ("step0", C.c_uint64), ("steps", C.c_uint64),
                ("gates", C.c_uint64), ("mac_only", C.c_int)]


class ProgramInfo(C.Structure):
    _fields_ = [("n_records", C.c_size_t), ("n_launches", C.c_size_t), ("n_words", C.c_uint32),
                ("n_reveal", C.c_uint32), ("in_base", C.c_uint32), ("rv_beta", C.c_uint32),
                ("rv_trace", C.c_uint32), ("rv_inputs", C.c_uint32), ("total_steps", C.c_uint64),
                ("total_gates", C.c_uint64), ("max_launch_steps", C.c_uint64),
                ("replicas", C.c_uint32), ("word_stride", C.c_uint32), ("reveal_stride", C.c_uint32),
                ("shared_end", C.c_uint32), ("prefix_launches", C.c_uint32), ("prefix_steps", C.c_uint64),
                ("total_xors", C.c_uint64)]


# The creation calls.  A program kind is the suffix of its C call -- lgc_program_build<kind>, lgc_solver_create<kind>,
# lgc_party_create<kind> -- and the three calls of a kind differ in their leading arguments only: kind -> the argtypes behind
# the lead.  (_sweep is _sweep_at with first = 0; the binding itself calls _sweep_at.)
_sz, _ci, _vp_t, _opts_p = C.c_size_t, C.c_int, C.c_void_p, C.POINTER(LassoOpts)
_KINDS = {
    "": [],                                                 # one solve (include/linreg_gc.h)
    "_sweep": [_sz, _vp_t], "_sweep_at": [_sz, _vp_t, _sz],  # count, lambdas[, first] (include/linreg_gc_sweep.h)
    "_targets": [_sz],                                      # k (include/linreg_gc_targets.h)
    "_lasso": [C.c_double],                                 # lambda1 (include/linreg_gc_lasso.h)
    "_lasso_path": [_sz, _vp_t, _ci],                       # count, values, mode (include/linreg_gc_lasso_path.h)
    "_lasso_opts": [_opts_p],                               # (include/linreg_gc_lasso_opts.h)
    "_lasso_select": [_opts_p, _ci],                        # options, reveal (include/linreg_gc_lasso_select.h)
    "_lasso_cv": [_opts_p, _sz, _ci],                       # options, folds, reveal (include/linreg_gc_lasso_cv.h)
    "_lasso_cv_se": [_opts_p, _sz, _ci, _ci],               # options, folds, reveal, rule (include/linreg_gc_lasso_cv_se.h)
    "_ridge_cv": [_sz, _vp_t, _sz, _ci],                    # count, lambdas, folds, reveal (include/linreg_gc_ridge_cv.h)
    "_inference": [C.c_double, _ci],                        # resid_scale, reveal (include/linreg_gc_inference.h)
    "_scan": [_sz, C.c_double, _ci],                        # M, resid_scale, flags (include/linreg_gc_scan.h)
}
_LEADS = {
    "lgc_program_build": [C.POINTER(_vp_t), C.POINTER(System)],                               # out, system
    "lgc_solver_create": [C.POINTER(_vp_t), _ci, C.POINTER(System), C.c_char_p],              # out, device, system, seed
    "lgc_party_create": [C.POINTER(_vp_t), _ci, C.POINTER(System), _ci, C.c_char_p, _sz],     # .., role, seed, max_launch_table_bytes
}

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("HIP extension missing: %s (run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "or `make -C linreg-mpc_amd/csrc`)" % LIB_PATH)
        # A process that also uses torch on the GPU must import torch BEFORE this library is loaded: torch ships
        # its own libamdhip64 under the same SONAME and whichever loads first serves both (bench.py, tests/conftest.py)
        L = C.CDLL(LIB_PATH)
        vp, ci, sz = C.c_void_p, C.c_int, C.c_size_t
        L.lgc_last_error.restype = C.c_char_p
        L.lgc_version.restype = C.c_char_p
        L.lgc_device_count.restype = ci
        creation = [(prefix + kind, lead + tail) for prefix, lead in _LEADS.items() for kind, tail in _KINDS.items()
                    if not (prefix == "lgc_party_create" and kind.startswith("_sweep"))]   # (the library has no party of a plain sweep)
        for name, args in creation + [
            ("lgc_solver_set_shares", [vp, vp]), ("lgc_solver_run", [vp, ci]),
            ("lgc_solver_get_beta", [vp, vp]), ("lgc_solver_get_trace", [vp, vp]),
            ("lgc_solver_get_inputs", [vp, vp]), ("lgc_solver_get_stats", [vp, C.POINTER(Stats)]),
            ("lgc_solver_get_profile", [vp, vp, vp, sz]), ("lgc_solver_get_iterations", [vp, vp, vp, sz]),
            ("lgc_party_iteration_marks", [vp, vp, vp, sz]),
            ("lgc_solver_prefix_garble", [vp]), ("lgc_solver_prefix_export", [vp, vp]), ("lgc_solver_prefix_import", [vp, vp]),
            ("lgc_program_info_get", [vp, C.POINTER(ProgramInfo)]),
            ("lgc_program_ring_plan", [vp, sz, C.POINTER(sz), vp, vp]),
            ("lgc_aes_bench", [ci, ci, ci, C.POINTER(C.c_double), C.POINTER(C.c_uint32)]),
            ("lgc_p1_create", [C.POINTER(vp), ci, sz, sz, ci, ci]), ("lgc_p1_set_data", [vp, vp, vp]),
            ("lgc_p1_local", [vp, sz, sz, ci, vp, vp]), ("lgc_p1_mask", [vp, vp, sz, vp, ci, vp]),
            ("lgc_p1_dot", [vp, vp, vp, vp, sz, vp, vp]),
            ("lgc_p1_ti_a", [vp, C.c_uint32, vp, vp, C.c_uint64, vp, C.POINTER(C.c_uint64)]),
            ("lgc_ti_generate", [ci, C.c_char_p, C.c_uint64, sz, sz, ci, vp, vp, vp, vp]),
            ("lgc_party_input_pairs", [vp, sz, vp, vp]), ("lgc_party_encode_inputs", [vp, sz, vp, vp]),
            ("lgc_party_set_input_labels", [vp, sz, vp]), ("lgc_party_garble", [vp, sz, vp]),
            ("lgc_party_evaluate", [vp, sz, vp]), ("lgc_party_decode_bits", [vp, vp]),
            ("lgc_party_finish", [vp, vp, vp, vp, vp]), ("lgc_party_program_fingerprint", [vp, vp]),
            ("lgc_party_ring_create", [vp, ci, vp, C.POINTER(sz)]), ("lgc_party_ring_open", [vp, vp, ci, sz]),
            ("lgc_party_garble_ring", [vp, sz]), ("lgc_party_evaluate_ring", [vp, sz]),
            ("lgc_party_garble_ring_begin", [vp, sz]), ("lgc_party_garble_ring_wait", [vp, sz]),
            ("lgc_party_garble_ring_streams", [vp, C.c_int]),
            ("lgc_test_party_garble_ring_stage", [vp, sz, ci, C.POINTER(ci)]), ("lgc_test_party_ring_read", [vp, sz, vp, sz]),
            ("lgc_ot_sender_create", [C.POINTER(vp), ci, C.c_char_p, vp]),
            ("lgc_ot_receiver_create", [C.POINTER(vp), ci, vp, vp]),
            ("lgc_ot_sender_set_device_io", [vp, ci]), ("lgc_ot_receiver_set_device_io", [vp, ci]),
            ("lgc_ot_gilboa_recv_start", [vp, vp, sz, sz, ci, vp]),
            ("lgc_ot_gilboa_send", [vp, vp, sz, sz, ci, vp, vp, vp]),
            ("lgc_ot_gilboa_recv_finish", [vp, vp, vp]),
            ("lgc_ot_labels_recv_start", [vp, vp, sz, vp]), ("lgc_ot_labels_send", [vp, vp, vp, sz, vp, vp]),
            ("lgc_ot_labels_recv_finish", [vp, vp, vp]),
            ("lgc_aes_encrypt", [ci, vp, vp, sz]),
            # several targets in one solve (include/linreg_gc_targets.h)
            ("lgc_p1_create_targets", [C.POINTER(vp), ci, sz, sz, sz, ci, ci]), ("lgc_p1_set_targets", [vp, vp, vp]),
            ("lgc_p1_local_targets", [vp, sz, sz, vp, vp]),
            # the words yy of the folds (include/linreg_gc_lasso_cv_se.h) and of the whole (include/linreg_gc_inference.h)
            ("lgc_p1_local_folds_yy", [vp, sz, sz, sz, vp, vp, vp]), ("lgc_p1_local_yy", [vp, sz, sz, vp, vp, vp]),
            # an association scan: M candidate columns against shared covariates (include/linreg_gc_scan.h)
            ("lgc_p1_set_divisor", [vp, sz]), ("lgc_p1_local_scan", [vp, sz, sz, sz, sz, ci, vp, vp, vp]),
            # phase 1 on row folds (include/linreg_gc_folds.h)
            ("lgc_fold_rows", [sz, sz, sz, C.POINTER(sz), C.POINTER(sz)]),
            ("lgc_p1_set_rows", [vp, sz, sz]), ("lgc_p1_local_folds", [vp, sz, sz, ci, sz, vp, vp]),
            ("lgc_p1_ti_a_batch", [vp, vp, sz, vp, vp, vp, vp, vp]),
            # one matrix triple per provider pair under the trusted initializer (include/linreg_gc_p1_matrix.h)
            ("lgc_p1_set_device_io", [vp, ci]),
            ("lgc_p1_matrix_mask", [vp, vp, sz, C.c_char_p, vp]),
            ("lgc_p1_matrix_share_a", [vp, sz, C.c_char_p, C.c_char_p, vp, sz, vp]),
            ("lgc_p1_matrix_share_b", [vp, vp, sz, vp, sz, vp, vp]),
            ("lgc_ti_matrix_generate", [ci, C.c_char_p, C.c_char_p, C.c_char_p, sz, sz, sz, ci, vp]),
            ("lgc_ti_matrix_seeds", [C.c_char_p, C.c_uint64, vp, vp, vp]),
        ] + [
            # Gilboa with one vector OT per operand bit (include/linreg_gc_ot_matrix.h) and its half-payload form
            # (include/linreg_gc_ot_half.h): the same signatures
            ("lgc_ot_gilboa_%s_%s" % (form, op), args) for form in _OT_BLOCK_FORMS
            for op, args in (("recv_start", [vp, vp, sz, sz, sz, ci, vp]), ("send", [vp, vp, sz, sz, sz, ci, vp, vp, vp]),
                             ("recv_finish", [vp, vp, vp]))
        ]:
            fn = getattr(L, name)
            fn.restype, fn.argtypes = ci, args
        L.lgc_set_split_kernels.argtypes = [ci, ci]; L.lgc_set_split_kernels.restype = None
        L.lgc_release_cached_memory.argtypes = []; L.lgc_release_cached_memory.restype = None
        L.lgc_solver_destroy.argtypes = [vp]; L.lgc_solver_destroy.restype = None
        L.lgc_solver_prefix_bytes.argtypes = [vp]; L.lgc_solver_prefix_bytes.restype = sz
        L.lgc_solver_num_targets.argtypes = [vp]; L.lgc_solver_num_targets.restype = sz
        L.lgc_solver_path_length.argtypes = [vp]; L.lgc_solver_path_length.restype = sz
        L.lgc_solver_num_folds.argtypes = [vp]; L.lgc_solver_num_folds.restype = sz
        L.lgc_solver_selected_index.argtypes = [vp]; L.lgc_solver_selected_index.restype = C.c_int64
        L.lgc_party_selected_index.argtypes = [vp]; L.lgc_party_selected_index.restype = C.c_int64
        L.lgc_solver_min_index.argtypes = [vp]; L.lgc_solver_min_index.restype = C.c_int64
        L.lgc_party_min_index.argtypes = [vp]; L.lgc_party_min_index.restype = C.c_int64
        L.lgc_program_destroy.argtypes = [vp]; L.lgc_program_destroy.restype = None
        L.lgc_p1_destroy.argtypes = [vp]; L.lgc_p1_destroy.restype = None
        L.lgc_party_destroy.argtypes = [vp]; L.lgc_party_destroy.restype = None
        for nme in ("lgc_party_num_launches", "lgc_party_input_bits", "lgc_party_num_reveal", "lgc_party_num_targets",
                    "lgc_party_path_length", "lgc_party_num_folds"):
            getattr(L, nme).argtypes = [vp]; getattr(L, nme).restype = sz
        L.lgc_party_table_bytes.argtypes = [vp, sz]; L.lgc_party_table_bytes.restype = sz
        L.lgc_party_and_gates.argtypes = [vp]; L.lgc_party_and_gates.restype = C.c_uint64
        L.lgc_ot_sender_destroy.argtypes = [vp]; L.lgc_ot_sender_destroy.restype = None
        L.lgc_ot_receiver_destroy.argtypes = [vp]; L.lgc_ot_receiver_destroy.restype = None
        L.lgc_ot_u_bytes.argtypes = [C.c_uint64]; L.lgc_ot_u_bytes.restype = sz
        L.lgc_ot_gilboa_matrix_y_bytes.argtypes = [sz, sz, sz, ci]; L.lgc_ot_gilboa_matrix_y_bytes.restype = sz
        L.lgc_ot_gilboa_half_y_bytes.argtypes = [sz, sz, sz, ci]; L.lgc_ot_gilboa_half_y_bytes.restype = sz
        L.lgc_program_records.argtypes = [vp]; L.lgc_program_records.restype = C.POINTER(Record)
        L.lgc_program_launches.argtypes = [vp]; L.lgc_program_launches.restype = C.POINTER(Launch)
        _lib = L
    return _lib


def _chk(rc):
    if rc != 0:
        raise LgcError(rc, lib().lgc_last_error().decode())


def _no_sweep_targets(lambdas, targets):
    # a lambda sweep of a multi-target system is not lowered (yet): one axis per program
    if lambdas is not None and targets is not None:
        raise LgcError(-1, "targets cannot be combined with a lambda sweep")


def _no_lasso_mix(lambdas, targets, l1):
    # lasso fits one target on one lambda2: the other axes are not lowered for it
    if l1 is not None and (lambdas is not None or targets is not None):
        raise LgcError(-1, "l1 (lasso) cannot be combined with a lambda sweep or with targets")


L1_ABSOLUTE, L1_RATIO = 0, 1                                # include/linreg_gc_lasso_path.h


def _l1_path(l1, l1_ratios):
    """(values, mode) of a lasso path, or None for a single lambda1 (a number) or no lasso at all.  l1: a number (one solve)
    or a sequence of lambda1 values (an absolute path); l1_ratios: a sequence of ratios of lambda_max (a ratio path)"""
    if l1 is not None and l1_ratios is not None:
        raise LgcError(-1, "l1 and l1_ratios exclude each other")
    if l1_ratios is not None:
        return np.ascontiguousarray(np.atleast_1d(np.asarray(l1_ratios, dtype=np.float64))), L1_RATIO
    if l1 is not None and np.ndim(l1) > 0:
        return np.ascontiguousarray(np.asarray(l1, dtype=np.float64).ravel()), L1_ABSOLUTE
    return None


SELECT_REVEAL_INDEX, SELECT_REVEAL_SCORES = 1, 2           # include/linreg_gc_lasso_select.h


def _select_flags(validation, reveal_index, reveal_scores, l1, l1_ratios, folds=None):
    """the LGC_SELECT_REVEAL_* word of validation=True or folds=K, or None with neither"""
    if validation and folds is not None:
        raise LgcError(-1, "validation=True (one hold-out) and folds=K (cross-validation) exclude each other")
    if not validation and folds is None:
        if reveal_index or reveal_scores:
            raise LgcError(-1, "reveal_index and reveal_scores belong to validation=True or folds=K")
        return None
    if l1 is None and l1_ratios is None:
        raise LgcError(-1, "%s selects among the models of a lasso path: it needs l1 or l1_ratios" % ("validation" if validation else "folds"))
    return (SELECT_REVEAL_INDEX if reveal_index else 0) | (SELECT_REVEAL_SCORES if reveal_scores else 0)


def _ridge_cv(system, lambdas, first, folds, validation, reveal_index, reveal_scores, rule, reveal_curve):
    """(values, K, LGC_SELECT_REVEAL_* word) of lambdas=[..] with folds=K -- the ridge sweep cross-validated in the circuit
    (include/linreg_gc_ridge_cv.h) -- or None when either is missing: every other combination is what it has always been"""
    if lambdas is None or folds is None:
        return None
    if validation:
        raise LgcError(-1, "validation=True (one hold-out) and folds=K (cross-validation) exclude each other")
    if int(system.algorithm) == ALG["lasso"]:
        raise LgcError(-1, "lambdas with folds cross-validates the ridge sweep of cgd, cholesky or ldlt: a lasso system takes l1 or l1_ratios with folds")
    if first:
        raise LgcError(-1, "first belongs to a sharded sweep: a cross-validation (folds=K) is one program, first must be 0")
    if rule is not None or reveal_curve:
        raise LgcError(-1, "rule and reveal_curve belong to the cross-validation of a lasso path")
    lam = np.ascontiguousarray(np.atleast_1d(np.asarray(lambdas, dtype=np.float64)).ravel())
    return lam, int(folds), (SELECT_REVEAL_INDEX if reveal_index else 0) | (SELECT_REVEAL_SCORES if reveal_scores else 0)


INFER_SE, INFER_FIT = 1, 2                                  # include/linreg_gc_inference.h
_INFER = {"se": INFER_SE, "fit": INFER_FIT}


def _inference(inference, resid_scale, **others):
    """(LGC_INFER_* word, resid_scale) of inference=("se", "fit") (any non-empty subset) with resid_scale=, or None without
    inference; `others`: the arguments of the other program kinds, none of which combines with it"""
    if inference is None:
        if resid_scale is not None:
            raise LgcError(-1, "resid_scale belongs to inference=")
        return None
    used = sorted(k for k, v in others.items() if v is not None and v is not False and v != 0)
    if used:
        raise LgcError(-1, "inference is a program of its own (one Cholesky solve): it does not combine with %s" % ", ".join(used))
    names = (inference,) if isinstance(inference, str) else tuple(inference)
    bad = [n for n in names if n not in _INFER]
    if bad:
        raise LgcError(-1, "unknown inference %r: a non-empty subset of (\"se\", \"fit\")" % (bad[0],))
    if resid_scale is None:
        raise LgcError(-1, "inference needs resid_scale= (n / (n - d) for the unbiased residual variance)")
    bits = 0
    for n in names:
        bits |= _INFER[n]
    return bits, float(resid_scale)


def _infer_split(words, d, bits):
    """(beta, u or None, s2 or None, r2 or None) of the words an inference program reveals"""
    words = np.asarray(words)
    k, u, s2, r2 = d, None, None, None
    if bits & INFER_SE:
        u = words[k:k + d].copy(); k += d
    if bits & INFER_FIT:
        s2, r2 = int(words[k]), int(words[k + 1])
    return words[:d].copy(), u, s2, r2


def _infer_summary(split, n, system):
    """floats of what an inference program revealed: se = u / sqrt(n), sigma2, r2 (None where not revealed).  On the
    data-provider path (normalize = 1) the system is the caller's divided by the public d, and so is s2: sigma2 = s2 d"""
    _, u, s2, r2 = split
    scale = float(1 << int(system.precision))
    unit = float(system.d) if int(system.normalize) else 1.0
    return dict(std_err=None if u is None else u.astype(np.float64) / scale / np.sqrt(float(n)),
                sigma2=None if s2 is None else s2 / scale * unit, r2=None if r2 is None else r2 / scale)


SCAN_SE = 1                                                 # include/linreg_gc_scan.h


def _scan(scan, scan_se, resid_scale, **others):
    """(M, LGC_SCAN_* word, resid_scale) of scan=M with scan_se= and resid_scale=, or None without scan; `others`: the
    arguments of the other program kinds, none of which combines with it"""
    if scan is None:
        if scan_se:
            raise LgcError(-1, "scan_se belongs to scan=M")
        return None
    used = sorted(k for k, v in others.items() if v is not None and v is not False and v != 0)
    if used:
        raise LgcError(-1, "a scan is a program of its own (one Cholesky factorisation, M candidates): it does not combine with %s" % ", ".join(used))
    if scan_se and resid_scale is None:
        raise LgcError(-1, "scan_se needs resid_scale= (n / (n - d) for the unbiased residual variance; d counts the candidate)")
    if not scan_se and resid_scale is not None:
        raise LgcError(-1, "resid_scale belongs to scan_se=True")
    if int(scan) < 0:
        raise LgcError(-1, "a scan takes 1..%d candidate columns (got %d)" % (1 << 20, int(scan)))
    return int(scan), SCAN_SE if scan_se else 0, float(resid_scale) if scan_se else 0.0


def _scan_in_words(system, M):
    """input words per share of a scan: [A (T_c)] [b (c)] [yy] [h_0 (c)] .. [h_{M-1} (c)] [gg (M)] [gy (M)], c = d - 1"""
    c = int(system.d) - 1
    return c * (c + 1) // 2 + c + 1 + M * (c + 2)


def _scan_summary(beta, w, n, system):
    """floats of what a scan revealed: beta, and std_err = w / sqrt(n) (None without scan_se)"""
    scale = float(1 << int(system.precision))
    return dict(beta=np.asarray(beta).astype(np.float64) / scale,
                std_err=None if w is None else np.asarray(w).astype(np.float64) / scale / np.sqrt(float(n)))


SELECT_REVEAL_CURVE = 4                                     # include/linreg_gc_lasso_cv_se.h
CV_RULE = {"min": 0, "1se": 1}


def _cv_rule(rule, reveal_curve, folds):
    """LGC_CV_RULE_* of rule= / reveal_curve= (the calls of linreg_gc_lasso_cv_se.h: every share ends with K words yy_k), or
    None with neither: the calls of linreg_gc_lasso_cv.h"""
    if rule is None and not reveal_curve:
        return None
    if folds is None:
        raise LgcError(-1, "rule and reveal_curve belong to folds=K")
    if rule is not None and rule not in CV_RULE:
        raise LgcError(-1, "unknown rule %r: \"min\" or \"1se\"" % (rule,))
    return CV_RULE[rule or "min"]


def _lasso_opts(system, l1, l1_ratios, positive, lower, upper, penalty_factors, always=False):
    """the struct lgc_lasso_opts of positive= / lower= / upper= / penalty_factors= (each list d long; +-inf: no bound on that
    side), or None when none is given (always: the struct even then).  positive: lower = 0 and no upper bound, and
    excludes lower"""
    if not always and not positive and lower is None and upper is None and penalty_factors is None:
        return None
    if positive and lower is not None:
        raise LgcError(-1, "positive and lower exclude each other (positive is lower = 0)")
    if l1 is None and l1_ratios is None:
        raise LgcError(-1, "positive, lower, upper and penalty_factors are options of the lasso: they need l1 or l1_ratios")
    d = int(system.d)
    if positive:
        lower = np.zeros(d)
    keep = []

    def arr(v, name):
        if v is None:
            return None
        a = np.ascontiguousarray(np.asarray(v, dtype=np.float64).ravel())
        if a.size != d:
            raise LgcError(-1, "%s needs d = %d entries (got %d)" % (name, d, a.size))
        keep.append(a)
        return a.ctypes.data
    path = _l1_path(l1, l1_ratios)
    values, mode = path if path is not None else (np.array([float(l1)]), L1_ABSOLUTE)
    keep.append(values)
    o = LassoOpts(values.size, values.ctypes.data, mode, arr(penalty_factors, "penalty_factors"), arr(lower, "lower"),
                  arr(upper, "upper"))
    o._keep = keep                                # (the arrays live as long as the struct)
    return o


def _trace_width(system):
    """words per trace row: cgd reveals x, gamma, eta, q, ng (cgd.oc:167-189), lasso x"""
    return int(system.d) + (0 if int(system.algorithm) == ALG["lasso"] else 4)


def _iterative(system):
    return int(system.algorithm) in (ALG["cgd"], ALG["lasso"])


def _in_words(system, targets, validation=False, folds=None, yy=False, infer=False):
    """input words per share: A (packed lower triangle), then b_0 .. b_{k-1}; with a validation system then A_v and b_v; with
    K folds K systems [A_k, b_k]; yy: then the K words yy_k; infer: [A, b, yy], one word yy"""
    d = int(system.d)
    if infer:
        return d * (d + 1) // 2 + d + 1
    return (d * (d + 1) // 2 + (targets or 1) * d) * (folds if folds else 2 if validation else 1) + (folds if folds and yy else 0)


def host_alloc(nbytes):
    """page-locked host buffer as a numpy uint8 array (lgc_host_alloc); free with host_free(arr)"""
    L = lib()
    L.lgc_host_alloc.restype = C.c_void_p; L.lgc_host_alloc.argtypes = [C.c_size_t]
    p = L.lgc_host_alloc(nbytes)
    if not p:
        raise LgcError(-4, L.lgc_last_error().decode())
    arr = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), (nbytes,))
    return arr


def host_free(arr):
    L = lib()
    L.lgc_host_free.restype = None; L.lgc_host_free.argtypes = [C.c_void_p]
    L.lgc_host_free(C.c_void_p(arr.ctypes.data))


def device_count():
    return lib().lgc_device_count()


def make_system(d, width=64, precision=56, algorithm="cgd", num_iterations=0, lam=0.0, nshares=2,
                normalize=0, reveal_inputs=0, trace=0):
    alg = ALG[algorithm] if isinstance(algorithm, str) else int(algorithm)
    return System(d, width, precision, alg, num_iterations, lam, nshares, normalize, reveal_inputs, trace)


class _Request:
    """What Program, Solver and Party are asked to lower, resolved once: the Python-side checks in their one order, the kind
    (the suffix of the C call, a key of _KINDS), the arguments of that call behind the front's lead, and the layout of what
    the program reads and reveals.  The keywords, the same on all three fronts:

    lambdas: a per-lambda sweep -- len(lambdas) circuits on the same shares in one program (_sweep_at); first: the index of
    lambdas[0] in a sweep sharded over several GPUs (all ranks share the seed).  With folds=K: the ridge sweep cross-validated
    in the circuit (_ridge_cv), K (T + d) words per share, beta the refit at the best lambda.
    targets: k right-hand sides for the one A (_targets): T + k d words per share, beta is (k, d).
    l1: lambda1 of the lasso solver (algorithm "lasso", _lasso), or a sequence of L of them, an absolute lasso path;
    l1_ratios: L ratios of lambda_max, a ratio path (_lasso_path).  beta of a path is (L, d).
    positive, lower, upper, penalty_factors: per-coefficient bounds and penalty factors of the lasso (_lasso_opts).
    validation: every share is [A, b, A_v, b_v], 2 (T + d) words, and the path's model is selected on (A_v, b_v) in the
    circuit (_lasso_select): beta is beta* (d); reveal_index, reveal_scores: reveal l* and the L scores beside it.
    folds: K-fold cross-validation instead (_lasso_cv): every share is [A_0, b_0, ..., A_{K-1}, b_{K-1}], K (T + d) words;
    beta is the refit on all folds at the value with the least summed score, the scores are the L sums.
    rule ("min" / "1se"), reveal_curve: the calls of linreg_gc_lasso_cv_se.h (_lasso_cv_se) -- every share ends with K words
    yy_k; with "1se" beta is the refit at l+, the selected index is l+, the min index l*, the curve the revealed (mean, se).
    inference=("se", "fit") (any non-empty subset) with resid_scale=: the Cholesky solve with standard errors, residual
    variance and R^2 (_inference) -- every share is [A, b, yy], T + d + 1 words; beta is the plain solve's.
    scan=M (scan_se, resid_scale): an association scan of M candidate columns against the system's c = d - 1 shared
    covariates (_scan): T_c + c + 1 + M (c + 2) words per share; beta is the M coefficient words, w the M words w_m.

    no_sweep: the refusal of a front that has no plain sweep (a party), raised where that front has always raised it.
    Attributes: kind, tail, and what the fronts show -- path, folds, select, rule, infer, scan, targets, count."""

    def __init__(self, system, lambdas=None, first=0, targets=None, l1=None, l1_ratios=None, positive=False, lower=None,
                 upper=None, penalty_factors=None, validation=False, reveal_index=False, reveal_scores=False, folds=None, rule=None,
                 reveal_curve=False, inference=None, resid_scale=None, scan=None, scan_se=False, no_sweep=None):
        self.system = system
        self.targets = None if targets is None else int(targets)
        self.path = self.program_path = self.folds = self.select = self.rule = self.infer = self.scan = self.count = None
        self.kind, *args = self._resolve(system, lambdas, first, targets, l1, l1_ratios, positive, lower, upper, penalty_factors,
                                         validation, reveal_index, reveal_scores, folds, rule, reveal_curve, inference, resid_scale,
                                         scan, scan_se, no_sweep)
        self._keep = args                         # (the arrays and the options the pointers of the tail point into)
        self.tail = [a.ctypes.data_as(C.c_void_p) if isinstance(a, np.ndarray) else C.byref(a) if isinstance(a, LassoOpts) else a
                     for a in args]

    def _resolve(self, system, lambdas, first, targets, l1, l1_ratios, positive, lower, upper, penalty_factors, validation,
                 reveal_index, reveal_scores, folds, rule, reveal_curve, inference, resid_scale, scan, scan_se, no_sweep):
        """(kind, arguments ...): arrays and the options struct as they are, the rest as the C call takes it"""
        others = dict(lambdas=lambdas, first=first, targets=targets, l1=l1, l1_ratios=l1_ratios, positive=positive, lower=lower,
                      upper=upper, penalty_factors=penalty_factors, validation=validation, reveal_index=reveal_index,
                      reveal_scores=reveal_scores, folds=folds, rule=rule, reveal_curve=reveal_curve)
        self.scan = _scan(scan, scan_se, resid_scale, inference=inference, **others)
        if self.scan is not None:
            return "_scan", self.scan[0], self.scan[2], self.scan[1]
        self.infer = _inference(inference, resid_scale, **others)
        if self.infer is not None:
            return "_inference", self.infer[1], self.infer[0]
        _no_sweep_targets(lambdas, targets)
        path = _l1_path(l1, l1_ratios)
        _no_lasso_mix(lambdas, targets, l1 if l1_ratios is None else l1_ratios)
        self.path = self.program_path = None if path is None else int(path[0].size)
        ridge = _ridge_cv(system, lambdas, first, folds, validation, reveal_index, reveal_scores, rule, reveal_curve)
        if no_sweep and lambdas is not None and ridge is None:
            raise LgcError(-1, no_sweep)
        if ridge is not None:                     # lambdas with folds: the ridge sweep cross-validated
            lam, self.folds, self.select = ridge
            self.path = self.program_path = int(lam.size)
            return "_ridge_cv", lam.size, lam, self.folds, self.select
        self.select = _select_flags(validation, reveal_index, reveal_scores, l1, l1_ratios, folds)
        self.folds = None if folds is None else int(folds)
        opts = _lasso_opts(system, l1, l1_ratios, positive, lower, upper, penalty_factors, always=self.select is not None)
        self.rule = _cv_rule(rule, reveal_curve, folds)
        if self.select is not None:               # a selection over a single l1 is a path of one model for Solver and Party;
            self.path = self.path or 1            # Program.path stays None there (program_path)
        if self.rule is not None:
            self.select |= SELECT_REVEAL_CURVE if reveal_curve else 0
            return "_lasso_cv_se", opts, self.folds, self.select, self.rule
        if self.folds is not None:
            return "_lasso_cv", opts, self.folds, self.select
        if self.select is not None:
            return "_lasso_select", opts, self.select
        if opts is not None:
            return "_lasso_opts", opts
        if path is not None:
            return "_lasso_path", path[0].size, path[0], path[1]
        if l1 is not None:
            return "_lasso", float(l1)
        if targets is not None:
            return "_targets", self.targets
        if lambdas is None:
            return ("",)
        lam = np.ascontiguousarray(lambdas, dtype=np.float64)   # per-lambda sweep: len(lambdas) circuits in one program
        self.count = int(lam.size)                # (circuits first .. of a larger sweep)
        return "_sweep_at", lam.size, lam, first

    def in_words(self):
        """input words per share"""
        if self.scan is not None:
            return _scan_in_words(self.system, self.scan[0])
        return _in_words(self.system, self.targets, self.select is not None, self.folds, self.rule is not None, self.infer is not None)

    def revealed_shape(self):
        """shape of the int64 buffer lgc_solver_get_beta and lgc_party_finish fill: beta of a single solve (d), a sweep
        (count, d), k targets (k, d) or a lasso path (L, d); of the other kinds every word the program may reveal"""
        d = int(self.system.d)
        if self.scan is not None:
            return self.scan[0] * (2 if self.scan[1] & SCAN_SE else 1)
        if self.infer is not None:
            return 2 * d + 2
        if self.select is not None:
            return d + 2 + 3 * self.path          # (room for the indices, the scores and the curve)
        rows = [n for n in (self.path, self.targets, self.count) if n is not None]
        return (rows[0], d) if rows else d

    def split(self, words):
        """everything the program reveals, out of that buffer; None where the kind or its flags reveal nothing:
        beta (in its shape); index, min_index, scores (L), curve (mean, se) of a selection; u (d), s2, r2 of an inference
        program; w (M) of a scan"""
        words = np.asarray(words)
        r = types.SimpleNamespace(beta=words, index=None, min_index=None, scores=None, curve=None, u=None, s2=None, r2=None, w=None)
        d = int(self.system.d)
        if self.scan is not None:                 # the M coefficients, then the M words w_m
            M = self.scan[0]
            r.beta = words[:M].copy()
            if self.scan[1] & SCAN_SE:
                r.w = words[M:2 * M].copy()
        elif self.infer is not None:              # beta, then u and (s2, r2)
            r.beta, r.u, r.s2, r.r2 = _infer_split(words, d, self.infer[0])
        elif self.select is not None:             # beta*, [l*], [scores]; under "1se" beta+, [l+, l*], [scores]; [mean, se]
            L, k = self.path, d
            r.beta = words[:d].copy()
            if self.select & SELECT_REVEAL_INDEX:
                r.index = r.min_index = int(words[k]); k += 1
                if self.rule == CV_RULE["1se"]:
                    r.min_index = int(words[k]); k += 1
            if self.select & SELECT_REVEAL_SCORES:
                r.scores = words[k:k + L].copy(); k += L
            if self.select & SELECT_REVEAL_CURVE:
                r.curve = (words[k:k + L].copy(), words[k + L:k + 2 * L].copy())
        return r


class _Results:
    """What Solver and Party show of a request and of the words its program reveals.  A front supplies _C (the prefix of its
    C calls), _need(what, name) -- its own refusal when the program reveals no such thing, or not yet -- and _revealed(), the
    split words"""

    def _adopt(self, request):
        r = self._req = request
        self.path, self.folds, self.select, self.rule, self.infer, self.scan, self.targets = \
            r.path, r.folds, r.select, r.rule, r.infer, r.scan, r.targets

    def _of(self, what, name):
        self._need(what, name)
        return self._revealed()

    def selected_index(self):
        """the index of the revealed model of a selection that has run / finished (l*; l+ under "1se"); -1 when reveal_index
        was not set (lgc_solver_selected_index, lgc_party_selected_index)"""
        self._need("select", "selected_index")
        return int(getattr(lib(), self._C + "selected_index")(self._h))

    def min_index(self):
        """l*, the arg-min, of a cross-validation that has run / finished; -1 when reveal_index was not set"""
        self._need("select", "min_index")
        return int(getattr(lib(), self._C + "min_index")(self._h))

    def scores(self):
        """the L scores of a model selection, or None when reveal_scores was not set"""
        return self._of("select", "scores").scores

    def cv_curve(self):
        """(mean, se): the L words each that reveal_curve=True revealed (cv.glmnet's cvm, cvsd), or None"""
        return self._of("curve", "cv_curve").curve

    def std_err_words(self):
        """the d words u_j = sqrt(mul(s2, v_j)) (the standard error of beta_j is u_j / sqrt(n)), or None without "se\""""
        return self._of("infer", "std_err_words").u

    def sigma2_word(self):
        """the word s2 = mulc(e, q(resid_scale)), or None without "fit\""""
        return self._of("infer", "sigma2_word").s2

    def r2_word(self):
        """the word r2 = 2^p - div(e, Y), or None without "fit\""""
        return self._of("infer", "r2_word").r2

    def summary(self, n):
        """floats: std_err = u / sqrt(n) for the public row count n, sigma2, r2 (None where not revealed); in the units of the
        data the shares were formed from (studentised data: studentised units)"""
        r = self._of("infer", "summary")
        return _infer_summary((r.beta, r.u, r.s2, r.r2), n, self.system)

    def scan_std_err_words(self):
        """the M words w_m = sqrt(mul(s2_m, v_m)) (the standard error of beta_m is w_m / sqrt(n)), or None without scan_se"""
        return self._of("scan", "scan_std_err_words").w

    def scan_summary(self, n):
        """floats: beta (M), std_err = w / sqrt(n) for the public row count n (None without scan_se)"""
        r = self._of("scan", "scan_summary")
        return _scan_summary(r.beta, r.w, n, self.system)


class Program:
    """The lowered circuit program (host only; needs no GPU)."""

    def __init__(self, system, lambdas=None, first=0, targets=None, l1=None, l1_ratios=None, positive=False, lower=None,
                 upper=None, penalty_factors=None, validation=False, reveal_index=False, reveal_scores=False, folds=None, rule=None,
                 reveal_curve=False, inference=None, resid_scale=None, scan=None, scan_se=False):
        """lgc_program_build<kind> of the request these keywords make: see _Request.  path is None for a single l1, also
        where validation= or folds= select over it (Solver and Party count one model there)"""
        self._h = C.c_void_p()
        r = _Request(system, lambdas=lambdas, first=first, targets=targets, l1=l1, l1_ratios=l1_ratios, positive=positive,
                     lower=lower, upper=upper, penalty_factors=penalty_factors, validation=validation, reveal_index=reveal_index, reveal_scores=reveal_scores,
                     folds=folds, rule=rule, reveal_curve=reveal_curve, inference=inference, resid_scale=resid_scale, scan=scan,
                     scan_se=scan_se)
        self.path, self.folds, self.select, self.rule, self.infer, self.scan = r.program_path, r.folds, r.select, r.rule, r.infer, r.scan
        _chk(getattr(lib(), "lgc_program_build" + r.kind)(C.byref(self._h), C.byref(system), *r.tail))
        self.info = ProgramInfo()
        _chk(lib().lgc_program_info_get(self._h, C.byref(self.info)))
        self.system = system

    def records(self):
        n = self.info.n_records
        ptr = lib().lgc_program_records(self._h)
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), (n * C.sizeof(Record),)).copy()

    def launches(self):
        ptr = lib().lgc_program_launches(self._h)
        return [dict(first_rec=ptr[i].first_rec, nrec=ptr[i].nrec, step0=ptr[i].step0, steps=ptr[i].steps,
                     gates=ptr[i].gates, mac_only=ptr[i].mac_only) for i in range(self.info.n_launches)]

    def ring_plan(self, ring_bytes=0):
        """(ring size, offsets, wait_for) of the co-located solver's garbled-table ring"""
        n = self.info.n_launches
        off = np.zeros(n, dtype=np.uint64); wait = np.zeros(n, dtype=np.int64); rb = C.c_size_t()
        _chk(lib().lgc_program_ring_plan(self._h, ring_bytes, C.byref(rb), off.ctypes.data_as(C.c_void_p),
                                         wait.ctypes.data_as(C.c_void_p)))
        return rb.value, off, wait

    def close(self):
        if self._h:
            lib().lgc_program_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()


class Solver(_Results):
    """Garble + evaluate one linear system on one MI355X (both roles co-located).

    Replaces `execYaoProtocol(pd, solver, &ls)` (reference src/cmd/linreg.c:177)."""
    _C = "lgc_solver_"
    _NEEDS = {"select": ("select", "not a model selection: the solver was not created with validation=True or folds=K"),
              "curve": ("rule", "no curve: the solver was not created with rule= or reveal_curve="),
              "infer": ("infer", "not an inference program: the solver was not created with inference="),
              "scan": ("scan", "not a scan: the solver was not created with scan=M")}

    def __init__(self, system, seed=b"\x01" * 16, device=0, lambdas=None, first=0, targets=None, l1=None, l1_ratios=None,
                 positive=False, lower=None, upper=None, penalty_factors=None, validation=False, reveal_index=False,
                 reveal_scores=False, folds=None, rule=None, reveal_curve=False, inference=None, resid_scale=None, scan=None,
                 scan_se=False):
        """lgc_solver_create<kind> of the request these keywords make: see _Request.  Shares are nshares x the words per share
        given there; beta() has the shape given there, a sweep's is (len(lambdas), d) and count is its length.
        selected_index(), min_index(), scores(), cv_curve() show the rest of a selection; std_err_words(), sigma2_word(),
        r2_word() the raw words of an inference program and summary(n) the floats; scan_std_err_words() the M words w_m of a
        scan and scan_summary(n) the floats"""
        assert len(seed) == 16
        self._h = C.c_void_p()
        self.system = system
        self._adopt(_Request(system, lambdas=lambdas, first=first, targets=targets, l1=l1, l1_ratios=l1_ratios, positive=positive,
                             lower=lower, upper=upper, penalty_factors=penalty_factors, validation=validation, reveal_index=reveal_index, reveal_scores=reveal_scores,
                             folds=folds, rule=rule, reveal_curve=reveal_curve, inference=inference, resid_scale=resid_scale, scan=scan,
                             scan_se=scan_se))
        self.count = self._req.count
        _chk(getattr(lib(), "lgc_solver_create" + self._req.kind)(C.byref(self._h), device, C.byref(system), seed, *self._req.tail))

    # ---- shared prefix of a sweep block (input labels + garbled share summation): garbled on one rank,
    # broadcast, imported by every rank.  dev_ptr: device memory of prefix_bytes() bytes (e.g. tensor.data_ptr())
    def prefix_bytes(self):
        return int(lib().lgc_solver_prefix_bytes(self._h))

    def prefix_garble(self):
        _chk(lib().lgc_solver_prefix_garble(self._h))

    def prefix_export(self, dev_ptr):
        _chk(lib().lgc_solver_prefix_export(self._h, C.c_void_p(dev_ptr)))

    def prefix_import(self, dev_ptr):
        _chk(lib().lgc_solver_prefix_import(self._h, C.c_void_p(dev_ptr)))

    def set_shares(self, shares):
        shares = np.ascontiguousarray(shares, dtype=np.uint64)
        assert shares.size == self.system.nshares * self._req.in_words(), shares.shape
        _chk(lib().lgc_solver_set_shares(self._h, shares.ctypes.data_as(C.c_void_p)))

    def run(self, profile=False):
        _chk(lib().lgc_solver_run(self._h, 1 if profile else 0))

    def _need(self, what, name):
        attr, refusal = self._NEEDS[what]
        if getattr(self, attr) is None:
            raise LgcError(-1, refusal)

    def _revealed(self):
        out = np.zeros(self._req.revealed_shape(), dtype=np.int64)
        _chk(lib().lgc_solver_get_beta(self._h, out.ctypes.data_as(C.c_void_p)))
        return self._req.split(out)

    def beta(self):
        return self._revealed().beta

    def trace(self):
        out = np.zeros((self.system.num_iterations, _trace_width(self.system)), dtype=np.int64)
        _chk(lib().lgc_solver_get_trace(self._h, out.ctypes.data_as(C.c_void_p)))
        return out

    def inputs(self):
        out = np.zeros(self._req.in_words(), dtype=np.int64)
        _chk(lib().lgc_solver_get_inputs(self._h, out.ctypes.data_as(C.c_void_p)))
        return out

    def stats(self):
        st = Stats()
        _chk(lib().lgc_solver_get_stats(self._h, C.byref(st)))
        return st.asdict()

    def profile(self, nlaunches):
        g = np.zeros(nlaunches); e = np.zeros(nlaunches)
        _chk(lib().lgc_solver_get_profile(self._h, g.ctypes.data_as(C.c_void_p), e.ctypes.data_as(C.c_void_p), nlaunches))
        return g, e

    def iterations(self):
        """cgd, lasso: (cumulative AND gates, device seconds since the start of run) per iteration -- the
        values src/cgd.oc:190-194 prints as 'Iteration t gate count' / 'Iteration t time'."""
        n = int(self.system.num_iterations) if _iterative(self.system) else 0
        g = np.zeros(n, dtype=np.uint64); t = np.zeros(n)
        _chk(lib().lgc_solver_get_iterations(self._h, g.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p), n))
        return g, t

    def close(self):
        if self._h:
            lib().lgc_solver_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def fold_rows(n, folds, k):
    """(r0, r1): fold k of `folds` over n rows is rows [r0, r1) (lgc_fold_rows, the one statement of the rule)"""
    r0, r1 = C.c_size_t(), C.c_size_t()
    _chk(lib().lgc_fold_rows(n, folds, k, C.byref(r0), C.byref(r1)))
    return r0.value, r1.value


class Phase1:
    """One data provider's quantised data on the device (phase-1 aggregation arithmetic,
    reference src/phase1.c)."""

    def __init__(self, Xq, yq=None, width=64, precision=56, device=0, targets=None):
        """targets: k target columns (lgc_p1_create_targets); yq is then n x k (or None), and column d + t of
        mask / dot / ti_a is target t"""
        Xq = np.ascontiguousarray(Xq, dtype=np.int64)
        self.n, self.d = Xq.shape
        self.n_all = self.n
        self.w, self.p = width, precision
        self.dev_io = False
        self.targets = None if targets is None else int(targets)
        self._h = C.c_void_p()
        if targets is None:
            _chk(lib().lgc_p1_create(C.byref(self._h), device, self.n, self.d, width, precision))
            yq = None if yq is None else np.ascontiguousarray(yq, dtype=np.int64)
            _chk(lib().lgc_p1_set_data(self._h, _vp(Xq), _vp(yq)))
        else:
            _chk(lib().lgc_p1_create_targets(C.byref(self._h), device, self.n, self.d, self.targets, width, precision))
            yq = None if yq is None else np.ascontiguousarray(yq, dtype=np.int64).reshape(self.n, self.targets)
            _chk(lib().lgc_p1_set_targets(self._h, _vp(Xq), _vp(yq)))

    def local(self, c0, c1, with_y=False):
        own = c1 - c0
        A = np.zeros(own * (own + 1) // 2, dtype=np.uint64)
        b = np.zeros(own, dtype=np.uint64)
        _chk(lib().lgc_p1_local(self._h, c0, c1, 1 if with_y else 0, _vp(A), _vp(b)))
        return (A, b) if with_y else A

    def local_yy(self, c0, c1):
        """local(c0, c1, with_y=True) and yy, the word sum y_q y_q, from the same launches (lgc_p1_local_yy)"""
        own = c1 - c0
        A = np.zeros(own * (own + 1) // 2, dtype=np.uint64)
        b = np.zeros(own, dtype=np.uint64)
        yy = np.zeros(1, dtype=np.uint64)
        _chk(lib().lgc_p1_local_yy(self._h, c0, c1, _vp(A), _vp(b), _vp(yy)))
        return A, b, yy[0]

    def set_divisor(self, divisor):
        """the divisor of the floating-point diagonal for every later call (lgc_p1_set_divisor); the default is d"""
        _chk(lib().lgc_p1_set_divisor(self._h, divisor))

    def local_scan(self, c0, c1, s0, s1, with_y=False):
        """the candidates' block of a scan (lgc_p1_local_scan): own covariates [c0, c1) (may be empty), own candidates [s0, s1).
        Returns (H (s1 - s0, c1 - c0), gg (s1 - s0)[, gy (s1 - s0)])"""
        ns, nc = max(0, s1 - s0), max(0, c1 - c0)
        H = np.zeros((ns, nc), dtype=np.uint64)
        gg = np.zeros(max(1, ns), dtype=np.uint64)
        gy = np.zeros(max(1, ns), dtype=np.uint64)
        _chk(lib().lgc_p1_local_scan(self._h, c0, c1, s0, s1, 1 if with_y else 0, _vp(H) if nc and ns else None, _vp(gg), _vp(gy) if with_y else None))
        return (H, gg[:ns], gy[:ns]) if with_y else (H, gg[:ns])

    def set_rows(self, r0, r1):
        """every later call acts on rows [r0, r1) only, as an object created from those rows would (lgc_p1_set_rows); self.n
        follows, self.n_all keeps the rows the object was created with"""
        _chk(lib().lgc_p1_set_rows(self._h, r0, r1))
        self.n = r1 - r0

    def local_folds(self, c0, c1, folds, with_y=False):
        """K windowed local() calls from one read of X (lgc_p1_local_folds): A as (K, own (own + 1) / 2), b as (K, own)"""
        own = c1 - c0
        A = np.zeros((folds, own * (own + 1) // 2), dtype=np.uint64)
        b = np.zeros((folds, own), dtype=np.uint64)
        _chk(lib().lgc_p1_local_folds(self._h, c0, c1, 1 if with_y else 0, folds, _vp(A), _vp(b)))
        return (A, b) if with_y else A

    def local_folds_yy(self, c0, c1, folds):
        """local_folds(c0, c1, folds, with_y=True) and yy, the K words sum y_q y_q of every fold, from the same launch
        (lgc_p1_local_folds_yy)"""
        own = c1 - c0
        A = np.zeros((folds, own * (own + 1) // 2), dtype=np.uint64)
        b = np.zeros((folds, own), dtype=np.uint64)
        yy = np.zeros(folds, dtype=np.uint64)
        _chk(lib().lgc_p1_local_folds_yy(self._h, c0, c1, folds, _vp(A), _vp(b), _vp(yy)))
        return A, b, yy

    def ti_a_batch(self, cols, y, inn, sub):
        """party a of a run of pairs in one device call (lgc_p1_ti_a_batch): (a - y as (npairs, n), the npairs shares)"""
        cols = np.ascontiguousarray(cols, dtype=np.uint32)
        y = np.ascontiguousarray(y, dtype=np.uint64).reshape(len(cols), self.n)
        inn = np.ascontiguousarray(inn, dtype=np.uint64).reshape(len(cols), self.n)
        sub = np.ascontiguousarray(sub, dtype=np.uint64).reshape(len(cols))
        out = np.empty_like(y); shares = np.zeros(len(cols), dtype=np.uint64)
        _chk(lib().lgc_p1_ti_a_batch(self._h, _vp(cols), len(cols), _vp(y), _vp(inn), _vp(sub), _vp(out), _vp(shares)))
        return out, shares

    def local_targets(self, c0, c1, with_b=True):
        """(A packed lower triangle of the own block, B = X[:, c0:c1]^T Y as (k, c1 - c0) or None)"""
        own = c1 - c0
        A = np.zeros(own * (own + 1) // 2, dtype=np.uint64)
        B = np.zeros(((self.targets or 1), own), dtype=np.uint64) if with_b else None
        _chk(lib().lgc_p1_local_targets(self._h, c0, c1, _vp(A), _vp(B)))
        return A, B

    def mask(self, cols, V, sign):
        cols = np.ascontiguousarray(cols, dtype=np.uint32)
        V = np.ascontiguousarray(V, dtype=np.uint64).reshape(len(cols), self.n)
        out = np.empty_like(V)
        _chk(lib().lgc_p1_mask(self._h, _vp(cols), len(cols), _vp(V), sign, _vp(out)))
        return out

    def ti_a(self, col, y, inn, sub):
        """party a of one inner_product_ti in a single pass: (a - y, <inn, y> - sub)"""
        y = np.ascontiguousarray(y, dtype=np.uint64).reshape(self.n)
        inn = np.ascontiguousarray(inn, dtype=np.uint64).reshape(self.n)
        out = np.empty(self.n, dtype=np.uint64); share = C.c_uint64()
        _chk(lib().lgc_p1_ti_a(self._h, int(col), _vp(y), _vp(inn), C.c_uint64(int(sub)), _vp(out), C.byref(share)))
        return out, np.uint64(share.value)

    def dot(self, A, B=None, cols=None, sub=None):
        A = np.ascontiguousarray(A, dtype=np.uint64).reshape(-1, self.n)
        npairs = A.shape[0]
        B = None if B is None else np.ascontiguousarray(B, dtype=np.uint64).reshape(npairs, self.n)
        cols = None if cols is None else np.ascontiguousarray(cols, dtype=np.uint32)
        sub = None if sub is None else np.ascontiguousarray(sub, dtype=np.uint64)
        out = np.zeros(npairs, dtype=np.uint64)
        _chk(lib().lgc_p1_dot(self._h, _vp(A), _vp(B), _vp(cols), npairs, _vp(sub), _vp(out)))
        return out

    # ---- one matrix triple per provider pair (include/linreg_gc_p1_matrix.h).  Blocks in wire form are arrays of uint32
    # (width 32) or uint64 words; with set_device_io(True) a block argument is a device address (an int) instead
    def set_device_io(self, on):
        """the block arguments of the calls below (and the vector arguments of mask / dot / ti_a_batch) are device memory"""
        _chk(lib().lgc_p1_set_device_io(self._h, 1 if on else 0))
        self.dev_io = bool(on)

    def _wire(self):
        return np.uint32 if self.w == 32 else np.uint64

    def _block(self, blk, ncols):
        """(the argument of the C call, what keeps it alive)"""
        if self.dev_io:
            return C.c_void_p(int(blk)), None
        blk = np.ascontiguousarray(blk, dtype=self._wire()).reshape(self.n, ncols)
        return _vp(blk), blk

    def matrix_mask(self, cols, seed, out_ptr=None):
        """E = (X[:, cols] - R) & m as (n, len(cols)) wire words, R the keystream of `seed` (lgc_p1_matrix_mask); with device
        I/O the block is written to the device address out_ptr and None is returned"""
        cols = np.ascontiguousarray(cols, dtype=np.uint32)
        if self.dev_io:
            _chk(lib().lgc_p1_matrix_mask(self._h, _vp(cols), len(cols), seed, C.c_void_p(int(out_ptr))))
            return None
        E = np.zeros((self.n, len(cols)), dtype=self._wire())
        _chk(lib().lgc_p1_matrix_mask(self._h, _vp(cols), len(cols), seed, _vp(E)))
        return E

    def matrix_share_a(self, ncols_a, seed_a, seed_s, F, ncols_b):
        """A's share (R_a^T F + S) & m as (ncols_a, ncols_b) uint64 (lgc_p1_matrix_share_a)"""
        arg, _keep = self._block(F, ncols_b)
        out = np.zeros((ncols_a, ncols_b), dtype=np.uint64)
        _chk(lib().lgc_p1_matrix_share_a(self._h, ncols_a, seed_a, seed_s, arg, ncols_b, _vp(out)))
        return out

    def matrix_share_b(self, cols_b, E, ncols_a, T):
        """B's share (E^T X[:, cols_b] + T) & m as (ncols_a, len(cols_b)) uint64 (lgc_p1_matrix_share_b)"""
        cols_b = np.ascontiguousarray(cols_b, dtype=np.uint32)
        arg, _keep = self._block(E, ncols_a)
        T = np.ascontiguousarray(T, dtype=self._wire()).reshape(ncols_a, len(cols_b))
        out = np.zeros((ncols_a, len(cols_b)), dtype=np.uint64)
        _chk(lib().lgc_p1_matrix_share_b(self._h, _vp(cols_b), len(cols_b), arg, ncols_a, _vp(T), _vp(out)))
        return out

    def close(self):
        if self._h:
            lib().lgc_p1_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def ti_generate(seed, first_pair, npairs, n, width=64, device=0):
    """(x, y, r, xy_minus_r) of the trusted initializer for `npairs` cross-party pairs"""
    x = np.zeros((npairs, n), dtype=np.uint64); y = np.zeros((npairs, n), dtype=np.uint64)
    r = np.zeros(npairs, dtype=np.uint64); xyr = np.zeros(npairs, dtype=np.uint64)
    _chk(lib().lgc_ti_generate(device, seed, first_pair, npairs, n, width, _vp(x), _vp(y), _vp(r), _vp(xyr)))
    return x, y, r, xyr


def ti_matrix_generate(seed_a, seed_b, seed_s, n, a, b, width=64, device=0):
    """the initializer's T = (R_a^T R_b - S) & m as (a, b) wire words (lgc_ti_matrix_generate)"""
    T = np.zeros((a, b), dtype=np.uint32 if width == 32 else np.uint64)
    _chk(lib().lgc_ti_matrix_generate(device, seed_a, seed_b, seed_s, n, a, b, width, _vp(T)))
    return T


def ti_matrix_seeds(master, u):
    """(seed_a, seed_b, seed_s) of instance u: blocks 3u, 3u + 1, 3u + 2 of the master seed's keystream (lgc_ti_matrix_seeds)"""
    out = [C.create_string_buffer(16) for _ in range(3)]
    _chk(lib().lgc_ti_matrix_seeds(master, u, *out))
    return tuple(o.raw for o in out)


GARBLER, EVALUATOR = 1, 2


class Party(_Results):
    """CSP (garbler, role 1) or Evaluator (role 2) on its own: the host carries tables, labels
    and decode bits between the two (reference src/cmd/linreg.c:145-199, src/input.c)."""
    _C = "lgc_party_"
    _FOLLOWS = {"scan": "the scan words follow finish() of a party created with scan=M",
                "infer": "the inference words follow finish() of a party created with inference="}

    def __init__(self, system, role, seed=None, device=0, max_launch_table_bytes=0, targets=None, l1=None, l1_ratios=None,
                 positive=False, lower=None, upper=None, penalty_factors=None, validation=False, reveal_index=False,
                 reveal_scores=False, folds=None, rule=None, reveal_curve=False, lambdas=None, inference=None, resid_scale=None,
                 scan=None, scan_se=False):
        """lgc_party_create<kind> of the request these keywords make: see _Request.  A party has no `first` and takes
        lambdas only with folds.  finish() returns (beta, trace, inputs), beta in the shape given there; the accessors of the
        rest (as Solver's) follow finish()"""
        self._h = C.c_void_p()
        self.system, self.role = system, role
        self._result = None
        first = 0                                 # (no sharded sweep between two parties)
        self._adopt(_Request(system, lambdas=lambdas, first=first, targets=targets, l1=l1, l1_ratios=l1_ratios, positive=positive,
                             lower=lower, upper=upper, penalty_factors=penalty_factors, validation=validation, reveal_index=reveal_index, reveal_scores=reveal_scores,
                             folds=folds, rule=rule, reveal_curve=reveal_curve, inference=inference, resid_scale=resid_scale, scan=scan,
                             scan_se=scan_se,
                             no_sweep="a party takes lambdas only with folds=K (a cross-validated ridge sweep)"))
        _chk(getattr(lib(), "lgc_party_create" + self._req.kind)(C.byref(self._h), device, C.byref(system), role, seed,
                                                                 max_launch_table_bytes, *self._req.tail))
        self._sizes()

    def _sizes(self):
        self.num_launches = lib().lgc_party_num_launches(self._h)
        self.input_bits = lib().lgc_party_input_bits(self._h)
        self.num_reveal = lib().lgc_party_num_reveal(self._h)
        self.and_gates = lib().lgc_party_and_gates(self._h)

    def table_bytes(self, k):
        return lib().lgc_party_table_bytes(self._h, k)

    def program_fingerprint(self):
        """32 bytes over everything the two roles must agree on (lgc_party_program_fingerprint)"""
        out = np.zeros(32, dtype=np.uint8)
        _chk(lib().lgc_party_program_fingerprint(self._h, _vp(out)))
        return out.tobytes()

    def input_pairs(self, share):
        m0 = np.zeros((self.input_bits, 16), dtype=np.uint8); m1 = np.zeros((self.input_bits, 16), dtype=np.uint8)
        _chk(lib().lgc_party_input_pairs(self._h, share, _vp(m0), _vp(m1)))
        return m0, m1

    def encode_inputs(self, share, values):
        values = np.ascontiguousarray(values, dtype=np.uint64)
        out = np.zeros((self.input_bits, 16), dtype=np.uint8)
        _chk(lib().lgc_party_encode_inputs(self._h, share, _vp(values), _vp(out)))
        return out

    def set_input_labels(self, share, labels):
        labels = np.ascontiguousarray(labels, dtype=np.uint8)
        assert labels.size == self.input_bits * 16
        _chk(lib().lgc_party_set_input_labels(self._h, share, _vp(labels)))

    def garble(self, k):
        buf = np.zeros(max(1, self.table_bytes(k)), dtype=np.uint8)
        _chk(lib().lgc_party_garble(self._h, k, _vp(buf)))
        return buf[:self.table_bytes(k)]

    def evaluate(self, k, tables):
        tables = np.ascontiguousarray(tables, dtype=np.uint8)
        _chk(lib().lgc_party_evaluate(self._h, k, _vp(tables) if tables.size else None))

    # ---- device-resident table ring (garbler and evaluator processes on one node)
    def ring_create(self, nslots):
        """garbler: allocate the ring; returns (64-byte hipIpc handle, slot bytes) for the evaluator process"""
        h = np.zeros(64, dtype=np.uint8); sb = C.c_size_t()
        _chk(lib().lgc_party_ring_create(self._h, nslots, _vp(h), C.byref(sb)))
        return h.tobytes(), sb.value

    def ring_open(self, handle, nslots, slot_bytes):
        _chk(lib().lgc_party_ring_open(self._h, _vp(np.frombuffer(handle, dtype=np.uint8).copy()), nslots, slot_bytes))

    def garble_ring(self, k):
        _chk(lib().lgc_party_garble_ring(self._h, k))

    def evaluate_ring(self, k):
        _chk(lib().lgc_party_evaluate_ring(self._h, k))

    def garble_ring_begin(self, k):
        """garbler: enqueue launch k into the ring and return at once (lgc_party_garble_ring_begin)"""
        _chk(lib().lgc_party_garble_ring_begin(self._h, k))

    def garble_ring_streams(self, n):
        """1: table passes on the record kernels' stream (before the first garble_ring_begin); 2: a stream of their own"""
        _chk(lib().lgc_party_garble_ring_streams(self._h, n))

    def garble_ring_wait(self, k):
        """garbler: return once the tables of launch k are complete in the ring"""
        _chk(lib().lgc_party_garble_ring_wait(self._h, k))

    def test_garble_ring_stage(self, k, stage):
        """test hook: stage 1 = record kernel of launch k into the ring path, 2 = its table pass; returns True when the
        launch is garbled on the critical path (has a table pass)"""
        crit = C.c_int()
        _chk(lib().lgc_test_party_garble_ring_stage(self._h, k, stage, C.byref(crit)))
        return bool(crit.value)

    def test_ring_read(self, k, nbytes):
        out = np.zeros(max(1, nbytes), dtype=np.uint8)
        _chk(lib().lgc_test_party_ring_read(self._h, k, _vp(out), nbytes))
        return out[:nbytes]

    def decode_bits(self):
        out = np.zeros(max(1, self.num_reveal), dtype=np.uint64)
        _chk(lib().lgc_party_decode_bits(self._h, _vp(out)))
        return out

    def finish(self, garbler_dec):
        """(beta, trace, inputs); what else the program reveals is kept for the accessors"""
        out = np.zeros(self._req.revealed_shape(), dtype=np.int64)
        trace = np.zeros((1 if self.scan is not None else max(1, self.system.num_iterations), _trace_width(self.system)), dtype=np.int64)
        inputs = np.zeros(self._req.in_words(), dtype=np.int64)
        garbler_dec = np.ascontiguousarray(garbler_dec, dtype=np.uint64)
        _chk(lib().lgc_party_finish(self._h, _vp(garbler_dec), _vp(out), _vp(trace), _vp(inputs)))
        self._result = self._req.split(out)
        return self._result.beta, trace, inputs

    def _need(self, what, name):
        what = "select" if what == "curve" else what      # (cv_curve() of a selection without rule= is None, not a refusal)
        if self._result is None or getattr(self, what) is None:
            raise LgcError(-1, self._FOLLOWS.get(what) or "%s follows finish() of a model selection" % name)

    def _revealed(self):
        return self._result

    def close(self):
        if self._h:
            lib().lgc_party_destroy(self._h); self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def share_choice_bits(values, width):
    """sel[i*intsize+j] = (input[i] >> j) & 1  (reference src/input.c:41)"""
    values = np.ascontiguousarray(values, dtype=np.uint64)
    return ((values[:, None] >> np.arange(width, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.uint8).ravel()


# The two payload forms of Gilboa on a whole block, lgc_ot_gilboa_<form>_{recv_start,send,recv_finish} with one signature per
# operation: form -> (words of y per (row, receiver column, sender column) at width w, its noun in a refusal)
_OT_BLOCK_FORMS = {"matrix": (lambda w: w, "matrix"), "half": (lambda w: w // 2 + 1, "half-payload")}


def _ot_block(form, op):
    return getattr(lib(), "lgc_ot_gilboa_%s_%s" % (form, op))


class OtSender:
    """IKNP extension sender (holds delta and the 128 seeds k_j^{delta_j} from the base OTs)"""

    def __init__(self, delta, seeds, device=0):
        seeds = np.ascontiguousarray(seeds, dtype=np.uint8).reshape(128, 16)
        self._h = C.c_void_p()
        _chk(lib().lgc_ot_sender_create(C.byref(self._h), device, bytes(delta), _vp(seeds)))

    def gilboa(self, b, width, u):
        b = np.ascontiguousarray(b, dtype=np.uint64); npairs, n = b.shape
        y = np.zeros(npairs * n * width, dtype=np.uint64); sh = np.zeros(npairs, dtype=np.uint64)
        _chk(lib().lgc_ot_gilboa_send(self._h, _vp(b), npairs, n, width, _vp(u), _vp(y), _vp(sh)))
        return y, sh

    # raw-pointer forms (integer addresses): page-locked host buffers (host_alloc) or, after
    # set_device_io(True), device memory used in place
    def set_device_io(self, on):
        _chk(lib().lgc_ot_sender_set_device_io(self._h, 1 if on else 0))

    def gilboa_ptr(self, b_ptr, npairs, n, width, u_ptr, y_ptr, shares_ptr):
        _chk(lib().lgc_ot_gilboa_send(self._h, C.c_void_p(b_ptr), npairs, n, width, C.c_void_p(u_ptr), C.c_void_p(y_ptr), C.c_void_p(shares_ptr)))

    # one vector OT per bit of the receiver's operand: xs is rows x s, the receiver holds rows x r.  `form` is "matrix"
    # (include/linreg_gc_ot_matrix.h) or "half" (include/linreg_gc_ot_half.h), see _ot_block
    def _block_send(self, form, xs, r, width, u):
        xs = np.ascontiguousarray(xs, dtype=np.uint64); rows, s = xs.shape
        y = np.zeros((rows * r * _OT_BLOCK_FORMS[form][0](width), s), dtype=np.uint32 if width == 32 else np.uint64)
        sh = np.zeros((r, s), dtype=np.uint64)
        _chk(_ot_block(form, "send")(self._h, _vp(xs), rows, r, s, width, _vp(u), _vp(y), _vp(sh)))
        return y, sh

    def _block_send_ptr(self, form, xs_ptr, rows, r, s, width, u_ptr, y_ptr, shares_ptr):
        _chk(_ot_block(form, "send")(self._h, C.c_void_p(xs_ptr), rows, r, s, width, C.c_void_p(u_ptr), C.c_void_p(y_ptr),
                                     C.c_void_p(shares_ptr)))

    # (xs, r, width, u) -> (y, shares): y is (rows * r * width, s), for the half form (rows * r * (width / 2 + 1), s), words of
    # `width` bits; shares r x s.  The _ptr forms: (xs_ptr, rows, r, s, width, u_ptr, y_ptr, shares_ptr)
    gilboa_matrix = functools.partialmethod(_block_send, "matrix")
    gilboa_matrix_ptr = functools.partialmethod(_block_send_ptr, "matrix")
    gilboa_half = functools.partialmethod(_block_send, "half")
    gilboa_half_ptr = functools.partialmethod(_block_send_ptr, "half")

    def labels(self, m0, m1, u):
        m0 = np.ascontiguousarray(m0, dtype=np.uint8).reshape(-1, 16); m1 = np.ascontiguousarray(m1, dtype=np.uint8).reshape(-1, 16)
        e = np.zeros((len(m0), 32), dtype=np.uint8)
        _chk(lib().lgc_ot_labels_send(self._h, _vp(m0), _vp(m1), len(m0), _vp(u), _vp(e)))
        return e

    def close(self):
        if self._h:
            lib().lgc_ot_sender_destroy(self._h); self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class OtReceiver:
    """IKNP extension receiver (holds the 128 seed pairs (k_j^0, k_j^1) from the base OTs)"""

    def __init__(self, seeds0, seeds1, device=0):
        seeds0 = np.ascontiguousarray(seeds0, dtype=np.uint8).reshape(128, 16)
        seeds1 = np.ascontiguousarray(seeds1, dtype=np.uint8).reshape(128, 16)
        self._h = C.c_void_p()
        _chk(lib().lgc_ot_receiver_create(C.byref(self._h), device, _vp(seeds0), _vp(seeds1)))

    def gilboa_start(self, a, width):
        a = np.ascontiguousarray(a, dtype=np.uint64); npairs, n = a.shape
        u = np.zeros(lib().lgc_ot_u_bytes(npairs * n * width), dtype=np.uint8)
        _chk(lib().lgc_ot_gilboa_recv_start(self._h, _vp(a), npairs, n, width, _vp(u)))
        if not hasattr(self, "_nps"):
            self._nps = []
        self._nps.append(npairs)               # several receives may be in flight; finishes complete the oldest
        return u

    def set_device_io(self, on):
        _chk(lib().lgc_ot_receiver_set_device_io(self._h, 1 if on else 0))

    def gilboa_start_ptr(self, a_ptr, npairs, n, width, u_ptr):
        _chk(lib().lgc_ot_gilboa_recv_start(self._h, C.c_void_p(a_ptr), npairs, n, width, C.c_void_p(u_ptr)))

    def gilboa_finish_ptr(self, y_ptr, shares_ptr):
        _chk(lib().lgc_ot_gilboa_recv_finish(self._h, C.c_void_p(y_ptr), C.c_void_p(shares_ptr)))

    def gilboa_finish(self, y):
        if not getattr(self, "_nps", None):
            sh = np.zeros(1, dtype=np.uint64)
            _chk(lib().lgc_ot_gilboa_recv_finish(self._h, _vp(np.ascontiguousarray(y, dtype=np.uint64)), _vp(sh)))
        sh = np.zeros(self._nps.pop(0), dtype=np.uint64)
        _chk(lib().lgc_ot_gilboa_recv_finish(self._h, _vp(np.ascontiguousarray(y, dtype=np.uint64)), _vp(sh)))
        return sh

    # one vector OT per bit of xr (rows x r) against a sender that holds s columns, in either form (_ot_block); each form is a kind
    # of its own in the library's queue of receives.  _blocks: (form, r, s, width) of the block receives in flight, oldest first
    def _block_start(self, form, xr, s, width):
        xr = np.ascontiguousarray(xr, dtype=np.uint64); rows, r = xr.shape
        u = np.zeros(lib().lgc_ot_u_bytes(rows * r * width), dtype=np.uint8)
        _chk(_ot_block(form, "recv_start")(self._h, _vp(xr), rows, r, s, width, _vp(u)))
        if not hasattr(self, "_blocks"):
            self._blocks = []
        self._blocks.append((form, r, s, width))
        return u

    def _block_finish(self, form, y):
        mine = [b for b in getattr(self, "_blocks", ()) if b[0] == form]
        if not mine:
            raise LgcError(-5, "no %s Gilboa receive was started on this receiver" % _OT_BLOCK_FORMS[form][1])    # LGC_ESTATE
        _, r, s, width = mine[0]               # the oldest of this form; the library refuses it unless it is the oldest of all
        sh = np.zeros((r, s), dtype=np.uint64)
        rc = _ot_block(form, "recv_finish")(self._h, _vp(np.ascontiguousarray(y, dtype=np.uint32 if width == 32 else np.uint64)), _vp(sh))
        if rc != -5:                           # the library consumed the receive, whether it succeeded or failed; LGC_ESTATE: it is not
            self._blocks.remove(mine[0])       # the oldest in flight and stays there
        _chk(rc)
        return sh

    def _block_start_ptr(self, form, xr_ptr, rows, r, s, width, u_ptr):
        _chk(_ot_block(form, "recv_start")(self._h, C.c_void_p(xr_ptr), rows, r, s, width, C.c_void_p(u_ptr)))

    def _block_finish_ptr(self, form, y_ptr, shares_ptr):
        _chk(_ot_block(form, "recv_finish")(self._h, C.c_void_p(y_ptr), C.c_void_p(shares_ptr)))

    # start: (xr, s, width) -> u; finish: (y) -> the r x s share block of the oldest receive of that form in flight;
    # start_ptr: (xr_ptr, rows, r, s, width, u_ptr); finish_ptr: (y_ptr, shares_ptr)
    gilboa_matrix_start = functools.partialmethod(_block_start, "matrix")
    gilboa_matrix_finish = functools.partialmethod(_block_finish, "matrix")
    gilboa_matrix_start_ptr = functools.partialmethod(_block_start_ptr, "matrix")
    gilboa_matrix_finish_ptr = functools.partialmethod(_block_finish_ptr, "matrix")
    gilboa_half_start = functools.partialmethod(_block_start, "half")
    gilboa_half_finish = functools.partialmethod(_block_finish, "half")
    gilboa_half_start_ptr = functools.partialmethod(_block_start_ptr, "half")
    gilboa_half_finish_ptr = functools.partialmethod(_block_finish_ptr, "half")

    def labels_start(self, choice):
        choice = np.ascontiguousarray(choice, dtype=np.uint8)
        self._m = len(choice)
        u = np.zeros(lib().lgc_ot_u_bytes(self._m), dtype=np.uint8)
        _chk(lib().lgc_ot_labels_recv_start(self._h, _vp(choice), self._m, _vp(u)))
        return u

    def labels_finish(self, e):
        out = np.zeros((self._m, 16), dtype=np.uint8)
        _chk(lib().lgc_ot_labels_recv_finish(self._h, _vp(np.ascontiguousarray(e, dtype=np.uint8)), _vp(out)))
        return out

    def close(self):
        if self._h:
            lib().lgc_ot_receiver_destroy(self._h); self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def release_cached_memory():
    """free the table ring a closed Solver left parked for the next one"""
    lib().lgc_release_cached_memory()


def set_split_kernels(garbler=True, evaluator=True):
    """which kernel runs the latency-bound launches of each role (16-wave column-split or 4-wave); interchangeable"""
    lib().lgc_set_split_kernels(int(bool(garbler)), int(bool(evaluator)))


def reference_gate_count(algorithm, width, d, iterations=0):
    """AND gates of the reference's circuit for the same solve, or None where it published none"""
    L = lib()
    L.lgc_reference_gate_count.argtypes = [C.c_int, C.c_int, C.c_size_t, C.c_int, C.POINTER(C.c_uint64)]
    L.lgc_reference_gate_count.restype = C.c_int
    g = C.c_uint64()
    alg = ALG[algorithm] if isinstance(algorithm, str) else int(algorithm)
    return int(g.value) if L.lgc_reference_gate_count(alg, width, d, iterations, C.byref(g)) == 0 else None


def set_karatsuba(on=True):
    """Karatsuba products in the CGD matrix-vector launches (width 64) for programs built from now on"""
    lib().lgc_set_karatsuba.argtypes = [C.c_int]; lib().lgc_set_karatsuba.restype = None
    lib().lgc_set_karatsuba(int(bool(on)))


def set_table_ring_slack(nbytes):
    """room in a co-located solver's table ring beyond its largest launch (0: the default, 8 GiB)"""
    lib().lgc_set_table_ring_slack.argtypes = [C.c_size_t]; lib().lgc_set_table_ring_slack.restype = None
    lib().lgc_set_table_ring_slack(int(nbytes))




def devices_preflight(devices):
    """lgc_devices_preflight (linreg_gc_sweep.h): every index exists and distinct devices can reach each other; raises LgcError
    with the index or the pair in the message otherwise"""
    arr = (C.c_int * len(devices))(*[int(v) for v in devices])
    L = lib()
    L.lgc_devices_preflight.argtypes = [C.c_void_p, C.c_size_t]; L.lgc_devices_preflight.restype = C.c_int
    _chk(L.lgc_devices_preflight(arr, len(devices)))


def gate_hash_eval(labels, tweaks, device=0):
    """the gate hash H(x, t) on the device: labels (n, 16) uint8, tweaks (n,) uint64 -> (n, 16) uint8"""
    x = np.ascontiguousarray(labels, dtype=np.uint8).reshape(-1, 16)
    t = np.ascontiguousarray(tweaks, dtype=np.uint64).reshape(-1)
    assert len(t) == len(x)
    out = np.zeros_like(x)
    L = lib()
    L.lgc_gate_hash_eval.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]; L.lgc_gate_hash_eval.restype = C.c_int
    _chk(L.lgc_gate_hash_eval(device, x.ctypes.data, t.ctypes.data, out.ctypes.data, len(x)))
    return out


class RowItem(C.Structure):
    _fields_ = [("label", C.c_uint8 * 16), ("tweak0", C.c_uint64), ("stride", C.c_uint64), ("rows", C.c_uint32),
                ("reserved", C.c_uint32)]


def row_hash_eval(items, device=0):
    """lgc_row_hash_eval (linreg_gc_debug.h): items = [(label: 16 bytes, tweak0, stride, rows)]; returns uint8
    (total rows, 2, 64, 16): per row the 64 lanes of row_hash, then the 64 lanes of the lane-uniform form"""
    arr = (RowItem * max(len(items), 1))()
    total = 0
    for it, (label, tweak0, stride, rows) in zip(arr, items):
        it.label[:] = bytes(label)
        it.tweak0, it.stride, it.rows = int(tweak0), int(stride), int(rows)
        total += int(rows)
    out = np.zeros((total, 2, 64, 16), dtype=np.uint8)
    L = lib()
    L.lgc_row_hash_eval.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]; L.lgc_row_hash_eval.restype = C.c_int
    _chk(L.lgc_row_hash_eval(device, C.cast(arr, C.c_void_p), len(items), out.ctypes.data))
    return out


def aes_bench(waves=8192, blocks_per_lane=256, device=0):
    rate, chk = C.c_double(), C.c_uint32()
    _chk(lib().lgc_aes_bench(device, waves, blocks_per_lane, C.byref(rate), C.byref(chk)))
    return rate.value, chk.value


def aes_encrypt(blocks, device=0):
    blocks = np.ascontiguousarray(blocks, dtype=np.uint8).reshape(-1, 16)
    out = np.empty_like(blocks)
    _chk(lib().lgc_aes_encrypt(device, blocks.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), len(blocks)))
    return out


# ---- test programs (linreg_gc_debug.h): raw records on a chosen record kernel
LM = {"auto": 0, "mac": 1, "mack": 2, "wide": 3, "split": 4, "quad2": 5, "split2": 20}   # LGC_LM_*


class LaunchConstants(C.Structure):
    _fields_ = [("wide_launch", C.c_uint32), ("narrow_mac", C.c_uint32), ("split_max_recs", C.c_uint32),
                ("mac_chunk", C.c_uint32), ("mac_adapt_lo", C.c_uint32), ("split2_min_steps", C.c_uint32)]


def _test_fn(name, restype, argtypes):
    fn = getattr(lib(), name)
    fn.restype, fn.argtypes = restype, argtypes
    return fn


def _modes(v, n):
    if v is None:
        return None
    v = [LM[m] if isinstance(m, str) else int(m) for m in v]
    assert len(v) == n, (len(v), n)
    return (C.c_int * n)(*v)


class RecordProgram(Program):
    """A program of raw records (lgc_test_program_create; host only).  records: (op, cnt, dst, a, b, c, sa, sb) tuples;
    launch_sizes: records per launch; modes_g / modes_e: per launch a key of LM (or an LGC_LM_* value), None = "auto".
    n_inputs input words start at word 1."""

    def __init__(self, width, precision, records, launch_sizes, modes_g=None, modes_e=None, n_inputs=0, n_words=None,
                 n_reveal=0):
        self._h = C.c_void_p()
        recs = (Record * len(records))(*[Record(*(tuple(r) + (0,))) for r in records])
        sizes = (C.c_uint32 * len(launch_sizes))(*[int(n) for n in launch_sizes])
        nl = len(launch_sizes)
        vp, sz, u32 = C.c_void_p, C.c_size_t, C.c_uint32
        fn = _test_fn("lgc_test_program_create", C.c_int,
                      [C.POINTER(vp), C.c_int, C.c_int, vp, sz, vp, sz, vp, vp, u32, u32, u32])
        _chk(fn(C.byref(self._h), width, precision, C.cast(recs, vp), len(records), C.cast(sizes, vp), nl,
                _modes(modes_g, nl), _modes(modes_e, nl), n_inputs, n_words, n_reveal))
        self.info = ProgramInfo()
        _chk(lib().lgc_program_info_get(self._h, C.byref(self.info)))
        self.system = make_system(0, width, precision, nshares=1)

    def modes(self):
        """(garbler, evaluator) kernel of every launch, LGC_LM_* values, as the solver picks them"""
        n = self.info.n_launches
        g = (C.c_int * n)(); e = (C.c_int * n)()
        _chk(_test_fn("lgc_test_launch_modes", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t])(self._h, g, e, n))
        return list(g), list(e)


class RecordSolver(Solver):
    """Both roles of a RecordProgram on one device (lgc_test_solver_create): inputs(values), run(), reveal()."""

    def __init__(self, program, seed=b"\x01" * 16, device=0):
        assert len(seed) == 16
        self._h = C.c_void_p()
        self.system = program.system
        self._adopt(_Request(program.system))     # (no request made this program: the plain one of its system stands in)
        self.count = None
        self._prog = program
        _chk(_test_fn("lgc_test_solver_create", C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_char_p])(
            C.byref(self._h), device, program._h, seed))

    def set_inputs(self, values):
        v = np.ascontiguousarray(values, dtype=np.uint64)
        _chk(lib().lgc_solver_set_shares(self._h, v.ctypes.data_as(C.c_void_p)))

    def reveal(self):
        n = self._prog.info.n_reveal
        out = np.zeros(n, dtype=np.uint64)
        _chk(_test_fn("lgc_test_solver_reveal", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t])(self._h, out.ctypes.data_as(C.c_void_p), n))
        return out


    def word_labels(self, garbler, first, n):
        """after run(): uint8 (n, 64, 16), the labels of words [first, first + n) in one role's word file"""
        out = np.zeros((n, 64, 16), dtype=np.uint8)
        fn = _test_fn("lgc_test_solver_read_words", C.c_int, [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p])
        _chk(fn(self._h, int(bool(garbler)), first, n, out.ctypes.data_as(C.c_void_p)))
        return out

    def tables(self, launch):
        """after run(): uint8 (steps, 2, 64, 16), the garbled table of a launch -- step, (TG | TE), lane, label"""
        steps = int(self._prog.launches()[launch]["steps"])
        out = np.zeros((steps, 2, 64, 16), dtype=np.uint8)
        fn = _test_fn("lgc_test_solver_read_tables", C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t])
        _chk(fn(self._h, launch, out.ctypes.data_as(C.c_void_p), out.nbytes))
        return out


def launch_shape(mode, garbler, nrec, cus):
    """(grid, threads, records per workgroup, __launch_bounds__) of a launch of nrec records in kernel `mode` on `cus` CUs"""
    u = C.c_uint32
    v = [u(), u(), u(), u()]
    fn = _test_fn("lgc_test_launch_shape", C.c_int, [C.c_int, C.c_int, u, u] + [C.POINTER(u)] * 4)
    _chk(fn(LM[mode] if isinstance(mode, str) else int(mode), int(bool(garbler)), nrec, cus, *[C.byref(x) for x in v]))
    return tuple(x.value for x in v)


def launch_constants():
    c = LaunchConstants()
    _test_fn("lgc_test_launch_constants", None, [C.POINTER(LaunchConstants)])(C.byref(c))
    return {k: getattr(c, k) for k, _ in LaunchConstants._fields_}
