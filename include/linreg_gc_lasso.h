/*
 * linreg_gc_lasso.h -- the lasso / elastic-net solver (liblinreg_gc.so).
 *
 * Not part of the drop-in surface of linreg_gc.h: the reference fits ridge regression only and has no counterpart for
 * these calls.  The solver minimises  1/2 beta^T M beta - b^T beta + lambda1 |beta|_1  with M = X^T X / n + lambda2 I and
 * b = X^T y / n as every other solver sees them (lgc_system.lambda is lambda2 and enters exactly as it does there), by
 * accelerated proximal gradient (FISTA) run for lgc_system.num_iterations iterations on the garbled word machine:
 *   step        2^(p - l), l = ceil(log2 d) + bitlen(max_i sum_j (|M_ij| >> ceil(log2 d))): a power of two at most
 *               1 / lambda_max(M), picked inside the circuit and never revealed
 *   iteration   g = M y - b, z = y - step(g), x' = z - clamp(z, -theta, theta) with theta = step(lambda1),
 *               y' = x' + c_k (x' - x), c_k the public FISTA coefficients
 * beta = x after N iterations.  Coordinates the soft-threshold sets to zero are the exact integer 0.  DESIGN.md 2.6 gives
 * the definition bit for bit, the lowering and the range condition (M, b and step(g) must fit in width - 1 - precision
 * integer bits, as for the other solvers).
 *
 * Every other linreg_gc.h call works on the objects created here unchanged: shares, beta (d words), inputs and input bits
 * have the sizes of a single-target solve, lgc_solver_get_iterations and lgc_party_iteration_marks have one entry per
 * iteration, and with lgc_system.trace the trace is num_iterations x d words (x after every iteration).
 * lgc_party_program_fingerprint covers lambda1 (the constant record that theta is formed from).
 * Rejected with LGC_EINVAL: lambda1 < 0 or not finite; LGC_ALG_LASSO through lgc_program_build, lgc_solver_create,
 * lgc_party_create (they carry no lambda1); lasso with several targets (linreg_gc_targets.h); lasso in a lambda sweep
 * (linreg_gc_sweep.h).
 */
#ifndef LINREG_GC_LASSO_H
#define LINREG_GC_LASSO_H
#include "linreg_gc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LGC_ALG_LASSO 4

/* the lowered program (host only, no GPU needed; the lgc_program calls of linreg_gc_debug.h introspect and destroy it) */
struct lgc_program;
int lgc_program_build_lasso(struct lgc_program **out, const lgc_system *sys, double l1);
int lgc_solver_create_lasso(lgc_solver **out, int device, const lgc_system *sys, const uint8_t seed[16], double l1);
int lgc_party_create_lasso(lgc_party **out, int device, const lgc_system *sys, int role, const uint8_t seed[16],
                           size_t max_launch_table_bytes, double l1);

#ifdef __cplusplus
}
#endif
#endif
