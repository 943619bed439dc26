/*
 * linreg_gc_lasso_path.h -- a lasso regularisation path: many values of lambda1 in one secure solve (liblinreg_gc.so).
 *
 * One program fits L values of lambda1 (1 <= L <= LGC_MAX_L1_PATH) against one M = X^T X / n + lambda2 I and one
 * b = X^T y / n, with lambda2 = lgc_system.lambda fixed.  Each value runs the FISTA recurrence of linreg_gc_lasso.h with
 * its own theta_l; the prefix, the copy of b, hdiff(M), the Gershgorin row sums and the step exponent are formed once, and
 * every iteration is one matrix-vector batch of L d dot products on the shared M and one launch of L d OP_PROX records.
 *   LGC_L1_ABSOLUTE  values are lambda1 itself, quantised as lgc_solver_create_lasso quantises it: beta_l is bit for bit
 *                    the beta of lgc_solver_create_lasso with lambda1 = values[l]
 *   LGC_L1_RATIO     values are ratios r_l in [0, 2] of lambda_max = max_i |b_i|, the smallest lambda1 whose lasso solution
 *                    is beta = 0 (the grid of glmnet and of sklearn's lasso_path): inside the circuit lambda1_l =
 *                    mul(lambda_max, r_l).  lambda_max is never revealed; neither are the step nor any theta_l.
 * DESIGN.md 2.6 gives the definition, the records and the range condition (in ratio mode 2 lambda_max must fit as well).
 *
 * Every other linreg_gc.h call works on the objects created here: shares, inputs and input bits have the sizes of a single
 * solve; lgc_solver_get_beta and lgc_party_finish give L x d words, lambda-major; iteration marks have one entry per
 * iteration; lgc_party_program_fingerprint covers the mode and every value.
 * Rejected with LGC_EINVAL: count 0 or above LGC_MAX_L1_PATH; values NULL; a value that is negative or not finite; a
 * ratio outside [0, 2] or one that the precision cannot hold; an unknown mode; a system that is not LGC_ALG_LASSO;
 * lgc_system.trace with count > 1.
 */
#ifndef LINREG_GC_LASSO_PATH_H
#define LINREG_GC_LASSO_PATH_H
#include "linreg_gc_lasso.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LGC_L1_ABSOLUTE 0
#define LGC_L1_RATIO 1
#define LGC_MAX_L1_PATH 256

struct lgc_program;
int lgc_program_build_lasso_path(struct lgc_program **out, const lgc_system *sys, size_t count, const double *values, int mode);
int lgc_solver_create_lasso_path(lgc_solver **out, int device, const lgc_system *sys, const uint8_t seed[16], size_t count,
                                 const double *values, int mode);
int lgc_party_create_lasso_path(lgc_party **out, int device, const lgc_system *sys, int role, const uint8_t seed[16],
                                size_t max_launch_table_bytes, size_t count, const double *values, int mode);
/* L: the number of lambda1 values (1 for every other object, 0 for NULL) */
size_t lgc_solver_path_length(const lgc_solver *s);
size_t lgc_party_path_length(const lgc_party *p);

#ifdef __cplusplus
}
#endif
#endif
