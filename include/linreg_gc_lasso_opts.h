/*
 * linreg_gc_lasso_opts.h -- per-coefficient controls of the lasso solver: penalty factors and bounds (liblinreg_gc.so).
 *
 * A lasso solve (linreg_gc_lasso.h) or a lasso path (linreg_gc_lasso_path.h) with, per coordinate i:
 *   penalty_factors[i]  w_i >= 0: coordinate i is penalised by lambda1 w_i (glmnet's penalty.factor; 0 leaves it
 *                       unpenalised; per-coordinate weights give the adaptive lasso).  NULL: every w_i = 1
 *   lower[i], upper[i]  lo_i <= hi_i: beta_i is kept in [lo_i, hi_i] (glmnet's lower.limits / upper.limits; lower = 0 and
 *                       upper = +INFINITY everywhere is sklearn's positive=True).  -INFINITY / +INFINITY: no bound on that
 *                       side.  NULL: no bound on that side for any coordinate
 * Every iteration is the FISTA step of linreg_gc_lasso.h with the proximal step of lambda1 w_i |x| plus the indicator of
 * [lo_i, hi_i], which is separable per coordinate:
 *   x_i' = clamp(soft(z_i; theta_{l,i}), lo_i, hi_i)
 *   LGC_L1_ABSOLUTE  theta_{l,i} = step(q(lambda1_l w_i)), the product formed in IEEE double on the host
 *   LGC_L1_RATIO     theta_{l,i} = step(mul(lambda_max, q(r_l w_i))), lambda_max = max_i |b_i| as for a ratio path.  With
 *                    non-uniform factors ratio 1 no longer guarantees beta = 0 (glmnet divides lambda_max by w_i, which
 *                    here would need a secret divider)
 * q(v) = (int64)(v 2^p) wrapped to the width, as lambda1 is quantised.  The step, the Gershgorin bound and the FISTA
 * coefficients are those of the unconstrained solve.  Factors and bounds are public, like lambda1: they enter the program as
 * constant records only, and beta alone is revealed.  DESIGN.md 2.6 gives the definition and the range condition.
 *
 * With every factor 1 and every bound infinite the program is the one of lgc_program_build_lasso (one value, absolute
 * mode) or lgc_program_build_lasso_path, record for record, with the same fingerprint.  Every other linreg_gc.h call works
 * on the objects created here as on a lasso path's; lgc_party_program_fingerprint covers the factors and the bounds.
 * Rejected with LGC_EINVAL: a null opts; every rejection of a lasso path (count, values, mode, algorithm, trace); a factor
 * that is negative or not finite; a NaN bound, a lower bound of +INFINITY or an upper bound of -INFINITY; lo_i > hi_i; a
 * finite bound or a lambda1 w_i that width - 1 - precision integer bits cannot hold; a ratio r_l w_i whose quantised value
 * reaches the sign bit.
 */
#ifndef LINREG_GC_LASSO_OPTS_H
#define LINREG_GC_LASSO_OPTS_H
#include "linreg_gc_lasso_path.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lgc_lasso_opts {
    size_t l1_count;                /* values of lambda1 (1..LGC_MAX_L1_PATH); 1 with LGC_L1_ABSOLUTE: a single solve */
    const double *l1;               /* l1_count values: lambda1 itself, or ratios of lambda_max (l1_mode) */
    int l1_mode;                    /* LGC_L1_ABSOLUTE or LGC_L1_RATIO */
    const double *penalty_factors;  /* d factors, or NULL */
    const double *lower;            /* d lower bounds, or NULL */
    const double *upper;            /* d upper bounds, or NULL */
} lgc_lasso_opts;

int lgc_program_build_lasso_opts(struct lgc_program **out, const lgc_system *sys, const lgc_lasso_opts *opts);
int lgc_solver_create_lasso_opts(lgc_solver **out, int device, const lgc_system *sys, const uint8_t seed[16],
                                 const lgc_lasso_opts *opts);
int lgc_party_create_lasso_opts(lgc_party **out, int device, const lgc_system *sys, int role, const uint8_t seed[16],
                                size_t max_launch_table_bytes, const lgc_lasso_opts *opts);

#ifdef __cplusplus
}
#endif
#endif
