/*
 * gsdf_align_loss.h -- the weight a robust loss gives one point of the registration (gsdf_align_points_robust), host and device.
 *
 * The loss family is the reference's ps_optimizer/loss.h:41-48 (L2, CAUCHY, HUBER, TUKEY, TRUNC_L2), the integers those of
 * gsdf_ba_set_loss.  The weight is the factor the term phi^2 / phi J / J J^T of RigidPointOptimizer.cpp:76-80 is multiplied
 * with (iteratively reweighted least squares); phi is the signed distance gsdf_grad_sample returns, k the loss's scale in metres.
 *
 * All float, one rounding per operation (compile with -ffp-contract=off and correctly rounded fp32 divisions, as gsdf_math.h):
 * one definition for k_align_pass_robust and for gsdf_align_loss_weight, so that a caller can restate a pass bit for bit.
 */
#ifndef GSDF_ALIGN_LOSS_H_
#define GSDF_ALIGN_LOSS_H_

#include "gsdf_math.h"

#define GSDF_ALIGN_LOSS_L2       0
#define GSDF_ALIGN_LOSS_CAUCHY   1
#define GSDF_ALIGN_LOSS_HUBER    2
#define GSDF_ALIGN_LOSS_TUKEY    3
#define GSDF_ALIGN_LOSS_TRUNC_L2 4

/* loss in 0..4, k > 0 and finite unless loss == 0 (the callers check).  A NaN phi gives NaN (CAUCHY, HUBER) or 0 (TUKEY,
 * TRUNC_L2); +-inf gives 0 everywhere but L2. */
GSDF_HD float gsdf_align_weight(int loss, float k, float phi) {
    if (loss == GSDF_ALIGN_LOSS_L2) return 1.f;
    const float a = fabsf(phi);
    if (loss == GSDF_ALIGN_LOSS_HUBER) return a <= k ? 1.f : k / a;
    if (loss == GSDF_ALIGN_LOSS_TRUNC_L2) return a < k ? 1.f : 0.f;
    const float r = phi / k;
    const float rr = r * r;
    if (loss == GSDF_ALIGN_LOSS_CAUCHY) return 1.f / (1.f + rr);
    const float u = 1.f - rr;                                              /* TUKEY */
    return a < k ? u * u : 0.f;
}

/* what the entries refuse: a loss outside 0..4, and for a loss other than L2 a scale that is not finite or not > 0 */
inline bool gsdf_align_loss_valid(int loss, float scale) {
    if (loss < GSDF_ALIGN_LOSS_L2 || loss > GSDF_ALIGN_LOSS_TRUNC_L2) return false;
    return loss == GSDF_ALIGN_LOSS_L2 || (isfinite(scale) && scale > 0.f);
}

#endif /* GSDF_ALIGN_LOSS_H_ */
