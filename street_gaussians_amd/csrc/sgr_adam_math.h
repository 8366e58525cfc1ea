// sgr_adam_math.h -- the per-element Adam arithmetic of include/sgr_optim.h as one device function, shared by the
// per-segment step (sgr_optim.hip) and the sky cube map's gather-and-step (sgr_texture.hip, include/sgr_sky_step.h).
// The five operations are separate IEEE single operations: contraction is switched off inside the body, so a source
// compiled with the toolchain's default contraction (sgr_texture.hip) inlines the same roundings as one compiled with
// -ffp-contract=off (sgr_optim.hip).
#pragma once
#include <hip/hip_runtime.h>

struct AdamConsts {
    float c1, beta2, c2;  // (float)(1 - beta1), (float)beta2, (float)(1 - beta2)
};

// the host side of the contract: the constants from the optimiser's betas, formed in double and rounded once
static inline AdamConsts adam_consts(double beta1, double beta2) {
    return AdamConsts{(float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2)};
}

__device__ __forceinline__ void adam1(float& p, const float g, float& m, float& v, const AdamConsts k, const float ss,
                                      const float bc2s, const float eps) {
#pragma clang fp contract(off)
    m = m + k.c1 * (g - m);
    v = v * k.beta2;
    v = v + k.c2 * (g * g);
    const float d = sqrtf(v) / bc2s + eps;
    p = p + ss * (m / d);
}
