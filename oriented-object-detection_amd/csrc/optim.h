// The per-element arithmetic of the optimiser step, shared by the single-group kernels (optim.hip) and the multi-group ones (trainupd.hip): one
// definition, so the two forms are bit-identical by construction.  Each function follows torch.optim's single-tensor reference order operation by
// operation (the library is built with -ffp-contract=off: every operation below rounds once).
#pragma once
#include <cmath>

#include "ctx.h"

namespace obb {

// torch.optim.SGD (dampening 0, maximize False): d = g + wd p;  buf = first ? d : mu buf + d;  d = nesterov ? d + mu buf : buf;  p -= lr d
// (`b`: the momentum buffer's element; with `first` or mu == 0 its incoming value is not used, and with mu == 0 it is left as it came)
__device__ __forceinline__ void sgd_one(float &p, float g, float &b, float lr, float mu, float wd, int nesterov, int first) {
    float d = wd != 0.f ? g + wd * p : g;
    if (mu != 0.f) {
        b = first ? d : mu * b + d;
        d = nesterov ? d + mu * b : b;
    }
    p = p - lr * d;
}

// torch.optim.AdamW (amsgrad False): p *= 1 - lr wd;  m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g g;
//   p -= (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)            (bias corrections computed on the host in double, as torch does)
// 1 - b1 and 1 - b2 arrive rounded from double (omb1, omb2), as torch rounds its Python-float 1 - beta: 1.0f - 0.999f is 1.3e-5 off 0.001.
__device__ __forceinline__ void adamw_one(float &p, float g, float &m, float &v, float lr, float omb1, float b2, float omb2, float eps, float wd, float step_size,
                                          float sqrt_bc2) {
    p = p * (1.0f - lr * wd);
    m = m + (g - m) * omb1;                // torch: exp_avg.lerp_(grad, 1 - beta1)
    v = v * b2 + omb2 * g * g;             // torch: exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    const float denom = sqrtf(v) / sqrt_bc2 + eps;  // torch: (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
    p = p - step_size * (m / denom);
}

// the host half of AdamW: the constants a launch receives, from the double betas and the step counted from 1
struct AdamwConsts {
    float omb1, b2, omb2, sqrt_bc2;
    double bc1;
    float step_size(float lr) const { return (float)((double)lr / bc1); }
};
inline AdamwConsts adamw_consts(double beta1, double beta2, int64_t step) {
    const double bc2 = 1.0 - std::pow(beta2, (double)step);
    return {(float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)std::sqrt(bc2), 1.0 - std::pow(beta1, (double)step)};
}

}  // namespace obb
