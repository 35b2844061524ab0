// Training-step slice: the optimiser update behind `model.train(...)` (Train_OBB.py:796-841).  Ultralytics'
// trainer builds torch.optim.SGD(momentum, nesterov=True) or torch.optim.AdamW(betas=(momentum, 0.999)) ("auto": by the iteration count,
// restated in train.py) over three parameter groups (weights with decay / norm weights / biases); here a group is ONE flat fp32 buffer
// (parameters, gradients and optimiser state side by side) and the update of the whole group is one streaming launch -- 16 (SGD) or 20
// (AdamW) bytes read and 8 / 12 written per parameter, float4 per lane, against the one launch per tensor and per elementary operation of
// the unfused form.  The arithmetic follows torch.optim's single-tensor reference order operation by operation (tests compare with it).
#include "optim.h"

namespace obb {

// (per-element arithmetic: sgd_one / adamw_one in optim.h, shared with the multi-group kernels of trainupd.hip)
__global__ __launch_bounds__(256) void k_sgd_step(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ buf, int64_t n, float lr, float mu,
                                                 float wd, int nesterov, int first) {
    const int64_t i4 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i4 >= n) return;
    const bool rd = !first && mu != 0.f;  // (momentum 0: `buf` may be NULL -- include/obbhip.h: "no buffer touched")
    if (i4 + 4 <= n) {
        float4 pv = *reinterpret_cast<const float4 *>(p + i4);
        const float4 gv = *reinterpret_cast<const float4 *>(g + i4);
        float4 bv = rd ? *reinterpret_cast<const float4 *>(buf + i4) : make_float4(0.f, 0.f, 0.f, 0.f);
        sgd_one(pv.x, gv.x, bv.x, lr, mu, wd, nesterov, first);
        sgd_one(pv.y, gv.y, bv.y, lr, mu, wd, nesterov, first);
        sgd_one(pv.z, gv.z, bv.z, lr, mu, wd, nesterov, first);
        sgd_one(pv.w, gv.w, bv.w, lr, mu, wd, nesterov, first);
        *reinterpret_cast<float4 *>(p + i4) = pv;
        if (mu != 0.f) *reinterpret_cast<float4 *>(buf + i4) = bv;
        return;
    }
    for (int64_t i = i4; i < n; ++i) {
        float b = rd ? buf[i] : 0.f;
        sgd_one(p[i], g[i], b, lr, mu, wd, nesterov, first);
        if (mu != 0.f) buf[i] = b;
    }
}

__global__ __launch_bounds__(256) void k_adamw_step(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m, float *__restrict__ v, int64_t n,
                                                   float lr, float omb1, float b2, float omb2, float eps, float wd, float step_size, float sqrt_bc2) {
    const int64_t i4 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i4 >= n) return;
    if (i4 + 4 <= n) {
        float4 pv = *reinterpret_cast<const float4 *>(p + i4), mv = *reinterpret_cast<const float4 *>(m + i4), vv = *reinterpret_cast<const float4 *>(v + i4);
        const float4 gv = *reinterpret_cast<const float4 *>(g + i4);
        adamw_one(pv.x, gv.x, mv.x, vv.x, lr, omb1, b2, omb2, eps, wd, step_size, sqrt_bc2);
        adamw_one(pv.y, gv.y, mv.y, vv.y, lr, omb1, b2, omb2, eps, wd, step_size, sqrt_bc2);
        adamw_one(pv.z, gv.z, mv.z, vv.z, lr, omb1, b2, omb2, eps, wd, step_size, sqrt_bc2);
        adamw_one(pv.w, gv.w, mv.w, vv.w, lr, omb1, b2, omb2, eps, wd, step_size, sqrt_bc2);
        *reinterpret_cast<float4 *>(p + i4) = pv;
        *reinterpret_cast<float4 *>(m + i4) = mv;
        *reinterpret_cast<float4 *>(v + i4) = vv;
        return;
    }
    for (int64_t i = i4; i < n; ++i) adamw_one(p[i], g[i], m[i], v[i], lr, omb1, b2, omb2, eps, wd, step_size, sqrt_bc2);
}

}  // namespace obb

using namespace obb;

extern "C" {

int obb_sgd_step(obb_ctx *ctx, float *param, const float *grad, float *momentum_buf, int64_t n, float lr, float momentum, float weight_decay,
                 int32_t nesterov, int32_t first_step, obb_stream_t s) {
    OBB_REQUIRE(ctx, ctx && n >= 0, "obb_sgd_step: bad arguments");
    if (n == 0) return OBB_OK;
    OBB_REQUIRE(ctx, param && grad && (momentum == 0.f || momentum_buf), "obb_sgd_step: NULL buffer");
    OBB_REQUIRE(ctx, !(nesterov && momentum <= 0.f), "obb_sgd_step: nesterov needs a momentum (as torch.optim.SGD)");
    OBB_REQUIRE(ctx, ((uintptr_t)param | (uintptr_t)grad | (uintptr_t)momentum_buf) % 16 == 0, "obb_sgd_step: buffers must be 16-byte aligned");
    const int64_t nb = (n + 1023) / 1024;
    OBB_REQUIRE(ctx, nb < (1ll << 31), "obb_sgd_step: n too large");
    hipLaunchKernelGGL(k_sgd_step, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)s, param, grad, momentum_buf, n, lr, momentum, weight_decay, nesterov, first_step);
    OBB_HIP(ctx, hipGetLastError());
    return OBB_OK;
}

int obb_adamw_step(obb_ctx *ctx, float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n, int64_t step, float lr, double beta1,
                   double beta2, float eps, float weight_decay, obb_stream_t s) {
    OBB_REQUIRE(ctx, ctx && n >= 0 && step >= 1, "obb_adamw_step: bad arguments (step counts from 1)");
    if (n == 0) return OBB_OK;
    OBB_REQUIRE(ctx, param && grad && exp_avg && exp_avg_sq, "obb_adamw_step: NULL buffer");
    OBB_REQUIRE(ctx, ((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) % 16 == 0, "obb_adamw_step: buffers must be 16-byte aligned");
    const AdamwConsts c = adamw_consts(beta1, beta2, step);
    const int64_t nb = (n + 1023) / 1024;
    OBB_REQUIRE(ctx, nb < (1ll << 31), "obb_adamw_step: n too large");
    hipLaunchKernelGGL(k_adamw_step, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)s, param, grad, exp_avg, exp_avg_sq, n, lr, c.omb1, c.b2, c.omb2, eps, weight_decay,
                       c.step_size(lr), c.sqrt_bc2);
    OBB_HIP(ctx, hipGetLastError());
    return OBB_OK;
}

}  // extern "C"
