// First slice of the training step (`model.train(...)`, Train_OBB.py:796-841 -> ultralytics==8.3.196
// v8OBBLoss -> RotatedBboxLoss): the ProbIoU rotated-box loss, forward AND backward in one kernel.
//
//   loss = sum_i (1 - probiou(pred_i, target_i)) * weight_i / target_scores_sum          
//   probiou: Gaussian (Bhattacharyya / Hellinger) overlap of the two boxes' covariance ellipses (Appendix A4, arXiv:2106.06072)
//
// One thread per matched (prediction, target) pair: the forward value and the closed-form gradient with respect to the prediction's
// (x, y, w, h, theta) come out of the same registers, so the pair's 40 + 4 bytes are read once and 4 + 20 bytes written -- an
// HBM-streaming kernel (68 B per pair).  The per-pair losses are summed by a second, tree-ordered launch (deterministic; no float
// atomics).  Gradients match torch.autograd on the same formula (tests/test_gpu_loss.py); clamps pass gradient inside their range and
// block it outside, like torch.clamp.
#include "ctx.h"
#include "loss_device.h"

namespace obb {

__global__ __launch_bounds__(256) void k_probiou_loss(const float *__restrict__ pred, const float *__restrict__ target, const float *__restrict__ weight,
                                                     int64_t n, float inv_tss, float *__restrict__ loss_elem, float *__restrict__ grad) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float wt = weight ? weight[i] : 1.0f;
    float g[5];
    loss_elem[i] = probiou_pair(pred[i * 5], pred[i * 5 + 1], pred[i * 5 + 2], pred[i * 5 + 3], pred[i * 5 + 4], target[i * 5], target[i * 5 + 1],
                                target[i * 5 + 2], target[i * 5 + 3], target[i * 5 + 4], wt, inv_tss, g);  // (csrc/loss_device.h)
    float *go = grad + i * 5;
    go[0] = g[0]; go[1] = g[1]; go[2] = g[2]; go[3] = g[3]; go[4] = g[4];
}

// deterministic sum: each block reduces 4096 consecutive values in a fixed tree, a second pass (same kernel, one block) reduces the partials
__global__ __launch_bounds__(256) void k_sum_f32(const float *__restrict__ v, int64_t n, float scale, float *__restrict__ out) {
    __shared__ double sh[256];
    const int64_t base = (int64_t)blockIdx.x * 4096;
    double acc = 0.0;
    for (int k = threadIdx.x; k < 4096; k += 256)
        if (base + k < n) acc += (double)v[base + k];
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int d = 128; d >= 1; d >>= 1) {
        if ((int)threadIdx.x < d) sh[threadIdx.x] += sh[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = (float)(sh[0] * (double)scale);
}


// ---- DFL (distribution focal loss) of the box branch: per (box, side) a 16-way distribution over integer distances; the target distance
// t in [0, reg_max - 1) is shared out between its two neighbouring bins:  l = CE(logits, floor t) * (ceil' - t) + CE(logits, floor t + 1) *
// (t - floor t); per box the mean over the 4 sides, times the box weight, over target_scores_sum (ultralytics DFLoss + RotatedBboxLoss).
// One thread per (box, side): 16 logits in, 16 gradients out: d l / d logit_k = softmax_k - (wl [k = tl] + wr [k = tr]).
template <int R>
__global__ __launch_bounds__(256) void k_dfl_loss(const float *__restrict__ logits, const float *__restrict__ target, const float *__restrict__ weight,
                                                 int64_t n4, float inv_tss, float *__restrict__ loss_elem, float *__restrict__ grad) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;  // (box, side)
    if (i >= n4) return;
    float x[R];
#pragma unroll
    for (int k = 0; k < R; k += 4) {
        const float4 v = *reinterpret_cast<const float4 *>(logits + i * R + k);
        x[k] = v.x; x[k + 1] = v.y; x[k + 2] = v.z; x[k + 3] = v.w;
    }
    float e[R], g[R], m, se;
    softmax_parts<R>(x, e, m, se);
    const float wt = (weight ? weight[i >> 2] : 1.0f) * 0.25f;
    loss_elem[i] = dfl_side<R>(x, e, m, se, target[i], wt, wt * inv_tss, g);  // (csrc/loss_device.h)
#pragma unroll
    for (int k = 0; k < R; k += 4) *reinterpret_cast<float4 *>(grad + i * R + k) = make_float4(g[k], g[k + 1], g[k + 2], g[k + 3]);
}

// ---- classification term: BCEWithLogitsLoss(reduction="none")(logits, targets).sum() / target_scores_sum (v8OBBLoss), element-wise:
// l = max(x, 0) - x t + log(1 + exp(-|x|)),  d l / d x = sigmoid(x) - t
__global__ __launch_bounds__(256) void k_bce_loss(const float *__restrict__ logits, const float *__restrict__ target, int64_t n, float inv_tss,
                                                 float *__restrict__ loss_elem, float *__restrict__ grad) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float t = target[i];
    float sig;
    loss_elem[i] = bce_elem(logits[i], t, sig);  // (csrc/loss_device.h)
    grad[i] = (sig - t) * inv_tss;
}

}  // namespace obb

using namespace obb;

// deterministic sum of elem[0..n) * scale -> *loss (tree of k_sum_f32 launches)
static int sum_to_scalar(obb_ctx *ctx, const float *elem, int64_t n, float scale, float *loss, hipStream_t st, const char *who) {
    const int64_t nb1 = cdiv(n, 4096), nb2 = cdiv(nb1, 4096);
    OBB_REQUIRE(ctx, nb2 <= 4096, "%s: n too large", who);
    float *part = (float *)ctx->workspace(WS_GEOM_B, sizeof(float) * (size_t)(nb1 + nb2 + 8));
    if (!part) return set_error(ctx, OBB_ERR_HIP, "%s: workspace allocation failed", who);
    if (nb1 == 1) {
        hipLaunchKernelGGL(k_sum_f32, dim3(1), dim3(256), 0, st, elem, n, scale, loss);
    } else {
        hipLaunchKernelGGL(k_sum_f32, dim3((unsigned)nb1), dim3(256), 0, st, elem, n, 1.0f, part);
        if (nb2 == 1) hipLaunchKernelGGL(k_sum_f32, dim3(1), dim3(256), 0, st, (const float *)part, nb1, scale, loss);
        else {
            hipLaunchKernelGGL(k_sum_f32, dim3((unsigned)nb2), dim3(256), 0, st, (const float *)part, nb1, 1.0f, part + nb1);
            hipLaunchKernelGGL(k_sum_f32, dim3(1), dim3(256), 0, st, (const float *)(part + nb1), nb2, scale, loss);
        }
    }
    OBB_LAUNCH_CHECK(ctx);
    return OBB_OK;
}

extern "C" int obb_dfl_loss(obb_ctx *ctx, const float *pred_dist, const float *target_ltrb, const float *weight, int64_t n, int32_t reg_max,
                            float target_scores_sum, float *loss, float *grad_pred, obb_stream_t s) {
    OBB_REQUIRE(ctx, ctx && n >= 0 && loss, "obb_dfl_loss: bad arguments");
    hipStream_t st = (hipStream_t)s;
    if (n == 0) { OBB_HIP(ctx, hipMemsetAsync(loss, 0, sizeof(float), st)); return OBB_OK; }
    OBB_REQUIRE(ctx, pred_dist && target_ltrb && grad_pred, "obb_dfl_loss: NULL buffer");
    OBB_REQUIRE(ctx, reg_max == 16, "obb_dfl_loss: reg_max %d unsupported (the OBB head uses 16 bins)", reg_max);
    OBB_REQUIRE(ctx, target_scores_sum > 0.0f, "obb_dfl_loss: target_scores_sum must be positive");
    OBB_REQUIRE(ctx, (((uintptr_t)pred_dist | (uintptr_t)grad_pred) & 15) == 0, "obb_dfl_loss: logits and gradient rows must be 16-byte aligned");
    const int64_t n4 = n * 4;
    float *elem = (float *)ctx->workspace(WS_GEOM_A, sizeof(float) * (size_t)n4);
    if (!elem) return set_error(ctx, OBB_ERR_HIP, "obb_dfl_loss: workspace allocation failed");
    hipLaunchKernelGGL(k_dfl_loss<16>, dim3((unsigned)cdiv(n4, 256)), dim3(256), 0, st, pred_dist, target_ltrb, weight, n4, 1.0f / target_scores_sum, elem, grad_pred);
    OBB_LAUNCH_CHECK(ctx);
    return sum_to_scalar(ctx, elem, n4, 1.0f / target_scores_sum, loss, st, "obb_dfl_loss");
}

extern "C" int obb_bce_loss(obb_ctx *ctx, const float *logits, const float *targets, int64_t n, float target_scores_sum, float *loss, float *grad_logits,
                            obb_stream_t s) {
    OBB_REQUIRE(ctx, ctx && n >= 0 && loss, "obb_bce_loss: bad arguments");
    hipStream_t st = (hipStream_t)s;
    if (n == 0) { OBB_HIP(ctx, hipMemsetAsync(loss, 0, sizeof(float), st)); return OBB_OK; }
    OBB_REQUIRE(ctx, logits && targets && grad_logits, "obb_bce_loss: NULL buffer");
    OBB_REQUIRE(ctx, target_scores_sum > 0.0f, "obb_bce_loss: target_scores_sum must be positive");
    float *elem = (float *)ctx->workspace(WS_GEOM_A, sizeof(float) * (size_t)n);
    if (!elem) return set_error(ctx, OBB_ERR_HIP, "obb_bce_loss: workspace allocation failed");
    hipLaunchKernelGGL(k_bce_loss, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, st, logits, targets, n, 1.0f / target_scores_sum, elem, grad_logits);
    OBB_LAUNCH_CHECK(ctx);
    return sum_to_scalar(ctx, elem, n, 1.0f / target_scores_sum, loss, st, "obb_bce_loss");
}

extern "C" int obb_probiou_loss(obb_ctx *ctx, const float *pred, const float *target, const float *weight, int64_t n, float target_scores_sum,
                                float *loss, float *grad_pred, obb_stream_t s) {
    OBB_REQUIRE(ctx, ctx && n >= 0 && loss, "obb_probiou_loss: bad arguments");
    hipStream_t st = (hipStream_t)s;
    if (n == 0) { OBB_HIP(ctx, hipMemsetAsync(loss, 0, sizeof(float), st)); return OBB_OK; }
    OBB_REQUIRE(ctx, pred && target && grad_pred, "obb_probiou_loss: NULL buffer");
    OBB_REQUIRE(ctx, target_scores_sum > 0.0f, "obb_probiou_loss: target_scores_sum must be positive");
    const int64_t nb1 = cdiv(n, 4096), nb2 = cdiv(nb1, 4096);
    OBB_REQUIRE(ctx, nb2 <= 4096, "obb_probiou_loss: n too large");
    float *elem = (float *)ctx->workspace(WS_GEOM_A, sizeof(float) * (size_t)n);
    float *part = (float *)ctx->workspace(WS_GEOM_B, sizeof(float) * (size_t)(nb1 + nb2 + 8));
    if (!elem || !part) return set_error(ctx, OBB_ERR_HIP, "obb_probiou_loss: workspace allocation failed");
    hipLaunchKernelGGL(k_probiou_loss, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, st, pred, target, weight, n, 1.0f / target_scores_sum, elem, grad_pred);
    OBB_LAUNCH_CHECK(ctx);
    const float inv = 1.0f / target_scores_sum;
    if (nb1 == 1) {
        hipLaunchKernelGGL(k_sum_f32, dim3(1), dim3(256), 0, st, (const float *)elem, n, inv, loss);
    } else {
        hipLaunchKernelGGL(k_sum_f32, dim3((unsigned)nb1), dim3(256), 0, st, (const float *)elem, n, 1.0f, part);
        if (nb2 == 1) hipLaunchKernelGGL(k_sum_f32, dim3(1), dim3(256), 0, st, (const float *)part, nb1, inv, loss);
        else {
            hipLaunchKernelGGL(k_sum_f32, dim3((unsigned)nb2), dim3(256), 0, st, (const float *)part, nb1, 1.0f, part + nb1);
            hipLaunchKernelGGL(k_sum_f32, dim3(1), dim3(256), 0, st, (const float *)(part + nb1), nb2, inv, loss);
        }
    }
    OBB_LAUNCH_CHECK(ctx);
    return OBB_OK;
}
