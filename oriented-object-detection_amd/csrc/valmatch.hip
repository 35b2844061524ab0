// Validation, the matching step: which detections of an image are true positives at each IoU threshold.
//
// Replaces `OBBValidator._process_batch` = `batch_probiou(gt_bboxes, pred_bboxes)` + `match_predictions(pred_cls, gt_cls, iou)` of the `val` pass
// `model.train(...)` runs after every epoch (Train_OBB.py:792-841; Ultralytics 8.3.x restated from recall: the package is not installed, so parity
// with it is UNPINNED; pinned is the device against this repository's fp64 restatement, tests/val_ref.py).
//
// Rule, per image and threshold i (thr = float32(linspace(0.5, 0.95, 10)), passed in by the host):
//   g(d)   the class-equal, unmasked ground truth with the largest ProbIoU to detection d, ties to the lower index;
//   d claims g(d) iff iou(d, g(d)) >= thr_i;  among the detections claiming one ground truth the LOWEST index (detections are in score order: the
//   most confident) is the true positive.  A detection that loses its ground truth does not fall back to its second best.
// k_val_match: one 256-lane workgroup per image.  The ground truths' covariance terms go to LDS once; a lane owns detections tid, tid + 256, ...: it
// evaluates ProbIoU against every class-equal ground truth, keeps the best, and claims it with an LDS atomicMin over the detection index per
// (ground truth, threshold) -- a minimum, so the result does not depend on the order of the claims.  After the barrier the same lane compares its
// index with the winners and writes the threshold bits.  ProbIoU is the covariance form of batch_probiou (eps 1e-7) in fp32, restated here in the
// operation order of the torch expression, in val_device.h (decode.hip's NMS form keeps its own code: its bit-exact tests pin it).
// Latency-bound: per image ~8 KB of detections and < 2 KB of ground truth are read and count x n_gt ProbIoUs evaluated; nothing is reused across
// images, and one workgroup per image leaves most of the chip idle at validation batch sizes.
#include "ctx.h"
#include "val_device.h"

using namespace obb;

namespace {

constexpr int kMaxGt = OBB_VAL_MAX_GT, kMaxThr = OBB_VAL_MAX_THR;

__global__ __launch_bounds__(256) void k_val_match(const float *__restrict__ det, const int32_t *__restrict__ count, const int32_t *__restrict__ gt_labels,
                                                  const float *__restrict__ gt_bboxes, const uint8_t *__restrict__ mask_gt, int max_det, int n_cap, int nc,
                                                  const float *__restrict__ thr, int n_thr, uint16_t *__restrict__ tp, float *__restrict__ best_iou,
                                                  int32_t *__restrict__ best_gt) {
    __shared__ float gx[kMaxGt], gy[kMaxGt], gA[kMaxGt], gB[kMaxGt], gC[kMaxGt], gD[kMaxGt], sthr[kMaxThr];
    __shared__ int glab[kMaxGt];             // class, or -1: masked out, class outside [0, nc) or a non-finite box -- never matched
    __shared__ int winner[kMaxGt * kMaxThr];  // [g * n_thr + i]: the lowest detection index claiming g at threshold i
    const int b = blockIdx.x, tid = threadIdx.x;
    const int cnt = min(max(count[b], 0), max_det);
    const float *db = det + (int64_t)b * max_det * 7;
    uint16_t *tpb = tp + (int64_t)b * max_det;
    float *bib = best_iou + (int64_t)b * max_det;
    int32_t *bgb = best_gt + (int64_t)b * max_det;
    for (int g = tid; g < n_cap; g += 256) {
        const int64_t row = (int64_t)b * n_cap + g;
        const float *p = gt_bboxes + row * 5;
        const int lab = gt_labels[row];
        const float x = p[0], y = p[1], w = p[2], h = p[3], t = p[4];
        const bool ok = mask_gt[row] != 0 && lab >= 0 && lab < nc && finite5(x, y, w, h, t);
        float A = 0.f, B = 0.f, C = 0.f;
        if (ok) cov_terms(w, h, t, A, B, C);
        gx[g] = ok ? x : 0.f; gy[g] = ok ? y : 0.f; gA[g] = A; gB[g] = B; gC[g] = C; gD[g] = fmaxf(A * B - C * C, 0.0f);
        glab[g] = ok ? lab : -1;
    }
    for (int i = tid; i < n_cap * n_thr; i += 256) winner[i] = 0x7fffffff;
    if (tid < n_thr) sthr[tid] = thr[tid];
    __syncthreads();
    for (int d = tid; d < max_det; d += 256) {
        int bg = -1;
        float bi = 0.0f;
        if (d < cnt) {
            const float *p = db + (int64_t)d * 7;
            const float x = p[0], y = p[1], w = p[2], h = p[3], cf = p[5], t = p[6];
            if (cf >= 0.0f && cf < (float)nc && finite5(x, y, w, h, t)) {  // (a NaN class fails both comparisons)
                const int c = (int)cf;
                float A, B, C;
                cov_terms(w, h, t, A, B, C);
                const float D = fmaxf(A * B - C * C, 0.0f);
                float best = -1.0f;
                for (int g = 0; g < n_cap; ++g) {
                    if (glab[g] != c) continue;
                    const float iou = probiou_cov(gx[g], gy[g], gA[g], gB[g], gC[g], gD[g], x, y, A, B, C, D);
                    if (iou > best) { best = iou; bg = g; }  // strict: a tie keeps the lower index; a NaN never wins
                }
                if (bg >= 0) {
                    bi = best;
                    for (int i = 0; i < n_thr; ++i)
                        if (bi >= sthr[i]) atomicMin(&winner[bg * n_thr + i], d);
                }
            }
        }
        bib[d] = bi; bgb[d] = bg;
    }
    __syncthreads();
    for (int d = tid; d < max_det; d += 256) {  // (the lane that wrote best_iou / best_gt of d reads them back)
        const int bg = bgb[d];
        const float bi = bib[d];
        unsigned bits = 0;
        if (bg >= 0)
            for (int i = 0; i < n_thr; ++i)
                if (bi >= sthr[i] && winner[bg * n_thr + i] == d) bits |= 1u << i;
        tpb[d] = (uint16_t)bits;
    }
}

}  // namespace

extern "C" int obb_val_match(obb_ctx *ctx, const float *det, const int32_t *count, const int32_t *gt_labels, const float *gt_bboxes, const uint8_t *mask_gt,
                             int32_t B, int32_t max_det, int32_t n_cap, int32_t nc, const float *thr, int32_t n_thr, uint16_t *tp, float *best_iou,
                             int32_t *best_gt, obb_stream_t s) {
    const char *fn = "obb_val_match";
    OBB_REQUIRE(ctx, ctx && B >= 0, "%s: bad arguments", fn);
    OBB_REQUIRE(ctx, n_cap >= 1 && n_cap <= kMaxGt, "%s: n_cap = %d outside [1, %d]", fn, (int)n_cap, kMaxGt);
    OBB_REQUIRE(ctx, max_det >= 1, "%s: max_det = %d: at least 1", fn, (int)max_det);
    OBB_REQUIRE(ctx, nc >= 1 && n_thr >= 1 && n_thr <= kMaxThr, "%s: nc = %d, %d thresholds: nc >= 1 and 1..%d thresholds (one bit each)", fn, (int)nc,
                (int)n_thr, kMaxThr);
    OBB_REQUIRE(ctx, det && count && gt_labels && gt_bboxes && mask_gt && thr && tp && best_iou && best_gt, "%s: NULL buffer", fn);
    if (B == 0) return OBB_OK;
    hipLaunchKernelGGL(k_val_match, dim3((unsigned)B), dim3(256), 0, (hipStream_t)s, det, count, gt_labels, gt_bboxes, mask_gt, (int)max_det, (int)n_cap,
                       (int)nc, thr, (int)n_thr, tp, best_iou, best_gt);
    OBB_LAUNCH_CHECK(ctx);
    return OBB_OK;
}
