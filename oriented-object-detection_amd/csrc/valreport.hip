// Validation, the report: the training loss of the engine's own head rows (obb_val_crit_decode, obb_val_crit_items) and the confusion matrix of the
// detections (obb_val_confusion).  Replaces, of the `val` pass `model.train(..., plots=True)` runs after every epoch (Train_OBB.py:792-841), the
// `self.loss += model.loss(batch, preds)[1]` of BaseValidator and `ConfusionMatrix.process_batch` of OBBValidator (Ultralytics 8.3.x restated from
// recall: the package is not installed, so parity with it is UNPINNED; pinned is the device against this repository's fp64 restatements,
// tests/criterion_ref.py and tests/valreport_ref.py).
//
// The criterion twins read obb_forward's `head float[B][A][NO]` in place (per anchor 64 DFL logits, nc class logits, 1 angle logit, padding up to
// NO = a multiple of 4: a row is 16-byte aligned, the padding is never read) and write no gradient.  The decode, the ProbIoU pair, the DFL side and
// the BCE element are loss_device.h's, the bodies obb_crit_decode / obb_crit_loss run: on equal logits the decode agrees bit for bit and the
// per-anchor loss elements are the same numbers.  Work split as in criterion.hip: four lanes per (image, anchor), one per side, the quad's values
// exchanged by __shfl; 256 lanes = 64 anchors per workgroup.
// Reduction of k_val_items, fixed order and no floating-point atomics: the 64 anchors of a workgroup go through an LDS tree in double (strides 32,
// 16, ... 1) -> one double per term and workgroup in the context's workspace; k_val_items_final, ONE workgroup, walks those partials strided by 256
// (ascending) and runs the same tree over its 256 lanes -> tss = max(float(sum of target_scores), 1), items[k] = float(sum_k gain_k / tss), added
// to what items holds when `accumulate` is set (one fp32 addition).  The sum of target_scores is the sum of the anchors' weights (each the
// ((0 + 1) + 2) + 3 of its quad's class partials).  Two runs give the same bits.
// UNMEASURED: the workgroup size of 256 is criterion.hip's, taken over so that both walk the anchors alike; nobody has timed 64, 128 or 512 here, nor
// the LDS tree against a wave-shuffle reduction (the tree's 6 + 8 barrier steps are noise next to the 64 expf per lane, by reasoning only).
//
// k_val_confusion: one 256-lane workgroup per image, like k_val_match, and the same ProbIoU (val_device.h), CLASS-AGNOSTIC.  Rule per image:
//   candidates = detections d < min(count, max_det) with conf > conf_thr, a class in [0, nc) and a finite box;
//   g(d) = the valid ground truth (unmasked, class in [0, nc), finite box) with the largest IoU > iou_thr, ties to the lower index;
//   of the candidates with g(d) = g the one with the largest IoU keeps g, ties to the lower detection index;
//   matrix[pred][gt] += 1 per kept pair, matrix[pred][nc] += 1 per candidate left without, matrix[nc][gt] += 1 per valid ground truth nobody kept.
// A lane owns detections tid, tid + 256, ...; it claims g(d) with ONE 64-bit LDS atomicMax over the key (IoU as an order-preserving integer, then
// ~d): a maximum, so the winner does not depend on the order of the claims.  After the barrier the lane evaluates g(d) again (the same arithmetic:
// the same bits; no per-detection scratch, so max_det has no upper limit) and compares.  The counts are integer atomicAdds into the caller's matrix:
// the sum does not depend on scheduling.  Latency-bound like k_val_match, and at twice its ProbIoU count.
#include "ctx.h"
#include "loss_device.h"
#include "val_device.h"

using namespace obb;

namespace {

constexpr int kMaxGt = OBB_VAL_MAX_GT;
constexpr int64_t kValMaxSum = (int64_t)4096 * 4096;  // obb_crit_*'s limit on B A nc, kept so that the two criteria accept the same batches

// the three levels of an h x w input (strides 8, 16, 32), as crit_anchor reads them; A = a2
struct ValLevels {
    int H0, H1, H2, W0, W1, W2, a0, a1, A;
};

__device__ __forceinline__ void val_load_side(const float *__restrict__ row, int side, float (&x)[kCritReg]) {
    const float4 *p = reinterpret_cast<const float4 *>(row + side * kCritReg);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float4 v = p[k];
        x[4 * k] = v.x; x[4 * k + 1] = v.y; x[4 * k + 2] = v.z; x[4 * k + 3] = v.w;
    }
}

__global__ __launch_bounds__(256) void k_val_decode(const float *__restrict__ head, int NO, ValLevels L, int B, int nc, float *__restrict__ pd_scores,
                                                   float *__restrict__ pd_bboxes, float *__restrict__ anc_points, float *__restrict__ stride) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t n = (int64_t)B * L.A;
    const bool live = (t >> 2) < n;
    const int64_t q = live ? (t >> 2) : n - 1;  // (a dead lane shadows the last anchor: the quad's shuffles stay whole; it stores nothing)
    const int side = (int)(t & 3), b = (int)(q / L.A), j = (int)(q - (int64_t)b * L.A);
    const CritAnchor an = crit_anchor(L.a0, L.a1, L.H0, L.H1, L.H2, L.W0, L.W1, L.W2, b, j);
    const float *row = head + q * NO;
    float x[kCritReg], e[kCritReg], m, se, E;
    val_load_side(row, side, x);
    const CritBox d = crit_decode_quad(x, e, m, se, E, row[64 + nc], an.ax, an.ay);
    if (!live) return;
    const float *cl = row + 64;
    for (int c = side; c < nc; c += 4) {
        float sig;
        (void)bce_elem(cl[c], 0.0f, sig);
        pd_scores[q * nc + c] = sig;
    }
    if (side == 0) {
        float *o = pd_bboxes + q * 5;
        o[0] = d.x * an.s; o[1] = d.y * an.s; o[2] = d.w * an.s; o[3] = d.h * an.s; o[4] = d.th;
        if (b == 0) { anc_points[j * 2] = an.ax * an.s; anc_points[j * 2 + 1] = an.ay * an.s; stride[j] = an.s; }
    }
}

// part: double [4][gridDim.x] = this workgroup's sums of the box, class and DFL elements (before the gains and 1 / tss) and of the anchors' weights
__global__ __launch_bounds__(256) void k_val_items(const float *__restrict__ head, int NO, ValLevels L, int B, int nc,
                                                  const float *__restrict__ target_bboxes, const float *__restrict__ target_scores,
                                                  const unsigned char *__restrict__ fg_mask, double *__restrict__ part) {
    __shared__ double sh[4][64];
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t n = (int64_t)B * L.A;
    const bool live = (t >> 2) < n;
    const int64_t q = live ? (t >> 2) : n - 1;
    const int side = (int)(t & 3), b = (int)(q / L.A), j = (int)(q - (int64_t)b * L.A);
    const CritAnchor an = crit_anchor(L.a0, L.a1, L.H0, L.H1, L.H2, L.W0, L.W1, L.W2, b, j);
    const float *row = head + q * NO;
    float x[kCritReg], e[kCritReg], m, se, E;
    val_load_side(row, side, x);
    const CritBox d = crit_decode_quad(x, e, m, se, E, row[64 + nc], an.ax, an.ay);
    // ---- class term: this lane's classes; the anchor's weight = sum_c target_scores (lane partials, then ((0 + 1) + 2) + 3)
    const float *cl = row + 64;
    const float *ts = target_scores + q * nc;
    float lcls = 0.f, wsum = 0.f;
    for (int c = side; c < nc; c += 4) {
        const float tc = ts[c];
        float sig;
        lcls += bce_elem(cl[c], tc, sig);
        wsum += tc;
    }
    lcls = ((__shfl(lcls, 0, 4) + __shfl(lcls, 1, 4)) + __shfl(lcls, 2, 4)) + __shfl(lcls, 3, 4);
    const float weight = ((__shfl(wsum, 0, 4) + __shfl(wsum, 1, 4)) + __shfl(wsum, 2, 4)) + __shfl(wsum, 3, 4);
    // ---- box terms (foreground anchors; the branch is uniform over the quad); the gradients the shared bodies return are dropped
    float lbox = 0.f, ldfl = 0.f;
    if (fg_mask[q] != 0) {
        const float *tb = target_bboxes + q * 5;
        const float is = 1.0f / an.s;  // (a power of two: exact)
        const float tx = tb[0] * is, ty = tb[1] * is, tw = tb[2] * is, th = tb[3] * is, tth = tb[4];
        float gp[5], g[kCritReg];
        lbox = probiou_pair(d.x, d.y, d.w, d.h, d.th, tx, ty, tw, th, tth, weight, 0.0f, gp);
        const float tgt = side == 0 ? an.ax - (tx - tw * 0.5f) : (side == 1 ? an.ay - (ty - th * 0.5f) : (side == 2 ? (tx + tw * 0.5f) - an.ax : (ty + th * 0.5f) - an.ay));
        ldfl = dfl_side<kCritReg>(x, e, m, se, tgt, weight * 0.25f, 0.0f, g);
    }
    ldfl = ((__shfl(ldfl, 0, 4) + __shfl(ldfl, 1, 4)) + __shfl(ldfl, 2, 4)) + __shfl(ldfl, 3, 4);
    const int a = threadIdx.x >> 2;
    if (side == 0) {
        sh[0][a] = live ? (double)lbox : 0.0; sh[1][a] = live ? (double)lcls : 0.0;
        sh[2][a] = live ? (double)ldfl : 0.0; sh[3][a] = live ? (double)weight : 0.0;
    }
    __syncthreads();
    const int k = threadIdx.x >> 6, i = threadIdx.x & 63;  // wave k reduces term k
    for (int s = 32; s >= 1; s >>= 1) {
        if (i < s) sh[k][i] += sh[k][i + s];
        __syncthreads();
    }
    if (i == 0) part[(int64_t)k * gridDim.x + blockIdx.x] = sh[k][0];
}

struct ValGains { float g[3]; };
__global__ __launch_bounds__(256) void k_val_items_final(const double *__restrict__ part, int nb, ValGains gains, int accumulate, float *__restrict__ items,
                                                        float *__restrict__ tss) {
    __shared__ double sh[4][256];
    const int tid = threadIdx.x;
    for (int k = 0; k < 4; ++k) {
        double acc = 0.0;
        for (int i = tid; i < nb; i += 256) acc += part[(int64_t)k * nb + i];
        sh[k][tid] = acc;
    }
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (tid < s)
            for (int k = 0; k < 4; ++k) sh[k][tid] += sh[k][tid + s];
        __syncthreads();
    }
    if (tid != 0) return;
    const float ts = fmaxf((float)sh[3][0], 1.0f);
    tss[0] = ts;
    const float r0 = (float)(sh[0][0] * (double)gains.g[0] / (double)ts), r1 = (float)(sh[1][0] * (double)gains.g[1] / (double)ts),
                r2 = (float)(sh[2][0] * (double)gains.g[2] / (double)ts);
    items[0] = accumulate ? items[0] + r0 : r0;
    items[1] = accumulate ? items[1] + r1 : r1;
    items[2] = accumulate ? items[2] + r2 : r2;
}

// a float as an unsigned integer of the same order (any sign; NaN never reaches here)
__device__ __forceinline__ unsigned ordered_bits(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(256) void k_val_confusion(const float *__restrict__ det, const int32_t *__restrict__ count, const int32_t *__restrict__ gt_labels,
                                                      const float *__restrict__ gt_bboxes, const uint8_t *__restrict__ mask_gt, int max_det, int n_cap, int nc,
                                                      float conf_thr, float iou_thr, int32_t *__restrict__ matrix) {
    __shared__ float gx[kMaxGt], gy[kMaxGt], gA[kMaxGt], gB[kMaxGt], gC[kMaxGt], gD[kMaxGt];
    __shared__ int glab[kMaxGt];                  // class, or -1: masked out, class outside [0, nc) or a non-finite box -- never matched, never counted
    __shared__ unsigned long long claim[kMaxGt];  // max over the claimants of (ordered IoU << 32 | ~d); 0: nobody
    const int b = blockIdx.x, tid = threadIdx.x;
    const int cnt = min(max(count[b], 0), max_det);
    const float *db = det + (int64_t)b * max_det * 7;
    const int ld = nc + 1;
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
        claim[g] = 0ull;
    }
    __syncthreads();
    // pass 0: claim; pass 1 (after the barrier): the same evaluation again, compared with the winners
    for (int pass = 0; pass < 2; ++pass) {
        for (int d = tid; d < cnt; d += 256) {
            const float *p = db + (int64_t)d * 7;
            const float x = p[0], y = p[1], w = p[2], h = p[3], cf = p[4], cl = p[5], t = p[6];
            if (!(cf > conf_thr) || !(cl >= 0.0f && cl < (float)nc) || !finite5(x, y, w, h, t)) continue;  // (a NaN confidence or class fails its comparison)
            float A, B, C;
            cov_terms(w, h, t, A, B, C);
            const float D = fmaxf(A * B - C * C, 0.0f);
            int bg = -1;
            float best = iou_thr;
            for (int g = 0; g < n_cap; ++g) {
                if (glab[g] < 0) continue;
                const float iou = probiou_cov(gx[g], gy[g], gA[g], gB[g], gC[g], gD[g], x, y, A, B, C, D);
                if (iou > best) { best = iou; bg = g; }  // strict: above the threshold, and a tie keeps the lower index; a NaN never wins
            }
            const unsigned long long key = ((unsigned long long)ordered_bits(best) << 32) | (unsigned)~(unsigned)d;
            if (pass == 0) {
                if (bg >= 0) atomicMax(&claim[bg], key);
            } else {
                const int pc = (int)cl;
                const bool kept = bg >= 0 && claim[bg] == key;
                atomicAdd(&matrix[pc * ld + (kept ? glab[bg] : nc)], 1);
            }
        }
        __syncthreads();
    }
    for (int g = tid; g < n_cap; g += 256)
        if (glab[g] >= 0 && claim[g] == 0ull) atomicAdd(&matrix[nc * ld + glab[g]], 1);
}

// shared argument checks of the two criterion twins + the level table; nothing is launched and no output is touched when this refuses
int val_levels(obb_ctx *ctx, const char *who, const float *head, int32_t B, int32_t h, int32_t w, int32_t nc, ValLevels &L, int &NO) {
    OBB_REQUIRE(ctx, ctx && head, "%s: NULL argument", who);
    OBB_REQUIRE(ctx, B >= 1 && nc >= 1 && nc <= 64, "%s: B = %d, nc = %d: B >= 1, 1 <= nc <= 64", who, (int)B, (int)nc);
    OBB_REQUIRE(ctx, h >= 32 && w >= 32 && h % 32 == 0 && w % 32 == 0 && h <= 32768 && w <= 32768, "%s: input %d x %d: h, w multiples of 32 in [32, 32768]",
                who, (int)h, (int)w);
    OBB_REQUIRE(ctx, ((uintptr_t)head & 15) == 0, "%s: head must be 16-byte aligned", who);
    L.H0 = h / 8; L.H1 = h / 16; L.H2 = h / 32; L.W0 = w / 8; L.W1 = w / 16; L.W2 = w / 32;
    const int64_t a0 = (int64_t)L.H0 * L.W0, a1 = a0 + (int64_t)L.H1 * L.W1, A = a1 + (int64_t)L.H2 * L.W2;
    OBB_REQUIRE(ctx, (int64_t)B * A * nc <= kValMaxSum, "%s: B A nc = %lld exceeds %lld elements", who, (long long)((int64_t)B * A * nc), (long long)kValMaxSum);
    L.a0 = (int)a0; L.a1 = (int)a1; L.A = (int)A;
    NO = (64 + nc + 1 + 3) / 4 * 4;
    return OBB_OK;
}

}  // namespace

extern "C" int obb_val_crit_decode(obb_ctx *ctx, const float *head, int32_t B, int32_t h, int32_t w, int32_t nc, float *pd_scores, float *pd_bboxes,
                                   float *anc_points, float *stride, obb_stream_t s) {
    ValLevels L;
    int NO;
    if (int rc = val_levels(ctx, "obb_val_crit_decode", head, B, h, w, nc, L, NO)) return rc;
    OBB_REQUIRE(ctx, pd_scores && pd_bboxes && anc_points && stride, "obb_val_crit_decode: NULL output");
    const unsigned nb = (unsigned)cdiv((int64_t)B * L.A * 4, 256);
    hipLaunchKernelGGL(k_val_decode, dim3(nb), dim3(256), 0, (hipStream_t)s, head, NO, L, (int)B, (int)nc, pd_scores, pd_bboxes, anc_points, stride);
    OBB_LAUNCH_CHECK(ctx);
    return OBB_OK;
}

extern "C" int obb_val_crit_items(obb_ctx *ctx, const float *head, int32_t B, int32_t h, int32_t w, int32_t nc, const float *target_bboxes,
                                  const float *target_scores, const uint8_t *fg_mask, const float *gains, float *items, float *tss, int32_t accumulate,
                                  obb_stream_t s) {
    ValLevels L;
    int NO;
    if (int rc = val_levels(ctx, "obb_val_crit_items", head, B, h, w, nc, L, NO)) return rc;
    OBB_REQUIRE(ctx, target_bboxes && target_scores && fg_mask && gains && items && tss, "obb_val_crit_items: NULL argument");
    const unsigned nb = (unsigned)cdiv((int64_t)B * L.A * 4, 256);
    double *part = (double *)ctx->workspace(WS_GEOM_A, sizeof(double) * (size_t)(4 * nb));
    if (!part) return set_error(ctx, OBB_ERR_HIP, "obb_val_crit_items: workspace allocation failed");
    ValGains g{{gains[0], gains[1], gains[2]}};
    hipStream_t st = (hipStream_t)s;
    hipLaunchKernelGGL(k_val_items, dim3(nb), dim3(256), 0, st, head, NO, L, (int)B, (int)nc, target_bboxes, target_scores, fg_mask, part);
    hipLaunchKernelGGL(k_val_items_final, dim3(1), dim3(256), 0, st, (const double *)part, (int)nb, g, (int)(accumulate != 0), items, tss);
    OBB_LAUNCH_CHECK(ctx);
    return OBB_OK;
}

extern "C" int obb_val_confusion(obb_ctx *ctx, const float *det, const int32_t *count, const int32_t *gt_labels, const float *gt_bboxes,
                                 const uint8_t *mask_gt, int32_t B, int32_t max_det, int32_t n_cap, int32_t nc, float conf_thr, float iou_thr,
                                 int32_t *matrix, obb_stream_t s) {
    const char *fn = "obb_val_confusion";
    OBB_REQUIRE(ctx, ctx && B >= 0, "%s: bad arguments", fn);
    OBB_REQUIRE(ctx, n_cap >= 1 && n_cap <= kMaxGt, "%s: n_cap = %d outside [1, %d]", fn, (int)n_cap, kMaxGt);
    OBB_REQUIRE(ctx, max_det >= 1, "%s: max_det = %d: at least 1", fn, (int)max_det);
    OBB_REQUIRE(ctx, nc >= 1 && nc <= 32766, "%s: nc = %d: 1..32766 (the matrix is indexed in int32)", fn, (int)nc);
    OBB_REQUIRE(ctx, conf_thr == conf_thr && iou_thr == iou_thr, "%s: a NaN threshold", fn);
    OBB_REQUIRE(ctx, det && count && gt_labels && gt_bboxes && mask_gt && matrix, "%s: NULL buffer", fn);
    if (B == 0) return OBB_OK;
    hipLaunchKernelGGL(k_val_confusion, dim3((unsigned)B), dim3(256), 0, (hipStream_t)s, det, count, gt_labels, gt_bboxes, mask_gt, (int)max_det, (int)n_cap,
                       (int)nc, conf_thr, iou_thr, matrix);
    OBB_LAUNCH_CHECK(ctx);
    return OBB_OK;
}
