// The fused OBB training criterion (`model.train(...)`, Train_OBB.py:796-841 -> ultralytics==8.3.x v8OBBLoss.__call__,
// restated from recall: the package is not installed, parity UNPINNED): head logits in the head's own per-level NHWC layouts -> the assigner's
// inputs (obb_crit_decode) and, given the assignment, the three loss terms with the gradient of every logit (obb_crit_loss).
//
//   decode, per anchor:  p = softmax over the 16 bins of a side, (l, t, r, b) = sum_k k p_k, theta = (sigmoid(a) - 0.25) pi,
//                        xf = (r - l) / 2, yf = (b - t) / 2, x = ax + xf cos - yf sin, y = ay + xf sin + yf cos, w = l + r, h = t + b   (grid units)
//   terms:               L_box = sum_fg (1 - probiou(pred, target / s)) weight / tss,  L_dfl = sum_fg DFL(logits, ltrb(target / s)) weight / tss,
//                        L_cls = sum_all BCE(class logits, target_scores) / tss,  weight = sum_c target_scores, tss = max(sum target_scores, 1)
//   gradients:           of B (g_box L_box + g_cls L_cls + g_dfl L_dfl), the chain rule through the decode in closed form.
//
// Work split: FOUR LANES PER (image, anchor), one per side.  A lane reads its side's 16 logits as 16-byte chunks (2 for bf16, 4 for fp32), keeps them
// and their exponentials in registers (compile-time indices: no scratch), and the four expectations travel between the lanes of the quad by
// __shfl.  Every lane of the quad then evaluates the pair's ProbIoU (the same arithmetic: the same bits) and finishes its own side: 16 gradients
// out as two 16-byte bf16 stores.  The nc classes are dealt round-robin to the quad's lanes.  Anchor index -> (level, y, x) by two compares.
// fp32 arithmetic, no atomics; the sums run in k_crit_sum's fixed tree (the tree of loss.hip's k_sum_f32); tss stays on the device and the
// loss kernel reads it through the pointer, so nothing returns to the host and the whole criterion is stream-ordered and capturable.
#include "ctx.h"
#include "loss_device.h"
#include "traindev.h"

namespace obb {

constexpr int kCritLevels = 3;

struct CritLevels {
    const void *box[kCritLevels];    // [B,H,W,64] bf16 or fp32
    const float *cls[kCritLevels];   // [B,H,W,nc]
    const float *ang[kCritLevels];   // [B,H,W,1]
    void *d_box[kCritLevels];        // bf16 [B,H,W,64]
    float *d_cls[kCritLevels];
    float *d_ang[kCritLevels];
    int H[kCritLevels], W[kCritLevels];
    int a0, a1, A;                   // anchors of level 0, of levels 0 + 1, of all three
};

template <typename TB>
__device__ __forceinline__ void crit_load_side(const void *base, int64_t row, int side, float (&x)[kCritReg]);
template <>
__device__ __forceinline__ void crit_load_side<float>(const void *base, int64_t row, int side, float (&x)[kCritReg]) {
    const float4 *p = reinterpret_cast<const float4 *>(reinterpret_cast<const float *>(base) + row * 64 + side * kCritReg);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float4 v = p[k];
        x[4 * k] = v.x; x[4 * k + 1] = v.y; x[4 * k + 2] = v.z; x[4 * k + 3] = v.w;
    }
}
template <>
__device__ __forceinline__ void crit_load_side<unsigned short>(const void *base, int64_t row, int side, float (&x)[kCritReg]) {
    const uint4 *p = reinterpret_cast<const uint4 *>(reinterpret_cast<const unsigned short *>(base) + row * 64 + side * kCritReg);
#pragma unroll
    for (int k = 0; k < 2; ++k) unpack8_bf16(p[k], x + 8 * k);
}

// (the level table is read through its constant indices only: a run-time index or a reference to it would copy the kernel argument to scratch)
#define CRIT_PICK(L, f, lv) ((lv) == 0 ? (L).f[0] : ((lv) == 1 ? (L).f[1] : (L).f[2]))
#define CRIT_ANCHOR(L, b, j) crit_anchor((L).a0, (L).a1, (L).H[0], (L).H[1], (L).H[2], (L).W[0], (L).W[1], (L).W[2], b, j)

template <typename TB>
__global__ __launch_bounds__(256) void k_crit_decode(CritLevels L, int B, int nc, float *__restrict__ pd_scores, float *__restrict__ pd_bboxes,
                                                    float *__restrict__ anc_points, float *__restrict__ stride) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t n = (int64_t)B * L.A;
    const bool live = (t >> 2) < n;
    const int64_t q = live ? (t >> 2) : n - 1;  // (a dead lane shadows the last anchor: the quad's shuffles stay whole; it stores nothing)
    const int side = (int)(t & 3), b = (int)(q / L.A), j = (int)(q - (int64_t)b * L.A);
    const CritAnchor an = CRIT_ANCHOR(L, b, j);
    float x[kCritReg], e[kCritReg], m, se, E;
    crit_load_side<TB>(CRIT_PICK(L, box, an.lv), an.row, side, x);
    const float a = CRIT_PICK(L, ang, an.lv)[an.row];
    const CritBox d = crit_decode_quad(x, e, m, se, E, a, an.ax, an.ay);
    if (!live) return;
    const float *cl = CRIT_PICK(L, cls, an.lv) + an.row * nc;
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

// elem: [3][n] per-(image, anchor) loss elements (box, cls, dfl), before the gains and 1 / tss
template <typename TB>
__global__ __launch_bounds__(256) void k_crit_loss(CritLevels L, int B, int nc, const float *__restrict__ target_bboxes,
                                                  const float *__restrict__ target_scores, const unsigned char *__restrict__ fg_mask,
                                                  const float *__restrict__ tss, float g_box, float g_cls, float g_dfl, float *__restrict__ elem) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t n = (int64_t)B * L.A;
    const bool live = (t >> 2) < n;
    const int64_t q = live ? (t >> 2) : n - 1;
    const int side = (int)(t & 3), b = (int)(q / L.A), j = (int)(q - (int64_t)b * L.A);
    const CritAnchor an = CRIT_ANCHOR(L, b, j);
    float x[kCritReg], e[kCritReg], m, se, E;
    crit_load_side<TB>(CRIT_PICK(L, box, an.lv), an.row, side, x);
    const float a = CRIT_PICK(L, ang, an.lv)[an.row];
    const CritBox d = crit_decode_quad(x, e, m, se, E, a, an.ax, an.ay);
    const float inv_tss = 1.0f / tss[0], fB = (float)B;
    // ---- class term: this lane's classes; the anchor's weight = sum_c target_scores (lane partials, then ((0 + 1) + 2) + 3)
    const float sc_cls = fB * g_cls * inv_tss;
    const float *cl = CRIT_PICK(L, cls, an.lv) + an.row * nc;
    float *dcl = CRIT_PICK(L, d_cls, an.lv) + an.row * nc;
    const float *ts = target_scores + q * nc;
    float lcls = 0.f, wsum = 0.f;
    for (int c = side; c < nc; c += 4) {
        const float tc = ts[c];
        float sig;
        lcls += bce_elem(cl[c], tc, sig);
        wsum += tc;
        if (live) dcl[c] = (sig - tc) * sc_cls;
    }
    lcls = ((__shfl(lcls, 0, 4) + __shfl(lcls, 1, 4)) + __shfl(lcls, 2, 4)) + __shfl(lcls, 3, 4);
    const float weight = ((__shfl(wsum, 0, 4) + __shfl(wsum, 1, 4)) + __shfl(wsum, 2, 4)) + __shfl(wsum, 3, 4);
    // ---- box terms (foreground anchors; the branch is uniform over the quad)
    const bool fg = fg_mask[q] != 0;
    float lbox = 0.f, ldfl = 0.f, g[kCritReg], dang = 0.f;
#pragma unroll
    for (int k = 0; k < kCritReg; ++k) g[k] = 0.f;
    if (fg) {
        const float *tb = target_bboxes + q * 5;
        const float is = 1.0f / an.s;  // (a power of two: exact)
        const float tx = tb[0] * is, ty = tb[1] * is, tw = tb[2] * is, th = tb[3] * is, tth = tb[4];
        float gp[5];
        lbox = probiou_pair(d.x, d.y, d.w, d.h, d.th, tx, ty, tw, th, tth, weight, fB * g_box * inv_tss, gp);
        const float u = gp[0] * d.c + gp[1] * d.s, v = -gp[0] * d.s + gp[1] * d.c;
        const float dside = side == 0 ? gp[2] - u * 0.5f : (side == 1 ? gp[3] - v * 0.5f : (side == 2 ? gp[2] + u * 0.5f : gp[3] + v * 0.5f));
        const float dth = gp[4] + gp[0] * (-d.xf * d.s - d.yf * d.c) + gp[1] * (d.xf * d.c - d.yf * d.s);
        dang = dth * (kCritPi * (d.sig * (1.0f - d.sig)));
        // bbox2dist of this lane's side (the clamp to [0, reg_max - 1.01] is dfl_side's)
        const float tgt = side == 0 ? an.ax - (tx - tw * 0.5f) : (side == 1 ? an.ay - (ty - th * 0.5f) : (side == 2 ? (tx + tw * 0.5f) - an.ax : (ty + th * 0.5f) - an.ay));
        const float wt = weight * 0.25f;
        ldfl = dfl_side<kCritReg>(x, e, m, se, tgt, wt, wt * (fB * g_dfl * inv_tss), g);
        const float inv_se = 1.0f / se;
#pragma unroll
        for (int k = 0; k < kCritReg; ++k) g[k] = (e[k] * inv_se) * ((float)k - E) * dside + g[k];
    }
    ldfl = ((__shfl(ldfl, 0, 4) + __shfl(ldfl, 1, 4)) + __shfl(ldfl, 2, 4)) + __shfl(ldfl, 3, 4);
    if (!live) return;
    uint4 *o = reinterpret_cast<uint4 *>(reinterpret_cast<unsigned short *>(CRIT_PICK(L, d_box, an.lv)) + an.row * 64 + side * kCritReg);
    o[0] = pack8_bf16(g);  // traindev.h's rounding
    o[1] = pack8_bf16(g + 8);
    if (side == 0) {
        CRIT_PICK(L, d_ang, an.lv)[an.row] = dang;
        elem[q] = lbox; elem[n + q] = lcls; elem[2 * n + q] = ldfl;
    }
}

// The fixed sum tree (loss.hip's k_sum_f32: 4096 consecutive values per block, double inside a block, one fp32 rounding per block), blockIdx.y =
// which of up to three arrays (v + y n -> out + y out_stride).  mode 0: partial sums; 1: out = max(sum, 1) (tss); 2: out = gain[y] * sum / tss.
struct CritGains { float g[3]; };
__global__ __launch_bounds__(256) void k_crit_sum(const float *__restrict__ v, int64_t n, int mode, CritGains gains, const float *__restrict__ tss,
                                                 float *__restrict__ out, int64_t out_stride) {
    __shared__ double sh[256];
    const int64_t base = (int64_t)blockIdx.x * 4096;
    v += (int64_t)blockIdx.y * n;
    double acc = 0.0;
    for (int k = threadIdx.x; k < 4096; k += 256)
        if (base + k < n) acc += (double)v[base + k];
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int d = 128; d >= 1; d >>= 1) {
        if ((int)threadIdx.x < d) sh[threadIdx.x] += sh[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    float r = (float)sh[0];
    if (mode == 1) r = fmaxf(r, 1.0f);
    if (mode == 2) {
        const float gy = blockIdx.y == 0 ? gains.g[0] : (blockIdx.y == 1 ? gains.g[1] : gains.g[2]);
        r = (float)(sh[0] * (double)gy / (double)tss[0]);
    }
    out[(int64_t)blockIdx.y * out_stride + blockIdx.x] = r;
}

}  // namespace obb

using namespace obb;

static const int64_t kCritMaxSum = (int64_t)4096 * 4096;  // two levels of the sum tree

// shared argument checks + the level table; nothing is launched and no output is touched when this refuses
static int crit_levels(obb_ctx *ctx, const char *who, const void *const *box, const float *const *cls, const float *const *angle, const int32_t *H,
                       const int32_t *W, int32_t B, int32_t nc, CritLevels &L) {
    OBB_REQUIRE(ctx, ctx && box && cls && angle && H && W, "%s: NULL argument", who);
    OBB_REQUIRE(ctx, B >= 1 && nc >= 1 && nc <= 64, "%s: B = %d, nc = %d: B >= 1, 1 <= nc <= 64", who, B, nc);
    int64_t A = 0;
    for (int i = 0; i < kCritLevels; ++i) {
        OBB_REQUIRE(ctx, H[i] >= 1 && W[i] >= 1 && H[i] <= 4096 && W[i] <= 4096, "%s: level %d is %d x %d: H, W in [1, 4096]", who, i, H[i], W[i]);
        OBB_REQUIRE(ctx, box[i] && cls[i] && angle[i], "%s: NULL logits at level %d", who, i);
        OBB_REQUIRE(ctx, ((uintptr_t)box[i] & 15) == 0, "%s: box logits of level %d must be 16-byte aligned", who, i);
        L.box[i] = box[i]; L.cls[i] = cls[i]; L.ang[i] = angle[i];
        L.d_box[i] = nullptr; L.d_cls[i] = nullptr; L.d_ang[i] = nullptr;
        L.H[i] = H[i]; L.W[i] = W[i];
        A += (int64_t)H[i] * W[i];
        if (i == 0) L.a0 = (int)A;
        if (i == 1) L.a1 = (int)A;
    }
    OBB_REQUIRE(ctx, (int64_t)B * A * nc <= kCritMaxSum, "%s: B A nc = %lld exceeds the sum tree's %lld elements", who, (long long)((int64_t)B * A * nc),
                (long long)kCritMaxSum);
    L.A = (int)A;
    return OBB_OK;
}

extern "C" int obb_crit_decode(obb_ctx *ctx, const void *const *box, int32_t box_bf16, const float *const *cls, const float *const *angle, const int32_t *H,
                               const int32_t *W, int32_t B, int32_t nc, float *pd_scores, float *pd_bboxes, float *anc_points, float *stride,
                               obb_stream_t s) {
    CritLevels L;
    if (int rc = crit_levels(ctx, "obb_crit_decode", box, cls, angle, H, W, B, nc, L)) return rc;
    OBB_REQUIRE(ctx, pd_scores && pd_bboxes && anc_points && stride, "obb_crit_decode: NULL output");
    hipStream_t st = (hipStream_t)s;
    const unsigned nb = (unsigned)cdiv((int64_t)B * L.A * 4, 256);
    if (box_bf16) hipLaunchKernelGGL(k_crit_decode<unsigned short>, dim3(nb), dim3(256), 0, st, L, B, nc, pd_scores, pd_bboxes, anc_points, stride);
    else hipLaunchKernelGGL(k_crit_decode<float>, dim3(nb), dim3(256), 0, st, L, B, nc, pd_scores, pd_bboxes, anc_points, stride);
    OBB_LAUNCH_CHECK(ctx);
    return OBB_OK;
}

// v[ny][n] -> out[y] through the tree (mode 1 or 2 at the last level)
static void crit_sum(const float *v, int64_t n, int ny, int mode, CritGains gains, const float *tss, float *part, float *out, hipStream_t st) {
    const int64_t nb1 = cdiv(n, 4096);
    if (nb1 == 1) {
        hipLaunchKernelGGL(k_crit_sum, dim3(1, ny), dim3(256), 0, st, v, n, mode, gains, tss, out, (int64_t)1);
    } else {  // nb1 <= 4096 (kCritMaxSum)
        hipLaunchKernelGGL(k_crit_sum, dim3((unsigned)nb1, ny), dim3(256), 0, st, v, n, 0, gains, tss, part, nb1);
        hipLaunchKernelGGL(k_crit_sum, dim3(1, ny), dim3(256), 0, st, (const float *)part, nb1, mode, gains, tss, out, (int64_t)1);
    }
}

extern "C" int obb_crit_loss(obb_ctx *ctx, const void *const *box, int32_t box_bf16, const float *const *cls, const float *const *angle, const int32_t *H,
                             const int32_t *W, int32_t B, int32_t nc, const float *target_bboxes, const float *target_scores, const uint8_t *fg_mask,
                             const float *gains, void *const *d_box, float *const *d_cls, float *const *d_angle, float *items, float *tss,
                             obb_stream_t s) {
    CritLevels L;
    if (int rc = crit_levels(ctx, "obb_crit_loss", box, cls, angle, H, W, B, nc, L)) return rc;
    OBB_REQUIRE(ctx, target_bboxes && target_scores && fg_mask && gains && d_box && d_cls && d_angle && items && tss, "obb_crit_loss: NULL argument");
    for (int i = 0; i < kCritLevels; ++i) {
        OBB_REQUIRE(ctx, d_box[i] && d_cls[i] && d_angle[i], "obb_crit_loss: NULL gradient buffer at level %d", i);
        OBB_REQUIRE(ctx, ((uintptr_t)d_box[i] & 15) == 0, "obb_crit_loss: d_box of level %d must be 16-byte aligned", i);
        L.d_box[i] = d_box[i]; L.d_cls[i] = d_cls[i]; L.d_ang[i] = d_angle[i];
    }
    hipStream_t st = (hipStream_t)s;
    const int64_t n = (int64_t)B * L.A, nts = n * nc;
    float *elem = (float *)ctx->workspace(WS_GEOM_A, sizeof(float) * (size_t)(3 * n));
    float *part = (float *)ctx->workspace(WS_GEOM_B, sizeof(float) * (size_t)(3 * cdiv(nts, 4096) + 8));
    if (!elem || !part) return set_error(ctx, OBB_ERR_HIP, "obb_crit_loss: workspace allocation failed");
    CritGains g{{gains[0], gains[1], gains[2]}};
    crit_sum(target_scores, nts, 1, 1, g, nullptr, part, tss, st);  // (a) tss = max(sum target_scores, 1), on the device
    const unsigned nb = (unsigned)cdiv(n * 4, 256);                  // (b) every (image, anchor): reads tss through the pointer
    if (box_bf16) hipLaunchKernelGGL(k_crit_loss<unsigned short>, dim3(nb), dim3(256), 0, st, L, B, nc, target_bboxes, target_scores, fg_mask, (const float *)tss, g.g[0], g.g[1], g.g[2], elem);
    else hipLaunchKernelGGL(k_crit_loss<float>, dim3(nb), dim3(256), 0, st, L, B, nc, target_bboxes, target_scores, fg_mask, (const float *)tss, g.g[0], g.g[1], g.g[2], elem);
    crit_sum(elem, n, 3, 2, g, tss, part, items, st);               // items[k] = gain_k sum_k / tss
    OBB_LAUNCH_CHECK(ctx);
    return OBB_OK;
}
