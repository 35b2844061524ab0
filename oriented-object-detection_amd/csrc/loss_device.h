// Per-pair / per-side bodies of the OBB loss terms, shared by the stand-alone loss kernels (loss.hip), the fused criterion (criterion.hip) and
// the validation criterion (valreport.hip): the same fp32 operations in the same order in all, so they agree bit for bit on equal inputs.
#pragma once
#include <hip/hip_runtime.h>

namespace obb {

// ProbIoU of one (prediction, target) pair, forward and the closed-form gradient with respect to the prediction's (x, y, w, h, theta).
// -> (1 - iou) * wt; go[0..5) = wt * inv_tss * d (1 - iou) / d pred.  Clamps pass the gradient inside their range and block it outside.
__device__ __forceinline__ float probiou_pair(float x1, float y1, float w1, float h1, float t1a, float x2, float y2, float w2, float h2, float t2a,
                                              float wt, float inv_tss, float (&go)[5]) {
    const float eps = 1e-7f;
    // covariance terms (_get_covariance_matrix)
    const float a1 = w1 * w1 / 12.0f, b1 = h1 * h1 / 12.0f, c1 = cosf(t1a), s1 = sinf(t1a);
    const float a2 = w2 * w2 / 12.0f, b2 = h2 * h2 / 12.0f, c2 = cosf(t2a), s2 = sinf(t2a);
    const float A1 = a1 * c1 * c1 + b1 * s1 * s1, B1 = a1 * s1 * s1 + b1 * c1 * c1, C1 = (a1 - b1) * c1 * s1;
    const float A2 = a2 * c2 * c2 + b2 * s2 * s2, B2 = a2 * s2 * s2 + b2 * c2 * c2, C2 = (a2 - b2) * c2 * s2;
    const float A = A1 + A2, B = B1 + B2, C = C1 + C2;
    const float dx = x1 - x2, dy = y1 - y2;
    const float D = A * B - C * C, den = D + eps;
    const float N1 = A * dy * dy + B * dx * dx, N2 = C * dx * dy;
    const float T1 = 0.25f * N1 / den, T2 = -0.5f * N2 / den;
    const float d1raw = A1 * B1 - C1 * C1, d2raw = A2 * B2 - C2 * C2;
    const float d1 = fmaxf(d1raw, 0.0f), d2 = fmaxf(d2raw, 0.0f);
    const float r = sqrtf(d1 * d2), g = 4.0f * r + eps;
    const float u = D / g;
    const float T3 = 0.5f * logf(u + eps);
    const float braw = T1 + T2 + T3;
    const float bd = fminf(fmaxf(braw, eps), 100.0f);
    const float ex = expf(-bd);
    const float hd = sqrtf(1.0f - ex + eps);
    // ---- backward: dL/dbd, then the chain down to (x, y, w, h, theta) of the prediction
    float gb = (braw >= eps && braw <= 100.0f) ? wt * inv_tss * ex / (2.0f * hd) : 0.0f;
    const float iden = 1.0f / den, iden2 = iden * iden;
    // d(bd) / d(A, B, C, dx, dy)
    float gA = 0.25f * (dy * dy * iden - N1 * B * iden2) + 0.5f * N2 * B * iden2;
    float gB = 0.25f * (dx * dx * iden - N1 * A * iden2) + 0.5f * N2 * A * iden2;
    float gC = 0.5f * N1 * C * iden2 - 0.5f * dx * dy * iden - N2 * C * iden2;
    const float gdx = 0.5f * B * dx * iden - 0.5f * C * dy * iden;
    const float gdy = 0.5f * A * dy * iden - 0.5f * C * dx * iden;
    const float k3 = 0.5f / (u + eps);
    const float gD = k3 / g, gg = -k3 * D / (g * g);
    gA += gD * B; gB += gD * A; gC += gD * (-2.0f * C);
    // g = 4 sqrt(d1 d2) + eps: only det1 belongs to the prediction
    const float gdet1 = (d1raw >= 0.0f && r > 0.0f) ? gg * 2.0f * d2 / r : 0.0f;
    const float gA1 = gA + gdet1 * B1, gB1 = gB + gdet1 * A1, gC1 = gC + gdet1 * (-2.0f * C1);
    const float cs = c1 * s1;
    const float ga = gA1 * c1 * c1 + gB1 * s1 * s1 + gC1 * cs;
    const float gbb = gA1 * s1 * s1 + gB1 * c1 * c1 - gC1 * cs;
    const float gt = gA1 * (-2.0f * C1) + gB1 * (2.0f * C1) + gC1 * (a1 - b1) * (c1 * c1 - s1 * s1);
    go[0] = gb * gdx; go[1] = gb * gdy; go[2] = gb * ga * (w1 / 6.0f); go[3] = gb * gbb * (h1 / 6.0f); go[4] = gb * gt;
    return hd * wt;  // (1 - iou) * weight with iou = 1 - hd
}

// softmax pieces of one side's R logits: e_k = exp(x_k - m), se = sum_k e_k (k ascending)
template <int R>
__device__ __forceinline__ void softmax_parts(const float (&x)[R], float (&e)[R], float &m, float &se) {
    m = x[0];
#pragma unroll
    for (int k = 1; k < R; ++k) m = fmaxf(m, x[k]);
    se = 0.f;
#pragma unroll
    for (int k = 0; k < R; ++k) { e[k] = expf(x[k] - m); se += e[k]; }
}

// DFL of one (box, side) from its softmax pieces: the target distance clamped to [0, R - 1.01] shared out between its two neighbouring bins.
// -> loss element (times wt); g[k] = (softmax_k - (wl [k = tl] + wr [k = tr])) * gs
template <int R>
__device__ __forceinline__ float dfl_side(const float (&x)[R], const float (&e)[R], float m, float se, float target, float wt, float gs, float (&g)[R]) {
    const float lse = m + logf(se);
    const float t = fminf(fmaxf(target, 0.0f), (float)(R - 1) - 0.01f);
    const int tl = (int)t, tr = tl + 1;
    const float wl = (float)tr - t, wr = 1.0f - wl;
    float xl = 0.f, xr = 0.f;
#pragma unroll
    for (int k = 0; k < R; ++k) { xl = k == tl ? x[k] : xl; xr = k == tr ? x[k] : xr; }
    const float inv_se = 1.0f / se;
#pragma unroll
    for (int k = 0; k < R; ++k) g[k] = (e[k] * inv_se - (k == tl ? wl : 0.f) - (k == tr ? wr : 0.f)) * gs;
    return ((lse - xl) * wl + (lse - xr) * wr) * wt;
}

// BCEWithLogits of one element: l = max(x, 0) - x t + log(1 + exp(-|x|)); sig = sigmoid(x)
__device__ __forceinline__ float bce_elem(float x, float t, float &sig) {
    const float ea = expf(-fabsf(x));
    sig = x >= 0.0f ? 1.0f / (1.0f + ea) : ea / (1.0f + ea);
    return fmaxf(x, 0.0f) - x * t + log1pf(ea);
}

// ---- the head's decode, shared by the training criterion (criterion.hip: per-level tensors) and the validation criterion (valreport.hip: the
// engine's head rows): the same fp32 operations in the same order in both, so the two agree bit for bit on equal logits.
constexpr int kCritReg = 16;
constexpr float kCritPi = 3.14159265358979323846f;

// where an (image, anchor) lives: its level, its row in the level's [B*H*W] tensors, its anchor point and stride
struct CritAnchor {
    int lv;
    int64_t row;
    float ax, ay, s;
};
__device__ __forceinline__ CritAnchor crit_anchor(int a0, int a1, int H0, int H1, int H2, int W0, int W1, int W2, int b, int j) {
    CritAnchor r;
    r.lv = j < a0 ? 0 : (j < a1 ? 1 : 2);
    const int jj = j - (r.lv == 0 ? 0 : (r.lv == 1 ? a0 : a1));
    const int H = r.lv == 0 ? H0 : (r.lv == 1 ? H1 : H2);
    const int W = r.lv == 0 ? W0 : (r.lv == 1 ? W1 : W2);
    const int y = jj / W, x = jj - y * W;
    r.row = (int64_t)b * H * W + jj;
    r.ax = (float)x + 0.5f; r.ay = (float)y + 0.5f;
    r.s = r.lv == 0 ? 8.0f : (r.lv == 1 ? 16.0f : 32.0f);
    return r;
}

// the decode of one anchor, as every lane of its quad holds it after the exchange
struct CritBox {
    float l, t, r, b, sig, th, c, s, xf, yf, x, y, w, h;
};
// x: this lane's side logits -> softmax pieces (e, m, se, left for the DFL term), p = e / se, E = sum_k k p_k; the quad's four E by __shfl
__device__ __forceinline__ CritBox crit_decode_quad(const float (&x)[kCritReg], float (&e)[kCritReg], float &m, float &se, float &E, float a,
                                                    float ax, float ay) {
    softmax_parts<kCritReg>(x, e, m, se);
    const float inv_se = 1.0f / se;
    E = 0.f;
#pragma unroll
    for (int k = 0; k < kCritReg; ++k) E += (float)k * (e[k] * inv_se);
    CritBox d;
    d.l = __shfl(E, 0, 4); d.t = __shfl(E, 1, 4); d.r = __shfl(E, 2, 4); d.b = __shfl(E, 3, 4);
    const float ea = expf(-fabsf(a));
    d.sig = a >= 0.0f ? 1.0f / (1.0f + ea) : ea / (1.0f + ea);
    d.th = (d.sig - 0.25f) * kCritPi;
    d.c = cosf(d.th); d.s = sinf(d.th);
    d.xf = (d.r - d.l) * 0.5f; d.yf = (d.b - d.t) * 0.5f;
    d.x = ax + (d.xf * d.c - d.yf * d.s);
    d.y = ay + (d.xf * d.s + d.yf * d.c);
    d.w = d.l + d.r; d.h = d.t + d.b;
    return d;
}

}  // namespace obb
