// f1 (training batches): what the Ultralytics dataloader does between the tiles on disk and `model.train(...)`'s batch (Train_OBB.py:796-841 leaves
// every augmentation argument at its default: 4-image Mosaic p = 1, RandomPerspective(translate 0.1, scale 0.5, degrees 0), RandomHSV(0.015, 0.7,
// 0.4), fliplr 0.5; Ultralytics 8.3.x and cv2 restated from recall: neither is installed, parity UNPINNED -- pinned is the device against this
// repository's numpy / fp64 restatement, tests/aug_ref.py).  Two kernels over one per-tile parameter table (AugRec, include/obbhip.h):
//   k_aug_tiles   one fused gather: output pixel -> (flip) -> inverse affine map in warpAffine's fixed point -> four taps of a VIRTUAL mosaic canvas
//                 (never materialised: every lane finds its taps' quadrant and source address itself) -> bilinear in integers -> HSV gains (cv2's
//                 8-bit integer BGR->HSV, three LUTs, a fixed fp32 HSV->BGR sequence) -> store.  No atomics; every output byte has one writer.
//   k_aug_labels  one workgroup per output tile, one thread per (source, label) candidate: corners -> canvas -> M -> flips -> box_candidates ->
//                 hull, clip to the tile, minimum-area rectangle -> (x, y, w, h, theta) -> workgroup prefix sum -> padded targets.  fp64 throughout.
// Both only enqueue on the caller's stream (no host read, no allocation): capturable.
#include "ctx.h"

using namespace obb;

namespace {

struct AugRec {
    double inv[6];   // dst -> canvas (the host inverts M in double)
    double fwd[6];   // canvas -> dst, M = T R C
    double scale;    // the R factor of M: box_candidates scales the boxes before by it
    int32_t xc, yc;  // mosaic centre
    int32_t src[4];  // pool tiles of the four quadrants (top-left, top-right, bottom-left, bottom-right); src[0] alone without mosaic
    uint32_t flags;  // OBB_AUG_MOSAIC | OBB_AUG_FLIPLR | OBB_AUG_FLIPUD | OBB_AUG_HSV
    int32_t reserved;
    uint8_t lut[768];  // lut_h | lut_s | lut_v
};
static_assert(sizeof(AugRec) == OBB_AUG_REC_BYTES, "AugRec is the record of include/obbhip.h");

constexpr int kStripRows = 8;  // output rows per workgroup of k_aug_tiles
constexpr int kBorder = 114;
// A later edge replaces the running minimum-area rectangle only when it is smaller by more than this (relative).  Every edge of a triangle gives the
// same area, so exact ties are common; without the slack, rounding would pick the edge.
constexpr double kTie = 1e-7;

// A record a workgroup can act on without leaving the pool: the table lives on the device, so the entry points cannot look at it.
__device__ __forceinline__ bool rec_ok(const AugRec &r, int N, int s) {
    const bool mosaic = r.flags & OBB_AUG_MOSAIC;
    bool ok = (unsigned)r.src[0] < (unsigned)N;
    if (mosaic) {
        for (int q = 1; q < 4; ++q) ok = ok && (unsigned)r.src[q] < (unsigned)N;
        ok = ok && r.xc >= 0 && r.xc <= 2 * s && r.yc >= 0 && r.yc <= 2 * s;
    }
    return ok;
}

// saturate_cast<int>(double) of warpAffine's tables, limited to +-2^29 so that the sum of two and the rounding term stays inside int32
__device__ __forceinline__ int fix_round(double v) {
    v = fmin(fmax(v, -536870912.0), 536870912.0);
    return __double2int_rn(v);
}

__device__ __forceinline__ int sat_u8(float v) {
    const float r = rintf(v);
    return (int)fminf(fmaxf(r, 0.f), 255.f);
}

// cv2's 8-bit BGR -> HSV (H in 0..179): sdiv / hdiv are its shift-12 tables written out.  rint((255 << 12) / i) and rint((180 << 12) / (6 i)) have no
// ties for 1 <= i <= 255 (a tie needs 2^13 | i), so the round-half-up integer quotients below are the tables exactly.
__device__ __forceinline__ void bgr2hsv_u8(int b, int g, int r, int &h, int &s, int &v) {
    v = max(b, max(g, r));
    const int vmin = min(b, min(g, r)), diff = v - vmin;
    const int sdiv = v ? (2088960 + v) / (2 * v) : 0, hdiv = diff ? (245760 + diff) / (2 * diff) : 0;
    s = (diff * sdiv + 2048) >> 12;
    int hh = v == r ? g - b : (v == g ? b - r + 2 * diff : r - g + 4 * diff);
    hh = (hh * hdiv + 2048) >> 12;  // arithmetic shift: floor, as the int code it restates
    h = hh < 0 ? hh + 180 : hh;
}

// cv2's 8-bit HSV -> BGR: the float algorithm on (h, s / 255, v / 255), every product and sum rounded to fp32 on its own (no contraction)
__device__ __forceinline__ void hsv2bgr_u8(int h, int s, int v, int &b, int &g, int &r) {
    const float hf = __fmul_rn((float)h, 6.f / 180.f), sf = __fmul_rn((float)s, 1.f / 255.f), vf = __fmul_rn((float)v, 1.f / 255.f);
    int sector = (int)floorf(hf);
    float f = __fadd_rn(hf, -(float)sector);
    if ((unsigned)sector >= 6u) { sector = 0; f = 0.f; }
    const float t0 = vf, t1 = __fmul_rn(vf, __fadd_rn(1.f, -sf)), t2 = __fmul_rn(vf, __fadd_rn(1.f, -__fmul_rn(sf, f))),
                t3 = __fmul_rn(vf, __fadd_rn(1.f, -__fmul_rn(sf, __fadd_rn(1.f, -f))));
    float fb, fg, fr;
    switch (sector) {
        case 0: fb = t1; fg = t3; fr = t0; break;
        case 1: fb = t1; fg = t0; fr = t2; break;
        case 2: fb = t3; fg = t0; fr = t1; break;
        case 3: fb = t0; fg = t2; fr = t1; break;
        case 4: fb = t0; fg = t1; fr = t3; break;
        default: fb = t2; fg = t1; fr = t0; break;
    }
    b = sat_u8(__fmul_rn(fb, 255.f)); g = sat_u8(__fmul_rn(fg, 255.f)); r = sat_u8(__fmul_rn(fr, 255.f));
}

// grid (ceil(s / kStripRows), B): one workgroup = a strip of output rows of one tile
template <int C>
__global__ __launch_bounds__(256) void k_aug_tiles(const uint8_t *__restrict__ pool, int N, int s, const AugRec *__restrict__ table, int bgr, int swap_rb,
                                                   uint8_t *__restrict__ out) {
    const AugRec &r = table[blockIdx.y];
    if (!rec_ok(r, N, s)) return;  // (uniform over the workgroup)
    __shared__ uint32_t lut32[192];
    const uint32_t flags = r.flags;
    if (flags & OBB_AUG_HSV)
        for (int i = threadIdx.x; i < 192; i += 256) lut32[i] = reinterpret_cast<const uint32_t *>(r.lut)[i];
    __syncthreads();
    const uint8_t *lut = reinterpret_cast<const uint8_t *>(lut32);
    const bool mosaic = flags & OBB_AUG_MOSAIC;
    const int S = mosaic ? 2 * s : s, xc = r.xc, yc = r.yc;
    const int s0 = r.src[0], s1 = mosaic ? r.src[1] : 0, s2 = mosaic ? r.src[2] : 0, s3 = mosaic ? r.src[3] : 0;
    const double m00 = r.inv[0], m01 = r.inv[1], m02 = r.inv[2], m10 = r.inv[3], m11 = r.inv[4], m12 = r.inv[5];
    const int y0 = blockIdx.x * kStripRows, rows = min(kStripRows, s - y0);

    // pixel index of canvas(u, v) in the pool, or -1 where the canvas holds the border value
    auto tap = [&](int u, int v) -> int64_t {
        if ((unsigned)u >= (unsigned)S || (unsigned)v >= (unsigned)S) return -1;
        int t = s0, sx = u, sy = v;
        if (mosaic) {
            const bool qx = u >= xc, qy = v >= yc;
            sx = u - (qx ? xc : xc - s);
            sy = v - (qy ? yc : yc - s);
            if ((unsigned)sx >= (unsigned)s || (unsigned)sy >= (unsigned)s) return -1;
            t = qy ? (qx ? s3 : s2) : (qx ? s1 : s0);
        }
        return ((int64_t)t * s + sy) * s + sx;
    };

    for (int i = threadIdx.x; i < rows * s; i += 256) {
        const int yo = y0 + i / s, xo = i % s;
        const int x = (flags & OBB_AUG_FLIPLR) ? s - 1 - xo : xo, y = (flags & OBB_AUG_FLIPUD) ? s - 1 - yo : yo;
        const int X = (fix_round(__dmul_rn(__dmul_rn(m00, (double)x), 1024.0)) + fix_round(__dmul_rn(__dadd_rn(__dmul_rn(m01, (double)y), m02), 1024.0)) + 16) >> 5;
        const int Y = (fix_round(__dmul_rn(__dmul_rn(m10, (double)x), 1024.0)) + fix_round(__dmul_rn(__dadd_rn(__dmul_rn(m11, (double)y), m12), 1024.0)) + 16) >> 5;
        const int ix = X >> 5, iy = Y >> 5, fx = X & 31, fy = Y & 31;
        const int w00 = 32 * (32 - fx) * (32 - fy), w01 = 32 * fx * (32 - fy), w10 = 32 * (32 - fx) * fy, w11 = 32 * fx * fy;
        const int64_t a00 = tap(ix, iy), a01 = tap(ix + 1, iy), a10 = tap(ix, iy + 1), a11 = tap(ix + 1, iy + 1);
        int c[4];
        if (C == 4) {
            const uint32_t *p32 = reinterpret_cast<const uint32_t *>(pool);
            const uint32_t kB = 0x01010101u * kBorder;
            const uint32_t v00 = a00 >= 0 ? p32[a00] : kB, v01 = a01 >= 0 ? p32[a01] : kB, v10 = a10 >= 0 ? p32[a10] : kB, v11 = a11 >= 0 ? p32[a11] : kB;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                c[k] = (int)(w00 * ((v00 >> (8 * k)) & 255) + w01 * ((v01 >> (8 * k)) & 255) + w10 * ((v10 >> (8 * k)) & 255) + w11 * ((v11 >> (8 * k)) & 255) + 16384) >> 15;
        } else {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int v00 = a00 >= 0 ? pool[a00 * 3 + k] : kBorder, v01 = a01 >= 0 ? pool[a01 * 3 + k] : kBorder;
                const int v10 = a10 >= 0 ? pool[a10 * 3 + k] : kBorder, v11 = a11 >= 0 ? pool[a11 * 3 + k] : kBorder;
                c[k] = (w00 * v00 + w01 * v01 + w10 * v10 + w11 * v11 + 16384) >> 15;
            }
            c[3] = 0;
        }
        if (flags & OBB_AUG_HSV) {
            int h, sa, va, b, g, rr;
            bgr2hsv_u8(bgr ? c[0] : c[2], c[1], bgr ? c[2] : c[0], h, sa, va);
            hsv2bgr_u8(lut[h], lut[256 + sa], lut[512 + va], b, g, rr);
            c[0] = bgr ? b : rr; c[1] = g; c[2] = bgr ? rr : b;
        }
        if (swap_rb) { const int t = c[0]; c[0] = c[2]; c[2] = t; }
        const int64_t o = ((int64_t)blockIdx.y * s + yo) * s + xo;
        if (C == 4) {
            reinterpret_cast<uint32_t *>(out)[o] = (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16) | ((uint32_t)c[3] << 24);
        } else {
            out[o * 3] = (uint8_t)c[0]; out[o * 3 + 1] = (uint8_t)c[1]; out[o * 3 + 2] = (uint8_t)c[2];
        }
    }
}

// ---------------------------------------------------------------- labels
struct P2 { double x, y; };
__device__ __forceinline__ double cross3(P2 o, P2 a, P2 b) { return (a.x - o.x) * (b.y - o.y) - (a.y - o.y) * (b.x - o.x); }
__device__ __forceinline__ bool lex_less(P2 a, P2 b) { return a.x < b.x || (a.x == b.x && a.y < b.y); }
__device__ __forceinline__ void cswap(P2 &a, P2 &b) { if (lex_less(b, a)) { const P2 t = a; a = b; b = t; } }

// Sutherland-Hodgman against one side of [0, s]^2: axis 0 = x, 1 = y; keep coordinate >= bound (lower) or <= bound (upper).  A crossing point gets
// the bound itself as its clipped coordinate.
__device__ int clip_side(const P2 *in, int n, P2 *out, int axis, double bound, bool lower) {
    int m = 0;
    for (int i = 0; i < n; ++i) {
        const P2 a = in[i], b = in[i + 1 == n ? 0 : i + 1];
        const double ca = axis ? a.y : a.x, cb = axis ? b.y : b.x;
        const bool ia = lower ? ca >= bound : ca <= bound, ib = lower ? cb >= bound : cb <= bound;
        if (ia && m < 8) out[m++] = a;
        if (ia != ib && m < 8) {
            const double t = (bound - ca) / (cb - ca);
            P2 p;
            if (axis) { p.x = a.x + t * (b.x - a.x); p.y = bound; } else { p.x = bound; p.y = a.y + t * (b.y - a.y); }
            out[m++] = p;
        }
    }
    return m;
}

// one candidate: row = class + 8 corner coordinates normalised to its pool tile; -> keep, class, (x, y, w, h, theta)
__device__ bool aug_candidate(const AugRec &r, int q, const double *__restrict__ row, int s, double wh_thr, double ar_thr, double area_thr, int &cls, float *box) {
    const bool mosaic = r.flags & OBB_AUG_MOSAIC;
    const double sd = (double)s, Sd = mosaic ? 2.0 * sd : sd;
    double padx = 0.0, pady = 0.0;
    if (mosaic) { padx = (double)((q & 1) ? r.xc : r.xc - s); pady = (double)((q & 2) ? r.yc : r.yc - s); }
    P2 p[4];
    double bx0 = 1e300, by0 = 1e300, bx1 = -1e300, by1 = -1e300, ax0 = 1e300, ay0 = 1e300, ax1 = -1e300, ay1 = -1e300;
    for (int k = 0; k < 4; ++k) {
        const double x = fmin(fmax(row[1 + 2 * k] * sd + padx, 0.0), Sd), y = fmin(fmax(row[2 + 2 * k] * sd + pady, 0.0), Sd);
        bx0 = fmin(bx0, x); bx1 = fmax(bx1, x); by0 = fmin(by0, y); by1 = fmax(by1, y);
        double tx = (r.fwd[0] * x + r.fwd[1] * y) + r.fwd[2], ty = (r.fwd[3] * x + r.fwd[4] * y) + r.fwd[5];
        if (r.flags & OBB_AUG_FLIPLR) tx = sd - tx;
        if (r.flags & OBB_AUG_FLIPUD) ty = sd - ty;
        p[k].x = tx; p[k].y = ty;
        ax0 = fmin(ax0, tx); ax1 = fmax(ax1, tx); ay0 = fmin(ay0, ty); ay1 = fmax(ay1, ty);
    }
    // box_candidates: the box before (times the scale) against the box after, clipped to the tile as the transformed points are
    const double w1 = (bx1 - bx0) * r.scale, h1 = (by1 - by0) * r.scale;
    const double w2 = fmin(fmax(ax1, 0.0), sd) - fmin(fmax(ax0, 0.0), sd), h2 = fmin(fmax(ay1, 0.0), sd) - fmin(fmax(ay0, 0.0), sd);
    const double ar = fmax(w2 / (h2 + 1e-16), h2 / (w2 + 1e-16));
    if (!(w2 > wh_thr && h2 > wh_thr && w2 * h2 / (w1 * h1 + 1e-16) > area_thr && ar < ar_thr)) return false;
    // convex hull of the four points (monotone chain; counter-clockwise in (x, y), collinear points dropped, starts at the lexicographic minimum)
    cswap(p[0], p[1]); cswap(p[2], p[3]); cswap(p[0], p[2]); cswap(p[1], p[3]); cswap(p[1], p[2]);
    P2 va[8], vb[8];
    int n = 0;
    for (int i = 0; i < 4; ++i) {
        while (n >= 2 && cross3(va[n - 2], va[n - 1], p[i]) <= 0.0) --n;
        va[n++] = p[i];
    }
    for (int i = 2, t = n + 1; i >= 0; --i) {
        while (n >= t && cross3(va[n - 2], va[n - 1], p[i]) <= 0.0) --n;
        va[n++] = p[i];
    }
    --n;
    if (n < 3) return false;
    n = clip_side(va, n, vb, 0, 0.0, true);
    n = clip_side(vb, n, va, 0, sd, false);
    n = clip_side(va, n, vb, 1, 0.0, true);
    n = clip_side(vb, n, va, 1, sd, false);
    if (n < 3) return false;
    // minimum-area enclosing rectangle over the edge directions; the first edge wins a tie (kTie)
    double best = 1e300, bux = 1.0, buy = 0.0, bu0 = 0, bu1 = 0, bn0 = 0, bn1 = 0;
    for (int i = 0; i < n; ++i) {
        const P2 a = va[i], b = va[i + 1 == n ? 0 : i + 1];
        const double dx = b.x - a.x, dy = b.y - a.y, l2 = dx * dx + dy * dy;
        if (l2 < 1e-12) continue;
        const double il = 1.0 / sqrt(l2), ux = dx * il, uy = dy * il;
        double u0 = 1e300, u1 = -1e300, n0 = 1e300, n1 = -1e300;
        for (int j = 0; j < n; ++j) {
            const double pu = va[j].x * ux + va[j].y * uy, pn = va[j].y * ux - va[j].x * uy;
            u0 = fmin(u0, pu); u1 = fmax(u1, pu); n0 = fmin(n0, pn); n1 = fmax(n1, pn);
        }
        const double area = (u1 - u0) * (n1 - n0);
        if (area < best * (1.0 - kTie)) { best = area; bux = ux; buy = uy; bu0 = u0; bu1 = u1; bn0 = n0; bn1 = n1; }
    }
    if (best == 1e300) return false;
    const double cu = 0.5 * (bu0 + bu1), cn = 0.5 * (bn0 + bn1);
    const double cx = cu * bux - cn * buy, cy = cu * buy + cn * bux;
    double w = bu1 - bu0, h = bn1 - bn0, c, sn;
    // theta in [0, pi / 2) with w along (cos theta, sin theta): turn u by quarter turns into the first quadrant; an odd count swaps the extents
    if (bux > 0.0 && buy >= 0.0) { c = bux; sn = buy; }
    else if (bux <= 0.0 && buy > 0.0) { c = buy; sn = -bux; const double t = w; w = h; h = t; }
    else if (bux < 0.0 && buy <= 0.0) { c = -bux; sn = -buy; }
    else { c = -buy; sn = bux; const double t = w; w = h; h = t; }
    if (w < 2.0 || h < 2.0) return false;  // pad_targets' rule
    cls = (int)row[0];
    box[0] = (float)cx; box[1] = (float)cy; box[2] = (float)w; box[3] = (float)h; box[4] = (float)atan2(sn, c);
    return true;
}

// grid B: one workgroup per output tile; candidates in (q, l) order, 256 per pass, compacted by a workgroup prefix sum
__global__ __launch_bounds__(256) void k_aug_labels(const double *__restrict__ pool_labels, const int32_t *__restrict__ pool_counts, int N, int Lmax,
                                                    const AugRec *__restrict__ table, int s, double wh_thr, double ar_thr, double area_thr, int n_cap,
                                                    int32_t *__restrict__ gt_labels, float *__restrict__ gt_bboxes, uint8_t *__restrict__ mask_gt,
                                                    int32_t *__restrict__ count) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const AugRec &r = table[b];
    if (!rec_ok(r, N, s)) return;
    __shared__ int sc[256];
    const int64_t total = (int64_t)((r.flags & OBB_AUG_MOSAIC) ? 4 : 1) * Lmax;
    int32_t *gl = gt_labels + (int64_t)b * n_cap;
    float *gb = gt_bboxes + (int64_t)b * n_cap * 5;
    uint8_t *mk = mask_gt + (int64_t)b * n_cap;
    int base = 0;
    for (int64_t c0 = 0; c0 < total; c0 += 256) {
        const int64_t c = c0 + tid;
        bool keep = false;
        int cls = 0;
        float box[5];
        if (c < total) {
            const int q = (int)(c / Lmax), l = (int)(c % Lmax), t = r.src[q];
            const int cnt = min(max(pool_counts[t], 0), Lmax);
            if (l < cnt) keep = aug_candidate(r, q, pool_labels + ((int64_t)t * Lmax + l) * 9, s, wh_thr, ar_thr, area_thr, cls, box);
        }
        sc[tid] = keep ? 1 : 0;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {
            const int v = tid >= off ? sc[tid - off] : 0;
            __syncthreads();
            sc[tid] += v;
            __syncthreads();
        }
        const int pos = base + sc[tid] - (keep ? 1 : 0);
        if (keep && pos < n_cap) {
            gl[pos] = cls; mk[pos] = 1;
            for (int k = 0; k < 5; ++k) gb[(int64_t)pos * 5 + k] = box[k];
        }
        base += sc[255];
        __syncthreads();
    }
    for (int j = min(base, n_cap) + tid; j < n_cap; j += 256) {
        gl[j] = 0; mk[j] = 0;
        for (int k = 0; k < 5; ++k) gb[(int64_t)j * 5 + k] = 0.f;
    }
    if (tid == 0) count[b] = base;
}

}  // namespace

extern "C" {

int obb_aug_tiles(obb_ctx *ctx, const uint8_t *pool, int32_t N, int32_t s, int32_t C, const void *table, int32_t B, int32_t bgr, int32_t swap_rb,
                  uint8_t *out, obb_stream_t st) {
    OBB_REQUIRE(ctx, ctx && N >= 1 && B >= 0, "obb_aug_tiles: bad arguments");
    OBB_REQUIRE(ctx, s >= 2 && s <= 16384, "obb_aug_tiles: tile side %d outside [2, 16384]", s);
    OBB_REQUIRE(ctx, C == 3 || C == 4, "obb_aug_tiles: %d channels (3 or 4)", C);
    if (B == 0) return OBB_OK;
    OBB_REQUIRE(ctx, pool && table && out, "obb_aug_tiles: NULL buffer");
    OBB_REQUIRE(ctx, B <= 65535, "obb_aug_tiles: more than 65535 tiles in one call");
    OBB_REQUIRE(ctx, ((uintptr_t)table & 7) == 0, "obb_aug_tiles: the parameter table must be 8-byte aligned");
    OBB_REQUIRE(ctx, C == 3 || ((((uintptr_t)pool | (uintptr_t)out) & 3) == 0), "obb_aug_tiles: 4-channel tiles must be 4-byte aligned");
    const dim3 grid((unsigned)cdiv(s, kStripRows), (unsigned)B);
    const AugRec *tb = (const AugRec *)table;
    if (C == 4)
        hipLaunchKernelGGL(k_aug_tiles<4>, grid, dim3(256), 0, (hipStream_t)st, pool, (int)N, (int)s, tb, (int)(bgr != 0), (int)(swap_rb != 0), out);
    else
        hipLaunchKernelGGL(k_aug_tiles<3>, grid, dim3(256), 0, (hipStream_t)st, pool, (int)N, (int)s, tb, (int)(bgr != 0), (int)(swap_rb != 0), out);
    OBB_LAUNCH_CHECK(ctx);
    return OBB_OK;
}

int obb_aug_labels(obb_ctx *ctx, const double *pool_labels, const int32_t *pool_counts, int32_t N, int32_t Lmax, const void *table, int32_t B, int32_t s,
                   double wh_thr, double ar_thr, double area_thr, int32_t n_cap, int32_t *gt_labels, float *gt_bboxes, uint8_t *mask_gt, int32_t *count,
                   obb_stream_t st) {
    OBB_REQUIRE(ctx, ctx && N >= 1 && B >= 0 && Lmax >= 0 && n_cap >= 1, "obb_aug_labels: bad arguments");
    OBB_REQUIRE(ctx, s >= 2 && s <= 16384, "obb_aug_labels: tile side %d outside [2, 16384]", s);
    if (B == 0) return OBB_OK;
    OBB_REQUIRE(ctx, (pool_labels || Lmax == 0) && pool_counts && table && gt_labels && gt_bboxes && mask_gt && count, "obb_aug_labels: NULL buffer");
    OBB_REQUIRE(ctx, ((uintptr_t)table & 7) == 0, "obb_aug_labels: the parameter table must be 8-byte aligned");
    hipLaunchKernelGGL(k_aug_labels, dim3((unsigned)B), dim3(256), 0, (hipStream_t)st, pool_labels, pool_counts, (int)N, (int)Lmax, (const AugRec *)table, (int)s,
                       wh_thr, ar_thr, area_thr, (int)n_cap, gt_labels, gt_bboxes, mask_gt, count);
    OBB_LAUNCH_CHECK(ctx);
    return OBB_OK;
}

}  // extern "C"
