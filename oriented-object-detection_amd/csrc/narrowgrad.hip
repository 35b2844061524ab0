// Training-mode kernels of the conv layers whose channel counts are no multiples of 8 (`model.train(...)`,
// Train_OBB.py:796-841): the plain `Conv2d` 1x1 + bias outputs of the head (model.23.cv3.i.2: c -> nc class logits, model.23.cv4.i.2: c -> 1 angle
// logit) and the stem (model.0: Conv 3x3 s2 on the 3- or 4-channel uint8 tile).  Conventions of dwgrad.hip: the fp32 master weights are read
// directly and rounded to bf16 (traindev.h's bf16_round) as they are loaded -- no pack step --, products and sums are fp32 (a bf16 x bf16 product is exact in
// fp32, so fmaf is the product followed by the addition), no atomics.  Every padded channel lives in registers or LDS, never in global memory.
//
// HEAD, pixels flattened, N = B H W, x bf16 [N][cin] (cin % 8 == 0, <= 512), y / dy fp32 [N][cout] dense (1 <= cout <= 64; rows of 4 cout bytes: scalar
// dword accesses, no row alignment assumed), dy rounded to bf16 at load (dy~):
//   forward   y[n,o]  = (sum_c w~[o,c] x[n,c]) + bias[o]       c ascending from 0, the bias last.  One lane per pixel; 16 (4 for cout <= 4) outputs
//                                                              at a time, their weights rounded once per workgroup into LDS (broadcast reads)
//   backward  dx[n,c] = sum_o w~[o,c] dy~[n,o]                 o ascending from 0, one bf16 rounding
//             dw[o,c] = sum_n dy~[n,o] x[n,c];  db[o] = sum_n dy~[n,o]
// Backward split (head_geo, the ONE place that decides it; obb_headconv_bwd_geometry returns it): a lane owns CPL input channels (2; 1 when cout >
// 16) and OT outputs (4 / 16 / 64 >= cout, the padding in registers): its OT x CPL weights and dw sums stay in registers while it walks pixels
// bx RP + row + t nbx RP, t < iters -- x, dy are read and dx is written once, dx / dw / db from the same pass.  A workgroup is CW channel lanes x
// RP pixel rows; the dy rows of a pass are rounded once into LDS by the whole workgroup.  The RP lanes of a channel meet in LDS in traindev.h's
// lds_row_tree, 8 outputs per pass; workgroup bx writes its partial to the fp32 slab [bx][cout cin + cout] (WS_TRAIN_E, never read before it is
// written: growing the slot changes nothing); k_narrow_final adds the slabs in slab_combine's order.  L = iters + ceil(log2 RP) + slab_chain(nbx).
//
// STEM, x uint8 [B][H][W][cin] (cin 3 or 4), operand x~ = bf16(v / 255) from a 256-entry LDS table (an fp32 division, then nearest even: the value
// the inference stem uses in its bf16 mode), w fp32 [cout][cin][3][3] (cout % 8 == 0, <= 64), z / dz bf16 [B][Ho][Wo][cout], Ho = (H + 1) / 2:
//   forward   z[b,i,j,o]    = sum_{ky,kx,c} w~[o,c,ky,kx] x~[b, 2i+ky-1, 2j+kx-1, c]     (ky, kx, c) ascending from 0, taps outside the map skipped
//   wgrad     dw[o,c,ky,kx] = sum_{b,i,j} dz[b,i,j,o] x~[b, 2i+ky-1, 2j+kx-1, c]
// Forward: a lane owns one output pixel and 8 (16 when cout % 16 == 0) outputs, the rounded weights in LDS as [tap][c][cout].  Wgrad split
// (stem_geo; obb_stemconv_wgrad_geometry): a lane owns 4 outputs and all 9 cin taps (36 cin sums in registers), CW = cout / 4 lanes per output pixel,
// RP = 256 / CW pixel rows, pixels bx RP + row + t nbx RP; the same LDS tree (one tap per pass), slab [bx][9][cin][cout] and final launch.  Same L.
#include <algorithm>

#include "ctx.h"
#include "traindev.h"

namespace obb {
namespace {

constexpr int kNrMaxSlabs = 512;   // workgroups (= slabs) per column group at most: beyond, a lane's run grows
constexpr int kNrMinRun = 8;       // pixels per lane run before a second workgroup is opened: amortises the lane's weight loads and the slab
constexpr int kHeadFwdThreads = 128;
constexpr int kHeadMaxCin = 512, kHeadMaxCout = 64, kStemMaxCout = 64;

struct HeadGeo { int OT, CPL, CW, RP, ny, nbx, L; int64_t iters; };
HeadGeo head_geo(int64_t N, int cin, int cout) {
    HeadGeo g;
    g.OT = cout <= 4 ? 4 : cout <= 16 ? 16 : 64;
    g.CPL = g.OT == 64 ? 1 : 2;
    const int CL = cin / g.CPL;  // channel lanes
    g.CW = std::min(CL, 256);
    g.ny = (CL + g.CW - 1) / g.CW;
    g.RP = 256 / g.CW;
    g.nbx = (int)std::min<int64_t>(cdiv(N, (int64_t)g.RP * kNrMinRun), kNrMaxSlabs);
    g.iters = cdiv(N, (int64_t)g.nbx * g.RP);
    g.L = (int)std::min<int64_t>(g.iters + tree_depth(g.RP) + slab_chain(g.nbx), INT32_MAX);
    return g;
}

struct StemGeo { int Ho, Wo, CW, RP, nbx, L; int64_t NP, iters; };
StemGeo stem_geo(int B, int H, int W, int cout) {
    StemGeo g;
    g.Ho = (H + 1) / 2;
    g.Wo = (W + 1) / 2;
    g.NP = (int64_t)B * g.Ho * g.Wo;
    g.CW = cout / 4;
    g.RP = 256 / g.CW;
    g.nbx = (int)std::min<int64_t>(cdiv(g.NP, (int64_t)g.RP * kNrMinRun), kNrMaxSlabs);
    g.iters = cdiv(g.NP, (int64_t)g.nbx * g.RP);
    g.L = (int)std::min<int64_t>(g.iters + tree_depth(g.RP) + slab_chain(g.nbx), INT32_MAX);
    return g;
}

}  // namespace

// ---------------------------------------------------------------------------------------------- head forward
template <int OT>
__global__ __launch_bounds__(kHeadFwdThreads) void k_headconv_fwd(const unsigned short *__restrict__ x, const float *__restrict__ w, const float *__restrict__ bias, int64_t N,
                                                                 int cin, int cout, float *__restrict__ y) {
    __shared__ __attribute__((aligned(16))) float wl[OT * kHeadMaxCin];  // [o][cin], rounded; rows past cout are zero
    const int64_t n = (int64_t)blockIdx.x * kHeadFwdThreads + threadIdx.x;
    for (int o0 = 0; o0 < cout; o0 += OT) {
        if (o0) __syncthreads();
        for (int e = threadIdx.x; e < OT * cin; e += kHeadFwdThreads) {
            const int o = o0 + e / cin;
            wl[e] = o < cout ? bf16_round(w[(size_t)o * cin + e % cin]) : 0.f;
        }
        __syncthreads();
        if (n < N) {
            float acc[OT];
#pragma unroll
            for (int o = 0; o < OT; ++o) acc[o] = 0.f;
            const uint4 *xr = reinterpret_cast<const uint4 *>(x + (size_t)n * cin);
            for (int c8 = 0; c8 < cin / 8; ++c8) {
                float f[8];
                unpack8_bf16(xr[c8], f);
#pragma unroll
                for (int o = 0; o < OT; ++o) {
                    const float4 *wr = reinterpret_cast<const float4 *>(wl + o * cin + c8 * 8);
                    const float4 w0 = wr[0], w1 = wr[1];
                    acc[o] = fmaf(w0.x, f[0], acc[o]); acc[o] = fmaf(w0.y, f[1], acc[o]); acc[o] = fmaf(w0.z, f[2], acc[o]); acc[o] = fmaf(w0.w, f[3], acc[o]);
                    acc[o] = fmaf(w1.x, f[4], acc[o]); acc[o] = fmaf(w1.y, f[5], acc[o]); acc[o] = fmaf(w1.z, f[6], acc[o]); acc[o] = fmaf(w1.w, f[7], acc[o]);
                }
            }
            float *yr = y + (size_t)n * cout + o0;
#pragma unroll
            for (int o = 0; o < OT; ++o)
                if (o0 + o < cout) yr[o] = bias ? acc[o] + bias[o0 + o] : acc[o];
        }
    }
}

// ---------------------------------------------------------------------------------------------- the slab combine (head and stem)
// out element q = sum over the slabs of slab[k][q] in slab_combine's order.  STEM: q = (tap cin + c) cout + o -> dw[o][c][tap];
// head: q < cout cin -> dw[q], else db[q - cout cin] (a NULL output is skipped)
template <bool STEM>
__global__ __launch_bounds__(256) void k_narrow_final(const float *__restrict__ slab, int nbx, int cin, int cout, float *__restrict__ dw, float *__restrict__ db) {
    const int q = slab_elem();
    float a[1];
    if (!slab_combine<1>({slab}, nbx, STEM ? 9 * cin * cout : cout * cin + cout, q, a)) return;
    if (STEM) {
        const int o = q % cout, tc = q / cout, c = tc % cin, tap = tc / cin;
        dw[((size_t)o * cin + c) * 9 + tap] = a[0];
    } else if (q < cout * cin) {
        if (dw) dw[q] = a[0];
    } else if (db) {
        db[q - cout * cin] = a[0];
    }
}

// ---------------------------------------------------------------------------------------------- head backward
// grid (nbx, ny), workgroup = CW channel lanes x RP pixel rows; lane (row, col) walks pixels bx RP + row + t nbx RP
template <int OT, int CPL, bool DX, bool DWG>
__global__ __launch_bounds__(256) void k_headconv_bwd(const unsigned short *__restrict__ x, const float *__restrict__ dy, const float *__restrict__ w, int64_t N, int cin,
                                                      int cout, int CW, int RP, int64_t iters, unsigned short *__restrict__ dx, float *__restrict__ slab) {
    constexpr int OP = OT < 8 ? OT : 8;  // outputs per LDS pass
    __shared__ __attribute__((aligned(16))) float red[256 * 8 * 2];
    const int tid = threadIdx.x, col = tid % CW, row = tid / CW;
    const int c0 = (blockIdx.y * CW + col) * CPL;
    const bool act = row < RP && c0 < cin, dbl = DWG && col == 0 && blockIdx.y == 0;
    float wt[OT][CPL], acc[OT][CPL], dbs[OT];
#pragma unroll
    for (int o = 0; o < OT; ++o) {
        dbs[o] = 0.f;
#pragma unroll
        for (int k = 0; k < CPL; ++k) { wt[o][k] = 0.f; acc[o][k] = 0.f; }
    }
    if (DX && act) {
#pragma unroll
        for (int o = 0; o < OT; ++o)
            if (o < cout) {
#pragma unroll
                for (int k = 0; k < CPL; ++k) wt[o][k] = bf16_round(w[(size_t)o * cin + c0 + k]);
            }
    }
    // the dy rows of the workgroup's RP pixels of pass t, rounded once into LDS as [row][OT] (zeros past cout and past N) by all 256 threads --
    // one coalesced read -- and read back by the CW lanes of each row; two buffers (the halves of `red`), one barrier per pass
    const int64_t stride = (int64_t)gridDim.x * RP;
    for (int64_t t = 0; t < iters; ++t) {
        float *buf = red + (int)(t & 1) * 2048;
        const int64_t n0 = (int64_t)blockIdx.x * RP + t * stride;
        for (int e = tid; e < RP * OT; e += 256) {
            const int r = e / OT, o = e % OT;
            buf[e] = (o < cout && n0 + r < N) ? bf16_round(dy[(size_t)(n0 + r) * cout + o]) : 0.f;
        }
        __syncthreads();
        const int64_t n = n0 + row;
        if (act && n < N) {
            float d[OT], xv[CPL];
#pragma unroll
            for (int q = 0; q < OT / 4; ++q) {
                const float4 v = reinterpret_cast<const float4 *>(buf + row * OT)[q];
                d[4 * q] = v.x; d[4 * q + 1] = v.y; d[4 * q + 2] = v.z; d[4 * q + 3] = v.w;
            }
            if (DWG) {
                if (CPL == 2) {
                    const unsigned u = *reinterpret_cast<const unsigned *>(x + (size_t)n * cin + c0);
                    xv[0] = bf16_lo(u);
                    xv[CPL - 1] = bf16_hi(u);
                } else {
                    xv[0] = bf16_widen(x[(size_t)n * cin + c0]);
                }
            }
            if (DX) {
                float g[CPL];
#pragma unroll
                for (int k = 0; k < CPL; ++k) g[k] = 0.f;
#pragma unroll
                for (int o = 0; o < OT; ++o)
#pragma unroll
                    for (int k = 0; k < CPL; ++k) g[k] = fmaf(wt[o][k], d[o], g[k]);
                if (CPL == 2)
                    *reinterpret_cast<unsigned *>(dx + (size_t)n * cin + c0) = bf16_pack2(g[0], g[CPL - 1]);
                else
                    dx[(size_t)n * cin + c0] = bf16_rne(g[0]);
            }
            if (DWG) {
#pragma unroll
                for (int o = 0; o < OT; ++o)
#pragma unroll
                    for (int k = 0; k < CPL; ++k) acc[o][k] = fmaf(xv[k], d[o], acc[o][k]);
                if (dbl) {
#pragma unroll
                    for (int o = 0; o < OT; ++o) dbs[o] += d[o];
                }
            }
        }
    }
    if (!DWG) return;
    __syncthreads();  // the last pass's reads of `red` are over
    const size_t nel = (size_t)cout * cin + cout;
    float *mine = slab + (size_t)blockIdx.x * nel;
#pragma unroll
    for (int o0 = 0; o0 < OT; o0 += OP) {
        if (o0 >= cout) break;  // (uniform) the padded outputs: nothing to store
        if (row < RP) {
#pragma unroll
            for (int oo = 0; oo < OP; ++oo)
#pragma unroll
                for (int k = 0; k < CPL; ++k) red[(row * CW + col) * (OP * CPL) + oo * CPL + k] = acc[o0 + oo][k];
        }
        lds_row_tree<OP * CPL>(red, 0, row, col, CW, RP);
        for (int e = tid; e < CW * OP * CPL; e += 256) {  // row 0: [col][oo][k]
            const int r = e % (OP * CPL), o = o0 + r / CPL, c = (blockIdx.y * CW + e / (OP * CPL)) * CPL + r % CPL;
            if (o < cout && c < cin) mine[(size_t)o * cin + c] = red[e];
        }
        __syncthreads();
    }
    if (blockIdx.y != 0) return;
    if (row < RP && col == 0) {
#pragma unroll
        for (int o = 0; o < OT; ++o) red[row * OT + o] = dbs[o];
    }
    lds_row_tree<OT>(red, 0, row, 0, 1, RP, col == 0);  // one column of OT values per row
    if (tid < cout) mine[(size_t)cout * cin + tid] = red[tid];
}

// ---------------------------------------------------------------------------------------------- stem
__device__ __forceinline__ void stem_table(float *tab) {  // tab[v] = bf16(v / 255)
    for (int v = threadIdx.x; v < 256; v += blockDim.x) tab[v] = bf16_round((float)v / 255.0f);
}
// the CIN operands of input pixel (yy, xx) of image `img`
template <int CIN>
__device__ __forceinline__ void stem_pixel(const unsigned char *__restrict__ img, int yy, int xx, int W, const float *tab, float xv[CIN]) {
    const unsigned char *p = img + ((size_t)yy * W + xx) * CIN;
    if (CIN == 4) {
        const unsigned u = *reinterpret_cast<const unsigned *>(p);
        xv[0] = tab[u & 255u]; xv[1] = tab[(u >> 8) & 255u]; xv[2] = tab[(u >> 16) & 255u]; xv[CIN - 1] = tab[u >> 24];
    } else {
#pragma unroll
        for (int c = 0; c < CIN; ++c) xv[c] = tab[p[c]];
    }
}

// forward: one (output pixel, group of OC 8-channel chunks) item per lane, group fastest
template <int CIN, int OC>
__global__ __launch_bounds__(256) void k_stemconv_fwd(const unsigned char *__restrict__ x, const float *__restrict__ w, int H, int W, int Ho, int Wo, int cout, int64_t nitem,
                                                      unsigned short *__restrict__ z) {
    __shared__ float tab[256];
    __shared__ __attribute__((aligned(16))) float wl[9 * CIN * kStemMaxCout];  // [tap][c][cout], rounded
    stem_table(tab);
    for (int e = threadIdx.x; e < 9 * CIN * cout; e += 256) {
        const int o = e % cout, tc = e / cout, c = tc % CIN, tap = tc / CIN;
        wl[e] = bf16_round(w[((size_t)o * CIN + c) * 9 + tap]);
    }
    __syncthreads();
    const int G = cout / (8 * OC);
    const int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (it >= nitem) return;
    const int o0 = (int)(it % G) * 8 * OC;
    const int64_t pix = it / G;
    const int j = (int)(pix % Wo), i = (int)((pix / Wo) % Ho);
    const int64_t b = pix / ((int64_t)Wo * Ho);
    const unsigned char *img = x + (size_t)b * H * W * CIN;
    float acc[8 * OC];
#pragma unroll
    for (int k = 0; k < 8 * OC; ++k) acc[k] = 0.f;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        const int yy = 2 * i + ky - 1;
        if (yy < 0 || yy >= H) continue;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int xx = 2 * j + kx - 1;
            if (xx < 0 || xx >= W) continue;
            float xv[CIN];
            stem_pixel<CIN>(img, yy, xx, W, tab, xv);
#pragma unroll
            for (int c = 0; c < CIN; ++c) {
                const float4 *wr = reinterpret_cast<const float4 *>(wl + ((ky * 3 + kx) * CIN + c) * cout + o0);
#pragma unroll
                for (int q = 0; q < 2 * OC; ++q) {
                    const float4 wv = wr[q];
                    acc[4 * q] = fmaf(wv.x, xv[c], acc[4 * q]); acc[4 * q + 1] = fmaf(wv.y, xv[c], acc[4 * q + 1]);
                    acc[4 * q + 2] = fmaf(wv.z, xv[c], acc[4 * q + 2]); acc[4 * q + 3] = fmaf(wv.w, xv[c], acc[4 * q + 3]);
                }
            }
        }
    }
    uint4 *zr = reinterpret_cast<uint4 *>(z + (size_t)pix * cout + o0);
#pragma unroll
    for (int q = 0; q < OC; ++q) zr[q] = pack8_bf16(acc + 8 * q);
}

// wgrad: grid nbx, workgroup = CW lanes of 4 outputs x RP pixel rows; lane (row, col) walks output pixels bx RP + row + t nbx RP
template <int CIN>
__global__ __launch_bounds__(256) void k_stemconv_wgrad(const unsigned char *__restrict__ x, const unsigned short *__restrict__ dz, int H, int W, int Ho, int Wo, int cout,
                                                        int64_t NP, int CW, int RP, int64_t iters, float *__restrict__ slab) {
    __shared__ float tab[256];
    __shared__ __attribute__((aligned(16))) float red[256 * CIN * 4];
    stem_table(tab);
    __syncthreads();
    const int tid = threadIdx.x, col = tid % CW, row = tid / CW;
    float acc[9][CIN][4];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int c = 0; c < CIN; ++c)
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[t][c][k] = 0.f;
    if (row < RP)
        for (int64_t t = 0; t < iters; ++t) {
            const int64_t pix = (int64_t)blockIdx.x * RP + row + t * gridDim.x * RP;
            if (pix >= NP) break;
            const int j = (int)(pix % Wo), i = (int)((pix / Wo) % Ho);
            const int64_t b = pix / ((int64_t)Wo * Ho);
            const unsigned char *img = x + (size_t)b * H * W * CIN;
            const uint2 dv = *reinterpret_cast<const uint2 *>(dz + (size_t)pix * cout + col * 4);
            const float d[4] = {bf16_lo(dv.x), bf16_hi(dv.x), bf16_lo(dv.y), bf16_hi(dv.y)};
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                const int yy = 2 * i + ky - 1;
                if (yy < 0 || yy >= H) continue;
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const int xx = 2 * j + kx - 1;
                    if (xx < 0 || xx >= W) continue;
                    float xv[CIN];
                    stem_pixel<CIN>(img, yy, xx, W, tab, xv);
#pragma unroll
                    for (int c = 0; c < CIN; ++c)
#pragma unroll
                        for (int k = 0; k < 4; ++k) acc[ky * 3 + kx][c][k] = fmaf(xv[c], d[k], acc[ky * 3 + kx][c][k]);
                }
            }
        }
    float *mine = slab + (size_t)blockIdx.x * 9 * CIN * cout;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        if (row < RP) {
#pragma unroll
            for (int c = 0; c < CIN; ++c)
#pragma unroll
                for (int k = 0; k < 4; ++k) red[(row * CW + col) * (CIN * 4) + c * 4 + k] = acc[tap][c][k];
        }
        lds_row_tree<CIN * 4>(red, 0, row, col, CW, RP);
        if (tid < CW * CIN * 4) {  // row 0: [col][c][k]
            const int r = tid % (CIN * 4), c = r / 4, o = (tid / (CIN * 4)) * 4 + r % 4;
            mine[((size_t)tap * CIN + c) * cout + o] = red[tid];
        }
        __syncthreads();
    }
}

namespace {
bool nr_aligned(const void *p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }  // (NULL passes)

int head_check(obb_ctx *ctx, const char *fn, int64_t N, int32_t cin, int32_t cout) {
    OBB_REQUIRE(ctx, ctx && cin >= 8 && cin <= kHeadMaxCin && cin % 8 == 0, "%s: cin = %d must be a multiple of 8 in [8, %d]", fn, (int)cin, kHeadMaxCin);
    OBB_REQUIRE(ctx, cout >= 1 && cout <= kHeadMaxCout, "%s: cout = %d must be in [1, %d]", fn, (int)cout, kHeadMaxCout);
    OBB_REQUIRE(ctx, N >= 1 && N < (1ll << 36), "%s: N = %lld pixels must be in [1, 2^36)", fn, (long long)N);
    return OBB_OK;
}

int stem_check(obb_ctx *ctx, const char *fn, int32_t B, int32_t H, int32_t W, int32_t cin, int32_t cout) {
    OBB_REQUIRE(ctx, ctx && (cin == 3 || cin == 4), "%s: cin = %d must be 3 or 4", fn, (int)cin);
    OBB_REQUIRE(ctx, cout >= 8 && cout <= kStemMaxCout && cout % 8 == 0, "%s: cout = %d must be a multiple of 8 in [8, %d]", fn, (int)cout, kStemMaxCout);
    OBB_REQUIRE(ctx, B >= 1 && H >= 1 && W >= 1, "%s: B = %d, H = %d, W = %d must be at least 1", fn, (int)B, (int)H, (int)W);
    OBB_REQUIRE(ctx, (int64_t)B * H * W < (1ll << 36), "%s: B = %d, H = %d, W = %d: too large", fn, (int)B, (int)H, (int)W);
    return OBB_OK;
}

template <int OT, int CPL>
void head_launch_bwd(const HeadGeo &g, hipStream_t st, const uint16_t *x, const float *dy, const float *w, int64_t N, int cin, int cout, uint16_t *dx, float *slab) {
    const dim3 grid((unsigned)g.nbx, (unsigned)g.ny), blk(256);
    if (dx && slab)
        hipLaunchKernelGGL((k_headconv_bwd<OT, CPL, true, true>), grid, blk, 0, st, x, dy, w, N, cin, cout, g.CW, g.RP, g.iters, dx, slab);
    else if (dx)
        hipLaunchKernelGGL((k_headconv_bwd<OT, CPL, true, false>), grid, blk, 0, st, x, dy, w, N, cin, cout, g.CW, g.RP, g.iters, dx, slab);
    else
        hipLaunchKernelGGL((k_headconv_bwd<OT, CPL, false, true>), grid, blk, 0, st, x, dy, w, N, cin, cout, g.CW, g.RP, g.iters, dx, slab);
}
}  // namespace

}  // namespace obb

using namespace obb;

extern "C" {

int obb_headconv_bwd_geometry(int64_t N, int32_t cin, int32_t cout, int32_t out[4]) {
    if (!out || N < 1 || N >= (1ll << 36) || cin < 8 || cin > kHeadMaxCin || cin % 8 || cout < 1 || cout > kHeadMaxCout) return OBB_ERR_INVALID;
    const HeadGeo g = head_geo(N, cin, cout);
    out[0] = (int32_t)std::min<int64_t>(g.iters, INT32_MAX);
    out[1] = g.RP;
    out[2] = g.nbx;
    out[3] = g.L;
    return OBB_OK;
}

int obb_stemconv_wgrad_geometry(int32_t B, int32_t H, int32_t W, int32_t cin, int32_t cout, int32_t out[4]) {
    if (!out || B < 1 || H < 1 || W < 1 || (cin != 3 && cin != 4) || cout < 8 || cout > kStemMaxCout || cout % 8 || (int64_t)B * H * W >= (1ll << 36))
        return OBB_ERR_INVALID;
    const StemGeo g = stem_geo(B, H, W, cout);
    out[0] = (int32_t)std::min<int64_t>(g.iters, INT32_MAX);
    out[1] = g.RP;
    out[2] = g.nbx;
    out[3] = g.L;
    return OBB_OK;
}

int obb_headconv_fwd_bf16(obb_ctx *ctx, const uint16_t *x, const float *w, const float *bias, int64_t N, int32_t cin, int32_t cout, float *y, obb_stream_t s) {
    if (int rc = head_check(ctx, "obb_headconv_fwd_bf16", N, cin, cout)) return rc;
    OBB_REQUIRE(ctx, x && w && y, "obb_headconv_fwd_bf16: NULL buffer");
    OBB_REQUIRE(ctx, nr_aligned(x, 16) && nr_aligned(y, 4) && nr_aligned(w, 4) && nr_aligned(bias, 4), "obb_headconv_fwd_bf16: x must be 16-byte aligned, w, bias and y 4-byte");
    const dim3 grid((unsigned)cdiv(N, kHeadFwdThreads));
    if (cout <= 4)
        hipLaunchKernelGGL((k_headconv_fwd<4>), grid, dim3(kHeadFwdThreads), 0, (hipStream_t)s, x, w, bias, N, (int)cin, (int)cout, y);
    else
        hipLaunchKernelGGL((k_headconv_fwd<16>), grid, dim3(kHeadFwdThreads), 0, (hipStream_t)s, x, w, bias, N, (int)cin, (int)cout, y);
    OBB_LAUNCH_CHECK(ctx);
    return OBB_OK;
}

int obb_headconv_bwd_bf16(obb_ctx *ctx, const uint16_t *x, const float *dy, const float *w, int64_t N, int32_t cin, int32_t cout, uint16_t *dx, float *dw, float *db,
                          obb_stream_t s) {
    if (int rc = head_check(ctx, "obb_headconv_bwd_bf16", N, cin, cout)) return rc;
    const bool grads = dw || db;
    OBB_REQUIRE(ctx, dx || grads, "obb_headconv_bwd_bf16: dx, dw and db are all NULL: nothing to compute");
    OBB_REQUIRE(ctx, dy && (!dx || w) && (!grads || x), "obb_headconv_bwd_bf16: NULL buffer (dy; w for dx; x for dw / db)");
    OBB_REQUIRE(ctx, nr_aligned(x, 4) && nr_aligned(dx, 4) && nr_aligned(dy, 4) && nr_aligned(w, 4) && nr_aligned(dw, 4) && nr_aligned(db, 4),
                "obb_headconv_bwd_bf16: every buffer must be 4-byte aligned");
    hipStream_t st = (hipStream_t)s;
    const HeadGeo g = head_geo(N, cin, cout);
    float *slab = nullptr;
    if (grads) {
        slab = (float *)ctx->workspace(WS_TRAIN_E, (size_t)g.nbx * ((size_t)cout * cin + cout) * 4);
        if (!slab) return set_error(ctx, OBB_ERR_HIP, "obb_headconv_bwd_bf16: workspace allocation failed");
    }
    if (g.OT == 4)
        head_launch_bwd<4, 2>(g, st, x, dy, w, N, (int)cin, (int)cout, dx, slab);
    else if (g.OT == 16)
        head_launch_bwd<16, 2>(g, st, x, dy, w, N, (int)cin, (int)cout, dx, slab);
    else
        head_launch_bwd<64, 1>(g, st, x, dy, w, N, (int)cin, (int)cout, dx, slab);
    if (grads)
        hipLaunchKernelGGL((k_narrow_final<false>), dim3((unsigned)cdiv((int64_t)cout * cin + cout, kSlabWalkEl)), dim3(256), 0, st, slab, g.nbx, (int)cin, (int)cout, dw, db);
    OBB_LAUNCH_CHECK(ctx);
    return OBB_OK;
}

int obb_stemconv_fwd_u8(obb_ctx *ctx, const uint8_t *x, const float *w, int32_t B, int32_t H, int32_t W, int32_t cin, int32_t cout, uint16_t *z, obb_stream_t s) {
    if (int rc = stem_check(ctx, "obb_stemconv_fwd_u8", B, H, W, cin, cout)) return rc;
    OBB_REQUIRE(ctx, x && w && z, "obb_stemconv_fwd_u8: NULL buffer");
    OBB_REQUIRE(ctx, (cin == 3 || nr_aligned(x, 4)) && nr_aligned(z, 16) && nr_aligned(w, 4), "obb_stemconv_fwd_u8: z must be 16-byte aligned, w 4-byte, x 4-byte at cin = 4");
    const StemGeo g = stem_geo(B, H, W, cout);
    const int OC = cout % 16 == 0 ? 2 : 1;
    const int64_t nitem = g.NP * (cout / (8 * OC));
    const dim3 grid((unsigned)cdiv(nitem, 256));
    hipStream_t st = (hipStream_t)s;
#define OBB_STEM_FWD(CIN, OCN) hipLaunchKernelGGL((k_stemconv_fwd<CIN, OCN>), grid, dim3(256), 0, st, x, w, (int)H, (int)W, g.Ho, g.Wo, (int)cout, nitem, z)
    if (cin == 3) { if (OC == 2) OBB_STEM_FWD(3, 2); else OBB_STEM_FWD(3, 1); }
    else { if (OC == 2) OBB_STEM_FWD(4, 2); else OBB_STEM_FWD(4, 1); }
#undef OBB_STEM_FWD
    OBB_LAUNCH_CHECK(ctx);
    return OBB_OK;
}

int obb_stemconv_wgrad_u8(obb_ctx *ctx, const uint8_t *x, const uint16_t *dz, int32_t B, int32_t H, int32_t W, int32_t cin, int32_t cout, float *dw, obb_stream_t s) {
    if (int rc = stem_check(ctx, "obb_stemconv_wgrad_u8", B, H, W, cin, cout)) return rc;
    OBB_REQUIRE(ctx, x && dz && dw, "obb_stemconv_wgrad_u8: NULL buffer");
    OBB_REQUIRE(ctx, (cin == 3 || nr_aligned(x, 4)) && nr_aligned(dz, 16) && nr_aligned(dw, 4), "obb_stemconv_wgrad_u8: dz must be 16-byte aligned, dw 4-byte, x 4-byte at cin = 4");
    const StemGeo g = stem_geo(B, H, W, cout);
    hipStream_t st = (hipStream_t)s;
    float *slab = (float *)ctx->workspace(WS_TRAIN_E, (size_t)g.nbx * 9 * cin * cout * 4);
    if (!slab) return set_error(ctx, OBB_ERR_HIP, "obb_stemconv_wgrad_u8: workspace allocation failed");
    if (cin == 3)
        hipLaunchKernelGGL((k_stemconv_wgrad<3>), dim3((unsigned)g.nbx), dim3(256), 0, st, x, dz, (int)H, (int)W, g.Ho, g.Wo, (int)cout, g.NP, g.CW, g.RP, g.iters, slab);
    else
        hipLaunchKernelGGL((k_stemconv_wgrad<4>), dim3((unsigned)g.nbx), dim3(256), 0, st, x, dz, (int)H, (int)W, g.Ho, g.Wo, (int)cout, g.NP, g.CW, g.RP, g.iters, slab);
    hipLaunchKernelGGL((k_narrow_final<true>), dim3((unsigned)cdiv(9 * (int64_t)cin * cout, kSlabWalkEl)), dim3(256), 0, st, slab, g.nbx, (int)cin, (int)cout, dw, (float *)nullptr);
    OBB_LAUNCH_CHECK(ctx);
    return OBB_OK;
}

}  // extern "C"
