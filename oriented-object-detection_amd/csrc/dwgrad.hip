// Training-mode depthwise 3x3 convolution (stride 1, pad 1, groups = C) of the Ultralytics `DWConv` / `Conv(g=c)` blocks (SURVEY.md section 8 row
// f1, `model.train(...)`, Train_OBB.py:796-841: the head's class branch model.23.cv3.i.{0,1}.0 and C2PSA's attn.pe): forward and a FUSED backward
// that takes dx and dw from one pass over x and dz.  bf16 NHWC tensors, C % 8 == 0: a lane moves one 16-byte chunk (8 channels).  The fp32 master
// weights w[C][1][3][3] are rounded to bf16 (nearest even) as they are loaded -- what bf16 autocast hands F.conv2d -- products and sums are fp32
// (a bf16 x bf16 product is exact in fp32, so fmaf is the product followed by the addition), one bf16 rounding at each bf16 store.
//
//   forward   z[b,i,j,c]   = sum_{ky,kx} w~[c,ky,kx] x[b, i+ky-1, j+kx-1, c]      taps added in (ky, kx) ascending order from 0, zero padding
//   backward  dx[b,i,j,c]  = sum_{ky,kx} w~[c,ky,kx] dz[b, i-ky+1, j-kx+1, c]     same order
//             dw[c,ky,kx]  = sum_{b,i,j} x[b,i,j,c] dz[b, i-ky+1, j-kx+1, c]      (= sum dz[p] x[p + (ky-1, kx-1)], summed over the x pixel)
//
// Work split (dw_geo, the ONE place that decides it; obb_dwconv3_bwd_geometry returns it): the map is cut into stripes of R rows (R = 4 above 16
// rows, else 2: the rule depends on the map alone).  A RUN is one pixel column of one stripe of one image; a lane owns one channel chunk of a
// run and walks its rows with a three-row register window: 3 loads per row of the windowed tensor instead of 9.  Both gradients read the SAME
// dz window (dx: the flipped taps; dw: the window times the centre x), so the fused backward loads 3 dz chunks + 1 x chunk per pixel -- each of
// x and dz comes from HBM once, the column neighbours and the stripe halo (2 rows per R) from the caches.
// dw: a lane keeps 9 x 8 fp32 sums over its runs (`iters` of them once the run count exceeds kDwMaxSlabs workgroups' worth).  A workgroup is CW
// chunk columns x RP run rows of lanes (traindev.h's row_split); the RP lanes of a chunk meet in LDS in lds_row_tree, three tap planes per pass
// under one barrier per step (24 KiB).  Workgroup bx writes its partial to the fp32 slab [bx][9][C] (WS_TRAIN_E, never read before it is
// written: growing the slot changes nothing); k_dw_final adds the slabs in slab_combine's order.  No atomics: bit-reproducible.  Longest fp32
// addition chain of a dw element: L = R iters + ceil(log2 RP) + slab_chain(nbx) (= ceil(nbx / 64) + 6).
#include <algorithm>

#include "ctx.h"
#include "traindev.h"

namespace obb {
namespace {

constexpr int kDwMaxSlabs = 512;    // workgroups per column group at most: beyond, a lane walks several runs
constexpr int kDwTapsPerPass = 3;   // taps reduced per LDS pass: 3 x 256 x 8 floats = 24 KiB

// the 72 weights of channel chunk c8 -> wt[tap][lane channel], rounded to bf16
__device__ __forceinline__ void dw_load_weights(const float *__restrict__ w, int c8, float wt[9][8]) {
    const float *wc = w + (size_t)c8 * 72;
#pragma unroll
    for (int k = 0; k < 8; ++k)
#pragma unroll
        for (int t = 0; t < 9; ++t) wt[t][k] = bf16_round(wc[k * 9 + t]);
}
// row `i` of the window: columns j - 1, j, j + 1 of image row i (zero outside the map); img: the image's first element, chunk offset included
__device__ __forceinline__ void dw_load_row(const unsigned short *__restrict__ img, int i, int j, int H, int W, int C, uint4 r[3]) {
    const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
    r[0] = r[1] = r[2] = zero;
    if (i < 0 || i >= H) return;
    const unsigned short *p = img + ((size_t)i * W + j) * C;
    r[1] = *reinterpret_cast<const uint4 *>(p);
    if (j > 0) r[0] = *reinterpret_cast<const uint4 *>(p - C);
    if (j + 1 < W) r[2] = *reinterpret_cast<const uint4 *>(p + C);
}

// Work split of the backward (and the stripes of the forward)
struct DwGeo : RowSplit { int R, ns, nbx, iters, L; int64_t P; };
DwGeo dw_geo(int B, int H, int W, int C) {
    DwGeo g;
    static_cast<RowSplit &>(g) = row_split(C);
    g.R = H > 16 ? 4 : 2;
    g.ns = (int)cdiv(H, g.R);
    g.P = (int64_t)B * g.ns * W;                                        // runs
    g.nbx = (int)std::min<int64_t>(cdiv(g.P, g.RP), kDwMaxSlabs);       // workgroups per column group = slabs
    g.iters = (int)std::min<int64_t>(cdiv(g.P, (int64_t)g.nbx * g.RP), 1 << 30);  // runs per lane
    g.L = (int)std::min<int64_t>((int64_t)g.R * g.iters + g.depth + slab_chain(g.nbx), INT32_MAX);
    return g;
}

}  // namespace

// forward: one (image, stripe, column, chunk) item per lane, chunk fastest
template <int R>
__global__ __launch_bounds__(256) void k_dwconv3_fwd(const unsigned short *__restrict__ x, const float *__restrict__ w, int H, int W, int C, int ns, int64_t nitem,
                                                     unsigned short *__restrict__ z) {
    const int C8 = C / 8;
    const int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (it < nitem) {
        const int c8 = (int)(it % C8);
        const int64_t run = it / C8;
        const int j = (int)(run % W), s = (int)((run / W) % ns);
        const int64_t b = run / ((int64_t)W * ns);
        const size_t base = (size_t)b * H * W * C + (size_t)c8 * 8;
        const unsigned short *img = x + base;
        float wt[9][8];
        dw_load_weights(w, c8, wt);
        const int i0 = s * R;
        uint4 win[3][3];
        dw_load_row(img, i0 - 1, j, H, W, C, win[0]);
        dw_load_row(img, i0, j, H, W, C, win[1]);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = i0 + r;
            if (i < H) {
                dw_load_row(img, i + 1, j, H, W, C, win[2]);
                float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, f[8];
#pragma unroll
                for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                    for (int kx = 0; kx < 3; ++kx) {
                        unpack8_bf16(win[ky][kx], f);
#pragma unroll
                        for (int k = 0; k < 8; ++k) acc[k] = fmaf(wt[ky * 3 + kx][k], f[k], acc[k]);
                    }
                *reinterpret_cast<uint4 *>(z + base + ((size_t)i * W + j) * C) = pack8_bf16(acc);
#pragma unroll
                for (int q = 0; q < 3; ++q) { win[0][q] = win[1][q]; win[1][q] = win[2][q]; }
            }
        }
    }
}

// fused backward: grid (nbx, ny), workgroup = CW chunk columns x RP run rows; lane (row, col) of workgroup bx walks runs bx * RP + row + t * nbx * RP
template <int R, bool DX, bool DWG>
__global__ __launch_bounds__(256) void k_dwconv3_bwd(const unsigned short *__restrict__ x, const unsigned short *__restrict__ dz, const float *__restrict__ w, int H, int W,
                                                     int C, int ns, int64_t P, int CW, int RP, int iters, unsigned short *__restrict__ dx, float *__restrict__ slab) {
    __shared__ __attribute__((aligned(16))) float red[kDwTapsPerPass * 256 * 8];
    const int tid = threadIdx.x, col = tid % CW, row = tid / CW;
    const int C8 = C / 8, c8 = blockIdx.y * kGroupChunks + col;
    const bool act = row < RP && c8 < C8;
    float wt[9][8], acc[9][8];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int k = 0; k < 8; ++k) { wt[t][k] = 0.f; acc[t][k] = 0.f; }
    if (DX && act) dw_load_weights(w, c8, wt);
    if (act)
        for (int t = 0; t < iters; ++t) {
            const int64_t run = (int64_t)blockIdx.x * RP + row + (int64_t)t * gridDim.x * RP;
            if (run >= P) break;
            const int j = (int)(run % W), s = (int)((run / W) % ns);
            const int64_t b = run / ((int64_t)W * ns);
            const size_t base = (size_t)b * H * W * C + (size_t)c8 * 8;
            const unsigned short *dimg = dz + base;
            const int i0 = s * R;
            uint4 win[3][3];  // dz rows i - 1, i, i + 1 x columns j - 1, j, j + 1
            dw_load_row(dimg, i0 - 1, j, H, W, C, win[0]);
            dw_load_row(dimg, i0, j, H, W, C, win[1]);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int i = i0 + r;
                if (i < H) {
                    dw_load_row(dimg, i + 1, j, H, W, C, win[2]);
                    float xc[8], g[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, f[8];
                    if (DWG) unpack8_bf16(*reinterpret_cast<const uint4 *>(x + base + ((size_t)i * W + j) * C), xc);
#pragma unroll
                    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                        for (int kx = 0; kx < 3; ++kx) {
                            unpack8_bf16(win[2 - ky][2 - kx], f);  // dz[i - ky + 1, j - kx + 1]
#pragma unroll
                            for (int k = 0; k < 8; ++k) {
                                if (DX) g[k] = fmaf(wt[ky * 3 + kx][k], f[k], g[k]);
                                if (DWG) acc[ky * 3 + kx][k] = fmaf(xc[k], f[k], acc[ky * 3 + kx][k]);
                            }
                        }
                    if (DX) *reinterpret_cast<uint4 *>(dx + base + ((size_t)i * W + j) * C) = pack8_bf16(g);
#pragma unroll
                    for (int q = 0; q < 3; ++q) { win[0][q] = win[1][q]; win[1][q] = win[2][q]; }
                }
            }
        }
    if (!DWG) return;
    // the RP lanes of a chunk column: pairwise tree over the rows, kDwTapsPerPass taps at a time; plane p of `red` is [row][col][8]
#pragma unroll
    for (int t0 = 0; t0 < 9; t0 += kDwTapsPerPass) {
        if (row < RP) {
#pragma unroll
            for (int p = 0; p < kDwTapsPerPass; ++p) {
                float4 *r4 = reinterpret_cast<float4 *>(red + p * 2048 + (row * CW + col) * 8);
                r4[0] = make_float4(acc[t0 + p][0], acc[t0 + p][1], acc[t0 + p][2], acc[t0 + p][3]);
                r4[1] = make_float4(acc[t0 + p][4], acc[t0 + p][5], acc[t0 + p][6], acc[t0 + p][7]);
            }
        }
        lds_row_tree<8, kDwTapsPerPass>(red, 2048, row, col, CW, RP);
        const int c = blockIdx.y * kGroupChunks * 8 + tid;  // row 0 of the plane: [col][8] = 8 CW consecutive channels
        if (tid < CW * 8 && c < C) {
#pragma unroll
            for (int p = 0; p < kDwTapsPerPass; ++p) slab[((size_t)blockIdx.x * 9 + t0 + p) * C + c] = red[p * 2048 + tid];
        }
        __syncthreads();
    }
}

// dw[c][tap] = sum over the slabs of slab[bx][tap][c]: element q = tap * C + c of the [nbx][9 C] matrix, walkers then the tree
__global__ __launch_bounds__(256) void k_dw_final(const float *__restrict__ slab, int nbx, int C, float *__restrict__ dw) {
    const int q = slab_elem();
    float a[1];
    if (!slab_combine<1>({slab}, nbx, 9 * C, q, a)) return;
    const int tap = q / C, c = q - tap * C;
    dw[(size_t)c * 9 + tap] = a[0];
}

namespace {
bool dw_aligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }  // a lane moves uint4 chunks (NULL passes)

int dw_check(obb_ctx *ctx, const char *fn, int32_t B, int32_t H, int32_t W, int32_t C) {
    OBB_REQUIRE(ctx, ctx && C >= 8 && C % 8 == 0, "%s: C = %d must be a positive multiple of 8", fn, (int)C);
    OBB_REQUIRE(ctx, B >= 1 && H >= 1 && W >= 1, "%s: B = %d, H = %d, W = %d must be at least 1", fn, (int)B, (int)H, (int)W);
    OBB_REQUIRE(ctx, (int64_t)B * H * W < (1ll << 40) && cdiv(C / 8, kGroupChunks) < 65536, "%s: B = %d, H = %d, W = %d, C = %d: too large", fn, (int)B, (int)H,
                (int)W, (int)C);
    return OBB_OK;
}

template <int R>
void dw_launch_bwd(const DwGeo &g, hipStream_t st, const uint16_t *x, const uint16_t *dz, const float *w, int H, int W, int C, uint16_t *dx, float *slab) {
    const dim3 grid((unsigned)g.nbx, (unsigned)g.ny), blk(256);
    if (dx && slab)
        hipLaunchKernelGGL((k_dwconv3_bwd<R, true, true>), grid, blk, 0, st, x, dz, w, H, W, C, g.ns, g.P, g.CW, g.RP, g.iters, dx, slab);
    else if (dx)
        hipLaunchKernelGGL((k_dwconv3_bwd<R, true, false>), grid, blk, 0, st, x, dz, w, H, W, C, g.ns, g.P, g.CW, g.RP, g.iters, dx, slab);
    else
        hipLaunchKernelGGL((k_dwconv3_bwd<R, false, true>), grid, blk, 0, st, x, dz, w, H, W, C, g.ns, g.P, g.CW, g.RP, g.iters, dx, slab);
}
}  // namespace

}  // namespace obb

using namespace obb;

extern "C" {

int obb_dwconv3_bwd_geometry(int32_t B, int32_t H, int32_t W, int32_t C, int32_t out[4]) {
    if (!out || B < 1 || H < 1 || W < 1 || C < 8 || C % 8) return OBB_ERR_INVALID;
    const DwGeo g = dw_geo(B, H, W, C);
    out[0] = g.R;
    out[1] = (int32_t)std::min<int64_t>((int64_t)g.R * g.iters, INT32_MAX);
    out[2] = g.nbx;
    out[3] = g.L;
    return OBB_OK;
}

int obb_dwconv3_fwd_bf16(obb_ctx *ctx, const uint16_t *x, const float *w, int32_t B, int32_t H, int32_t W, int32_t C, uint16_t *z, obb_stream_t s) {
    if (int rc = dw_check(ctx, "obb_dwconv3_fwd_bf16", B, H, W, C)) return rc;
    OBB_REQUIRE(ctx, x && w && z, "obb_dwconv3_fwd_bf16: NULL buffer");
    OBB_REQUIRE(ctx, dw_aligned(x) && dw_aligned(z), "obb_dwconv3_fwd_bf16: x and z must be 16-byte aligned");
    const DwGeo g = dw_geo(B, H, W, C);
    const int64_t nitem = g.P * g.C8;
    OBB_REQUIRE(ctx, cdiv(nitem, 256) < (1ll << 31), "obb_dwconv3_fwd_bf16: B = %d, H = %d, W = %d, C = %d: too many workgroups", (int)B, (int)H, (int)W, (int)C);
    const dim3 grid((unsigned)cdiv(nitem, 256));
    if (g.R == 4)
        hipLaunchKernelGGL((k_dwconv3_fwd<4>), grid, dim3(256), 0, (hipStream_t)s, x, w, (int)H, (int)W, (int)C, g.ns, nitem, z);
    else
        hipLaunchKernelGGL((k_dwconv3_fwd<2>), grid, dim3(256), 0, (hipStream_t)s, x, w, (int)H, (int)W, (int)C, g.ns, nitem, z);
    OBB_LAUNCH_CHECK(ctx);
    return OBB_OK;
}

int obb_dwconv3_bwd_bf16(obb_ctx *ctx, const uint16_t *x, const uint16_t *dz, const float *w, int32_t B, int32_t H, int32_t W, int32_t C, uint16_t *dx, float *dw,
                         obb_stream_t s) {
    if (int rc = dw_check(ctx, "obb_dwconv3_bwd_bf16", B, H, W, C)) return rc;
    OBB_REQUIRE(ctx, dz && (!dx || w) && (!dw || x), "obb_dwconv3_bwd_bf16: NULL buffer (dz; w for dx; x for dw)");
    OBB_REQUIRE(ctx, dx || dw, "obb_dwconv3_bwd_bf16: dx and dw are both NULL: nothing to compute");
    OBB_REQUIRE(ctx, dw_aligned(x) && dw_aligned(dz) && dw_aligned(dx), "obb_dwconv3_bwd_bf16: x, dz and dx must be 16-byte aligned");
    hipStream_t st = (hipStream_t)s;
    const DwGeo g = dw_geo(B, H, W, C);
    float *slab = nullptr;
    if (dw) {
        slab = (float *)ctx->workspace(WS_TRAIN_E, (size_t)g.nbx * 9 * C * 4);
        if (!slab) return set_error(ctx, OBB_ERR_HIP, "obb_dwconv3_bwd_bf16: workspace allocation failed");
    }
    if (g.R == 4)
        dw_launch_bwd<4>(g, st, x, dz, w, (int)H, (int)W, (int)C, dx, slab);
    else
        dw_launch_bwd<2>(g, st, x, dz, w, (int)H, (int)W, (int)C, dx, slab);
    if (dw) hipLaunchKernelGGL(k_dw_final, dim3((unsigned)cdiv(9 * (int64_t)C, kSlabWalkEl)), dim3(256), 0, st, slab, g.nbx, (int)C, dw);
    OBB_LAUNCH_CHECK(ctx);
    return OBB_OK;
}

}  // extern "C"
