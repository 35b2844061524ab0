// Gradient routing through the parts of the trunk that are not convolutions (`model.train(...)`, Train_OBB.py:796-841
// -> ultralytics SPPF / nn.Upsample / Concat): the three chained 5x5 max pools of SPPF (model 9), Upsample(2x) + Concat of the FPN (models 11/12,
// 14/15), the plain Concat of the PAN (models 18, 21) and the gradient sum of a tensor with two consumers.  bf16 NHWC tensors, channel counts
// multiples of 8: a lane moves one 16-byte chunk (8 channels; traindev.h's unpack8_bf16 / pack8_bf16, the one rounding rule).  No atomics, fixed
// summation order: bit-reproducible.  No workspace.
//
//   pools forward   cat = [x, y1, y2, y3], y_k = maxpool5x5(y_{k-1}) (stride 1, pad 2, padding never wins).  A workgroup owns one image and
//                   `share` channel chunks with their whole H x W map in LDS (two planes, pooled plane to plane); values are copied, never
//                   re-rounded.  The window is scanned dy then dx from -inf with a strict `>`, torch's rule for FINITE values, so ties (+0 / -0)
//                   come out alike.  Precondition: finite inputs (SiLU outputs are).  NaN is not propagated (torch's scan has an isnan clause),
//                   and a window that is all -inf routes no gradient (torch sends it to the window's first element).
//   pools backward  nothing saved but cat.  Level k = 3, 2, 1: member k - 1 of cat goes to LDS, every output pixel's argmax is recomputed as
//                   the FIRST maximum of that scan (a window offset 0..24 per channel), then every input pixel gathers g_{k-1}[p] =
//                   dcat_{k-1}[p] + sum over the <= 25 outputs q whose argmax is p of g_k[q] (fp32 in LDS, fixed order); dx = g_0 rounded to
//                   bf16 once.  LDS per chunk and pixel: two fp32 gradient planes (2 x 32 B) + the argmax bytes (8 B); the pool input
//                   (16 B) lives in the plane the level is about to write, dead before the first write.  72 B x 1024 = 72 KiB at the limit.
//   share           2 chunks per workgroup while H * W <= 512, 1 above (H, W <= 32 each): the rule depends on the map alone.
//   upcat           out = cat(nearest_upsample_up(a), b) along C, up in {1, 2}; backward da[p] = fp32 sum of the up^2 copies (dy then dx),
//                   db = the b slice; accum: the existing bf16 value is the first term of the fp32 sum.  One rounding per result.
//   add             out = bf16(fp32(a) + fp32(b)) over n elements, n % 8 == 0; out may alias a (a chunk is read before it is written, by the
//                   same lane): the residual adds of a PSA block and the gradient sum at their fan-outs.
//   chanwin         dst[p, d0:d0+n] = src[p, s0:s0+n] (+ add[p, a0:a0+n]) over npix pixels: a channel window of one NHWC tensor into a channel
//                   window of another -- `Tensor.chunk` / `split` / `torch.cat` inside C3k2 and C2PSA, and the sum of a concat member's gradient
//                   with the gradient that arrives from the chain.  Without add the chunk is copied as bits (never unpacked); with add one fp32
//                   add and one rounding, k_add_bf16's.  The other channels of dst are not touched.  dst may not overlap src or add.
#include <algorithm>

#include "ctx.h"
#include "launchcfg.h"
#include "traindev.h"

namespace obb {
namespace {

constexpr int kPoolMaxSide = 32;      // H, W <= 32: imgsz <= 1024 at stride 32
constexpr int kPoolMaxElems = 1024;   // pixels x chunks resident per workgroup
constexpr int kPoolBwdBytes = 72;     // LDS bytes per resident (pixel, chunk) in the backward
constexpr int kPoolFwdBytes = 32;

int pool_share(int H, int W) { return H * W * 2 <= kPoolMaxElems ? 2 : 1; }

}  // namespace

// grid: B * ngrp workgroups, workgroup (b, g) owns chunks g * share .. of image b; LDS: two planes of H * W * share uint4
__global__ __launch_bounds__(256) void k_sppf_pools_fwd(const unsigned short *__restrict__ x, int H, int W, int C, int share, int ngrp,
                                                        unsigned short *__restrict__ cat) {
    extern __shared__ __attribute__((aligned(16))) uint4 rg_sm[];
    const int HW = H * W, C8 = C / 8;
    const int b = blockIdx.x / ngrp, c8_0 = (blockIdx.x % ngrp) * share, cg = min(share, C8 - c8_0), n = HW * cg;
    uint4 *cur = rg_sm, *nxt = rg_sm + HW * share;
    const unsigned short *xb = x + (size_t)b * HW * C + c8_0 * 8;
    unsigned short *cb = cat + (size_t)b * HW * 4 * C + c8_0 * 8;
    for (int e = threadIdx.x; e < n; e += 256) {
        const int p = e / cg, ch = e - p * cg;
        const uint4 v = *reinterpret_cast<const uint4 *>(xb + (size_t)p * C + ch * 8);
        cur[e] = v;
        *reinterpret_cast<uint4 *>(cb + (size_t)p * 4 * C + ch * 8) = v;
    }
    for (int k = 1; k <= 3; ++k) {
        __syncthreads();
        for (int e = threadIdx.x; e < n; e += 256) {
            const int p = e / cg, ch = e - p * cg, py = p / W, px = p - py * W;
            float m[8], f[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) m[j] = -INFINITY;
            for (int yy = max(py - 2, 0); yy <= min(py + 2, H - 1); ++yy)
                for (int xx = max(px - 2, 0); xx <= min(px + 2, W - 1); ++xx) {
                    unpack8_bf16(cur[(yy * W + xx) * cg + ch], f);
#pragma unroll
                    for (int j = 0; j < 8; ++j) m[j] = f[j] > m[j] ? f[j] : m[j];
                }
            const uint4 r = pack8_bf16_exact(m);
            nxt[e] = r;
            *reinterpret_cast<uint4 *>(cb + (size_t)p * 4 * C + (size_t)k * C + ch * 8) = r;
        }
        uint4 *t = cur; cur = nxt; nxt = t;
    }
}

// same grid; LDS: [gradient plane A: n8 floats][gradient plane B: n8 floats][argmax bytes: 8 per (pixel, chunk)], n8 = H * W * share * 8
__global__ __launch_bounds__(256) void k_sppf_pools_bwd(const unsigned short *__restrict__ cat, const unsigned short *__restrict__ dcat, int H, int W, int C,
                                                        int share, int ngrp, unsigned short *__restrict__ dx) {
    extern __shared__ __attribute__((aligned(16))) uint4 rg_sm[];
    const int HW = H * W, C8 = C / 8;
    const int b = blockIdx.x / ngrp, c8_0 = (blockIdx.x % ngrp) * share, cg = min(share, C8 - c8_0), n = HW * cg;
    float4 *cur = reinterpret_cast<float4 *>(rg_sm), *nxt = cur + (size_t)HW * share * 2;
    uint2 *amax = reinterpret_cast<uint2 *>(cur + (size_t)HW * share * 4);
    const size_t ib = (size_t)b * HW * 4 * C + c8_0 * 8;
    const unsigned short *cb = cat + ib, *db = dcat + ib;
    unsigned short *xb = dx + (size_t)b * HW * C + c8_0 * 8;
    float f[8];
    for (int e = threadIdx.x; e < n; e += 256) {  // g_3 = dcat member 3
        const int p = e / cg, ch = e - p * cg;
        unpack8_bf16(*reinterpret_cast<const uint4 *>(db + (size_t)p * 4 * C + (size_t)3 * C + ch * 8), f);
        cur[2 * e] = make_float4(f[0], f[1], f[2], f[3]);
        cur[2 * e + 1] = make_float4(f[4], f[5], f[6], f[7]);
    }
    for (int k = 3; k >= 1; --k) {
        uint4 *val = reinterpret_cast<uint4 *>(nxt);  // the pool's input, member k - 1: dead before nxt is written
        for (int e = threadIdx.x; e < n; e += 256) {
            const int p = e / cg, ch = e - p * cg;
            val[e] = *reinterpret_cast<const uint4 *>(cb + (size_t)p * 4 * C + (size_t)(k - 1) * C + ch * 8);
        }
        __syncthreads();
        for (int e = threadIdx.x; e < n; e += 256) {  // argmax of output pixel p: first maximum, dy then dx
            const int p = e / cg, ch = e - p * cg, py = p / W, px = p - py * W;
            float m[8];
            unsigned code[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) { m[j] = -INFINITY; code[j] = 255u; }
            for (int yy = max(py - 2, 0); yy <= min(py + 2, H - 1); ++yy)
                for (int xx = max(px - 2, 0); xx <= min(px + 2, W - 1); ++xx) {
                    const unsigned c = (unsigned)((yy - py + 2) * 5 + (xx - px + 2));
                    unpack8_bf16(val[(yy * W + xx) * cg + ch], f);
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        if (f[j] > m[j]) { m[j] = f[j]; code[j] = c; }
                }
            amax[e] = make_uint2(code[0] | (code[1] << 8) | (code[2] << 16) | (code[3] << 24), code[4] | (code[5] << 8) | (code[6] << 16) | (code[7] << 24));
        }
        __syncthreads();
        for (int e = threadIdx.x; e < n; e += 256) {  // input pixel p gathers from the outputs whose argmax it is
            const int p = e / cg, ch = e - p * cg, py = p / W, px = p - py * W;
            float acc[8];
            unpack8_bf16(*reinterpret_cast<const uint4 *>(db + (size_t)p * 4 * C + (size_t)(k - 1) * C + ch * 8), acc);
            // output q = p - (oy, ox) holds p at window offset (oy, ox)
            for (int oy = -2; oy <= 2; ++oy) {
                const int qy = py - oy;
                if (qy < 0 || qy >= H) continue;
                for (int ox = -2; ox <= 2; ++ox) {
                    const int qx = px - ox;
                    if (qx < 0 || qx >= W) continue;
                    const int q = (qy * W + qx) * cg + ch;
                    const unsigned c = (unsigned)((oy + 2) * 5 + (ox + 2));
                    const uint2 a = amax[q];
                    const float4 g0 = cur[2 * q], g1 = cur[2 * q + 1];
                    const float g[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const unsigned aj = ((j < 4 ? a.x : a.y) >> (8 * (j & 3))) & 255u;
                        if (aj == c) acc[j] += g[j];
                    }
                }
            }
            if (k > 1) {
                nxt[2 * e] = make_float4(acc[0], acc[1], acc[2], acc[3]);
                nxt[2 * e + 1] = make_float4(acc[4], acc[5], acc[6], acc[7]);
            } else {
                *reinterpret_cast<uint4 *>(xb + (size_t)p * C + ch * 8) = pack8_bf16(acc);
            }
        }
        __syncthreads();
        float4 *t = cur; cur = nxt; nxt = t;
    }
}

// one 16-byte chunk of out per thread and step: chunk c of pixel (b, y, x) comes from a[b, y / up, x / up] (c < Ca8) or b[b, y, x]
__global__ __launch_bounds__(256) void k_upcat_fwd(const unsigned short *__restrict__ a, const unsigned short *__restrict__ bsrc, int64_t nchunk, int uH, int uW, int Ca8,
                                                   int Cb8, int up, unsigned short *__restrict__ out) {
    const int Co8 = Ca8 + Cb8, H = uH / up, W = uW / up;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nchunk; i += (int64_t)gridDim.x * 256) {
        const int64_t pix = i / Co8;
        const int c = (int)(i - pix * Co8);
        uint4 v;
        if (c < Ca8) {
            const int x = (int)(pix % uW), y = (int)((pix / uW) % uH);
            const int64_t img = pix / ((int64_t)uW * uH);
            v = reinterpret_cast<const uint4 *>(a)[((img * H + y / up) * W + x / up) * Ca8 + c];
        } else {
            v = reinterpret_cast<const uint4 *>(bsrc)[pix * Cb8 + (c - Ca8)];
        }
        reinterpret_cast<uint4 *>(out)[i] = v;
    }
}

// chunks [0, nA) are da's (pixel of a, chunk of Ca8), chunks [nA, nA + nB) are db's (pixel of dout, chunk of Cb8)
__global__ __launch_bounds__(256) void k_upcat_bwd(const unsigned short *__restrict__ dout, int64_t nA, int64_t nB, int H, int W, int Ca8, int Cb8, int up,
                                                   unsigned short *__restrict__ da, unsigned short *__restrict__ db, int accum_a, int accum_b) {
    const int Co8 = Ca8 + Cb8, uW = W * up, uH = H * up;
    const uint4 *d4 = reinterpret_cast<const uint4 *>(dout);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nA + nB; i += (int64_t)gridDim.x * 256) {
        float acc[8], f[8];
        if (i < nA) {
            const int64_t pix = i / Ca8;
            const int c = (int)(i - pix * Ca8), x = (int)(pix % W), y = (int)((pix / W) % H);
            const int64_t img = pix / ((int64_t)W * H);
            uint4 *dst = reinterpret_cast<uint4 *>(da) + i;
            if (accum_a) unpack8_bf16(*dst, acc);
            else {
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[j] = 0.f;
            }
            for (int dy = 0; dy < up; ++dy)
                for (int dxx = 0; dxx < up; ++dxx) {
                    unpack8_bf16(d4[((img * uH + y * up + dy) * uW + x * up + dxx) * Co8 + c], f);
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[j] += f[j];
                }
            *dst = pack8_bf16(acc);
        } else {
            const int64_t k = i - nA, pix = k / Cb8;
            const int c = (int)(k - pix * Cb8);
            const uint4 v = d4[pix * Co8 + Ca8 + c];
            uint4 *dst = reinterpret_cast<uint4 *>(db) + k;
            if (accum_b) {
                unpack8_bf16(*dst, acc);
                unpack8_bf16(v, f);
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[j] += f[j];
                *dst = pack8_bf16(acc);
            } else {
                *dst = v;
            }
        }
    }
}

// one 16-byte chunk per thread and step
__global__ __launch_bounds__(256) void k_add_bf16(const unsigned short *a, const unsigned short *__restrict__ b, int64_t nchunk, unsigned short *out) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nchunk; i += (int64_t)gridDim.x * 256) {
        float x[8], y[8];
        unpack8_bf16(reinterpret_cast<const uint4 *>(a)[i], x);
        unpack8_bf16(reinterpret_cast<const uint4 *>(b)[i], y);
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] += y[j];
        reinterpret_cast<uint4 *>(out)[i] = pack8_bf16(x);
    }
}

// one 16-byte chunk of the window per thread and step: chunk c of pixel p is src chunk p * Cs8 + s8 + c
__global__ __launch_bounds__(256) void k_chanwin(const unsigned short *__restrict__ src, int Cs8, int s8, const unsigned short *__restrict__ add, int Ca8, int a8,
                                                 int64_t nchunk, int n8, unsigned short *__restrict__ dst, int Cd8, int d8) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nchunk; i += (int64_t)gridDim.x * 256) {
        const int64_t pix = i / n8;
        const int c = (int)(i - pix * n8);
        uint4 v = reinterpret_cast<const uint4 *>(src)[pix * Cs8 + s8 + c];
        if (add) {
            float x[8], y[8];
            unpack8_bf16(v, x);
            unpack8_bf16(reinterpret_cast<const uint4 *>(add)[pix * Ca8 + a8 + c], y);
#pragma unroll
            for (int j = 0; j < 8; ++j) x[j] += y[j];
            v = pack8_bf16(x);
        }
        reinterpret_cast<uint4 *>(dst)[pix * Cd8 + d8 + c] = v;
    }
}

namespace {
unsigned route_grid(int64_t nchunk) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv(nchunk, 256), 4096)); }

int pools_check(obb_ctx *ctx, const char *fn, int32_t B, int32_t H, int32_t W, int32_t C) {
    OBB_REQUIRE(ctx, ctx && C >= 8 && C % 8 == 0, "%s: C = %d must be a positive multiple of 8", fn, (int)C);
    OBB_REQUIRE(ctx, B >= 1 && H >= 1 && W >= 1, "%s: B = %d, H = %d, W = %d must be at least 1", fn, (int)B, (int)H, (int)W);
    OBB_REQUIRE(ctx, H <= kPoolMaxSide && W <= kPoolMaxSide, "%s: map %d x %d: the pools keep the whole map in LDS, H and W at most %d", fn, (int)H, (int)W,
                kPoolMaxSide);
    OBB_REQUIRE(ctx, (int64_t)B * cdiv(C / 8, pool_share(H, W)) < (1ll << 31), "%s: B = %d x C = %d: too many workgroups", fn, (int)B, (int)C);
    return OBB_OK;
}

int upcat_check(obb_ctx *ctx, const char *fn, int32_t B, int32_t H, int32_t W, int32_t Ca, int32_t Cb, int32_t up) {
    OBB_REQUIRE(ctx, ctx && Ca >= 8 && Ca % 8 == 0, "%s: Ca = %d must be a positive multiple of 8", fn, (int)Ca);
    OBB_REQUIRE(ctx, Cb >= 8 && Cb % 8 == 0, "%s: Cb = %d must be a positive multiple of 8", fn, (int)Cb);
    OBB_REQUIRE(ctx, B >= 1 && H >= 1 && W >= 1, "%s: B = %d, H = %d, W = %d must be at least 1", fn, (int)B, (int)H, (int)W);
    OBB_REQUIRE(ctx, up == 1 || up == 2, "%s: up = %d must be 1 or 2", fn, (int)up);
    OBB_REQUIRE(ctx, (int64_t)H * up < (1ll << 30) && (int64_t)W * up < (1ll << 30), "%s: H = %d, W = %d: map too large", fn, (int)H, (int)W);
    return OBB_OK;
}
}  // namespace

}  // namespace obb

using namespace obb;

extern "C" {

int obb_sppf_pools_fwd_bf16(obb_ctx *ctx, const uint16_t *x, int32_t B, int32_t H, int32_t W, int32_t C, uint16_t *cat, obb_stream_t s) {
    if (int rc = pools_check(ctx, "obb_sppf_pools_fwd_bf16", B, H, W, C)) return rc;
    OBB_REQUIRE(ctx, x && cat, "obb_sppf_pools_fwd_bf16: NULL buffer");
    const int share = pool_share(H, W), ngrp = (int)cdiv(C / 8, share);
    const size_t lds = (size_t)H * W * share * kPoolFwdBytes;
    hipLaunchKernelGGL(k_sppf_pools_fwd, dim3((unsigned)((int64_t)B * ngrp)), dim3(256), lds, (hipStream_t)s, x, (int)H, (int)W, (int)C, share, ngrp, cat);
    OBB_LAUNCH_CHECK(ctx);
    return OBB_OK;
}

int obb_sppf_pools_bwd_bf16(obb_ctx *ctx, const uint16_t *cat, const uint16_t *dcat, int32_t B, int32_t H, int32_t W, int32_t C, uint16_t *dx, obb_stream_t s) {
    if (int rc = pools_check(ctx, "obb_sppf_pools_bwd_bf16", B, H, W, C)) return rc;
    OBB_REQUIRE(ctx, cat && dcat && dx, "obb_sppf_pools_bwd_bf16: NULL buffer");
    OBB_HIP(ctx, allow_dyn_lds((const void *)k_sppf_pools_bwd, kPoolMaxElems * kPoolBwdBytes));  // more than 64 KiB of dynamic LDS
    const int share = pool_share(H, W), ngrp = (int)cdiv(C / 8, share);
    const size_t lds = (size_t)H * W * share * kPoolBwdBytes;
    hipLaunchKernelGGL(k_sppf_pools_bwd, dim3((unsigned)((int64_t)B * ngrp)), dim3(256), lds, (hipStream_t)s, cat, dcat, (int)H, (int)W, (int)C, share, ngrp, dx);
    OBB_LAUNCH_CHECK(ctx);
    return OBB_OK;
}

int obb_upcat_fwd_bf16(obb_ctx *ctx, const uint16_t *a, const uint16_t *b, int32_t B, int32_t H, int32_t W, int32_t Ca, int32_t Cb, int32_t up, uint16_t *out,
                       obb_stream_t s) {
    if (int rc = upcat_check(ctx, "obb_upcat_fwd_bf16", B, H, W, Ca, Cb, up)) return rc;
    OBB_REQUIRE(ctx, a && b && out, "obb_upcat_fwd_bf16: NULL buffer");
    const int64_t nchunk = (int64_t)B * H * up * W * up * ((Ca + Cb) / 8);
    hipLaunchKernelGGL(k_upcat_fwd, dim3(route_grid(nchunk)), dim3(256), 0, (hipStream_t)s, a, b, nchunk, (int)(H * up), (int)(W * up), (int)(Ca / 8), (int)(Cb / 8),
                       (int)up, out);
    OBB_LAUNCH_CHECK(ctx);
    return OBB_OK;
}

int obb_upcat_bwd_bf16(obb_ctx *ctx, const uint16_t *dout, int32_t B, int32_t H, int32_t W, int32_t Ca, int32_t Cb, int32_t up, uint16_t *da, uint16_t *db,
                       int32_t accum_a, int32_t accum_b, obb_stream_t s) {
    if (int rc = upcat_check(ctx, "obb_upcat_bwd_bf16", B, H, W, Ca, Cb, up)) return rc;
    OBB_REQUIRE(ctx, dout, "obb_upcat_bwd_bf16: NULL dout");
    const int64_t nA = da ? (int64_t)B * H * W * (Ca / 8) : 0, nB = db ? (int64_t)B * H * up * W * up * (Cb / 8) : 0;
    if (nA + nB == 0) return OBB_OK;
    hipLaunchKernelGGL(k_upcat_bwd, dim3(route_grid(nA + nB)), dim3(256), 0, (hipStream_t)s, dout, nA, nB, (int)H, (int)W, (int)(Ca / 8), (int)(Cb / 8), (int)up, da,
                       db, (int)(accum_a != 0), (int)(accum_b != 0));
    OBB_LAUNCH_CHECK(ctx);
    return OBB_OK;
}

int obb_add_bf16(obb_ctx *ctx, const uint16_t *a, const uint16_t *b, int64_t n, uint16_t *out, obb_stream_t s) {
    OBB_REQUIRE(ctx, ctx && n >= 8 && n % 8 == 0, "obb_add_bf16: n = %lld must be a positive multiple of 8", (long long)n);
    OBB_REQUIRE(ctx, a && b && out, "obb_add_bf16: NULL buffer");
    OBB_REQUIRE(ctx, ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(out)) & 15u) == 0,
                "obb_add_bf16: a, b and out must be 16-byte aligned");
    hipLaunchKernelGGL(k_add_bf16, dim3(route_grid(n / 8)), dim3(256), 0, (hipStream_t)s, a, b, n / 8, out);
    OBB_LAUNCH_CHECK(ctx);
    return OBB_OK;
}

int obb_chanwin_bf16(obb_ctx *ctx, const uint16_t *src, int32_t Cs, int32_t s0, const uint16_t *add, int32_t Ca, int32_t a0, int64_t npix, int32_t n,
                     uint16_t *dst, int32_t Cd, int32_t d0, obb_stream_t s) {
    const char *fn = "obb_chanwin_bf16";
    OBB_REQUIRE(ctx, ctx && n >= 8 && n % 8 == 0, "%s: n = %d must be a positive multiple of 8", fn, (int)n);
    OBB_REQUIRE(ctx, Cs >= 8 && Cs % 8 == 0 && Cd >= 8 && Cd % 8 == 0, "%s: Cs = %d, Cd = %d must be positive multiples of 8", fn, (int)Cs, (int)Cd);
    OBB_REQUIRE(ctx, s0 >= 0 && s0 % 8 == 0 && d0 >= 0 && d0 % 8 == 0, "%s: s0 = %d, d0 = %d must be multiples of 8, at least 0", fn, (int)s0, (int)d0);
    OBB_REQUIRE(ctx, (int64_t)s0 + n <= Cs, "%s: the window %d + %d runs past src's %d channels", fn, (int)s0, (int)n, (int)Cs);
    OBB_REQUIRE(ctx, (int64_t)d0 + n <= Cd, "%s: the window %d + %d runs past dst's %d channels", fn, (int)d0, (int)n, (int)Cd);
    OBB_REQUIRE(ctx, npix >= 1 && npix < (1ll << 40), "%s: npix = %lld must be at least 1 (and below 2^40)", fn, (long long)npix);
    OBB_REQUIRE(ctx, src && dst, "%s: NULL buffer", fn);
    OBB_REQUIRE(ctx, ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(add) | reinterpret_cast<uintptr_t>(dst)) & 15u) == 0,
                "%s: src, add and dst must be 16-byte aligned", fn);
    const uintptr_t d_lo = reinterpret_cast<uintptr_t>(dst), d_hi = d_lo + (uintptr_t)npix * Cd * 2;
    const uintptr_t s_lo = reinterpret_cast<uintptr_t>(src), s_hi = s_lo + (uintptr_t)npix * Cs * 2;
    OBB_REQUIRE(ctx, d_hi <= s_lo || s_hi <= d_lo, "%s: dst overlaps src", fn);
    if (add) {
        OBB_REQUIRE(ctx, Ca >= 8 && Ca % 8 == 0 && a0 >= 0 && a0 % 8 == 0, "%s: Ca = %d, a0 = %d must be multiples of 8, Ca at least 8, a0 at least 0", fn, (int)Ca,
                    (int)a0);
        OBB_REQUIRE(ctx, (int64_t)a0 + n <= Ca, "%s: the window %d + %d runs past add's %d channels", fn, (int)a0, (int)n, (int)Ca);
        const uintptr_t a_lo = reinterpret_cast<uintptr_t>(add), a_hi = a_lo + (uintptr_t)npix * Ca * 2;
        OBB_REQUIRE(ctx, d_hi <= a_lo || a_hi <= d_lo, "%s: dst overlaps add", fn);
    }
    const int64_t nchunk = npix * (n / 8);
    hipLaunchKernelGGL(k_chanwin, dim3(route_grid(nchunk)), dim3(256), 0, (hipStream_t)s, src, (int)(Cs / 8), (int)(s0 / 8), add, (int)(add ? Ca / 8 : 0),
                       (int)(add ? a0 / 8 : 0), nchunk, (int)(n / 8), dst, (int)(Cd / 8), (int)(d0 / 8));
    OBB_LAUNCH_CHECK(ctx);
    return OBB_OK;
}

}  // extern "C"
