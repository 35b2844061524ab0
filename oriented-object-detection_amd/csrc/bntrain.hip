// Training-mode BatchNorm2d + SiLU of the Ultralytics `Conv` block (Conv2d(bias=False) -> BatchNorm2d -> SiLU; SURVEY.md section 8 row f1,
// `model.train(...)`, Train_OBB.py:796-841), bf16 NHWC tensors of npix = B*H*W rows x C channels (C % 8 == 0), fp32 statistics.
//
//   forward   mean_c, var_c = batch mean / biased variance of z[:, c];  invstd_c = 1 / sqrt(var_c + eps)
//             running_mean = (1 - m) running_mean + m mean;  running_var = (1 - m) running_var + m var N / (N - 1)   (unbiased, as torch)
//             a = silu(gamma (z - mean) invstd + beta), rounded to bf16 once   (act = 0, obb_bn_fwd_bf16 / obb_bn_bwd_bf16: no SiLU, g = da)
//   backward  xhat = (z - mean) invstd, y = gamma xhat + beta recomputed from z (no normalised tensor is stored);  g = da silu'(y)
//             dbeta = sum g,  dgamma = sum g xhat,  dz = gamma invstd (g - dbeta / N - xhat dgamma / N), rounded to bf16 once
//
// Reductions (deterministic, no float atomics -- the two passes of traindev.h): the pixel dimension is split into nbx contiguous blocks, one
// workgroup per (pixel block, 256-channel group); a thread owns 8 channels (one 16-byte load per pixel) and every RP-th pixel of the block,
// its partial sums meet in LDS in lds_row_tree.  The per-block results go to an fp32 slab [nbx][C]; a second kernel combines the slab in
// slab_combine's order (64 strided walkers per channel, then their pairwise tree).
// The forward's slab holds (mean, M2) pairs of each block -- the block's mean first, then the sum of squares about it, read back from
// cache -- combined with Chan's parallel formula, so the variance never comes from E[z^2] - E[z]^2 (which cancels catastrophically when
// |mean| >> std).  Every statistic is taken of z - z[pixel 0] (per channel; exact in fp32): the block means and the deviations between them
// that Chan's formula squares are then of the size of std, not of |mean| -- without the shift, the fp32 spacing of a mean of 8 (4.8e-7) made
// the variance of a std-0.05 channel wrong by 3e-6 relative (k_bn_stats_final: slab_combine's walkers and tree with chan_add as the operator,
// written out).  The backward's slab holds plain sums.  Both directions share the geometry (bn_geo) and the LDS reduction (block_reduce8).
#include <algorithm>

#include "ctx.h"
#include "traindev.h"

namespace obb {
namespace {  // helpers; the kernels below keep plain obb:: names for the traces

// Work split of the partial-sum kernels: CW chunk columns x RP pixel rows of threads, nbx pixel blocks of PB pixels
struct BnGeo : RowSplit { int nbx; int64_t PB; };
BnGeo bn_geo(int64_t npix, int C) {
    BnGeo g;
    static_cast<RowSplit &>(g) = row_split(C);
    const int64_t want = std::max(1, 1024 / g.ny);  // ~1024 workgroups: four per CU
    const int64_t nbx = std::min<int64_t>(cdiv(npix, g.RP), want);
    g.PB = cdiv(cdiv(npix, nbx), g.RP) * g.RP;
    g.nbx = (int)cdiv(npix, g.PB);
    return g;
}

// Sums the 8 per-thread values s[] over the RP rows of the workgroup in the fixed pairwise tree (lds_row_tree); thread t < CW*8 gets channel
// chunk t / 8, lane t % 8.  (A serial walk over the rows was a 256-term fp32 chain at C = 8: 2e-6 of the variance of a mean-8, std-0.05
// channel.)  red: 256 * 8 floats of LDS.  Returns the sum for threads t < CW*8 (0 elsewhere).  Ends with every thread past a barrier.
__device__ __forceinline__ float block_reduce8(float *red, const float s[8], int row, int col, int CW, int RP) {
    float4 *r4 = reinterpret_cast<float4 *>(red + (row * CW + col) * 8);
    if (row < RP) {
        r4[0] = make_float4(s[0], s[1], s[2], s[3]);
        r4[1] = make_float4(s[4], s[5], s[6], s[7]);
    }
    lds_row_tree<8>(red, 0, row, col, CW, RP);
    const float t = (int)threadIdx.x < CW * 8 ? red[threadIdx.x] : 0.f;
    __syncthreads();
    return t;
}

// (n, mean, M2) <- (n, mean, M2) + (nb, mb, m2b): Chan, Golub & LeVeque's pairwise update
__device__ __forceinline__ void chan_add(float &n, float &mu, float &m2, float nb, float mb, float m2b) {
    if (nb == 0.f) return;
    if (n == 0.f) { n = nb; mu = mb; m2 = m2b; return; }
    const float nn = n + nb, d = mb - mu;
    mu += d * (nb / nn);
    m2 += m2b + d * d * (n * nb / nn);
    n = nn;
}

}  // namespace

// forward, pass 1: per pixel block the mean and the sum of squared deviations from it (M2), one (mean, M2) pair per channel into the slab
__global__ __launch_bounds__(256) void k_bn_stats_part(const unsigned short *__restrict__ z, int64_t npix, int C, int64_t PB, int CW, int RP,
                                                       float *__restrict__ slab_mean, float *__restrict__ slab_m2) {
    __shared__ __attribute__((aligned(16))) float red[256 * 8];
    __shared__ float bmean[kGroupChunks * 8];
    const int tid = threadIdx.x, col = tid % CW, row = tid / CW;
    const int C8 = C / 8, c8 = blockIdx.y * kGroupChunks + col;
    const bool act = row < RP && c8 < C8;
    const int64_t p0 = (int64_t)blockIdx.x * PB, p1 = min(p0 + PB, npix);
    const float inv_n = 1.0f / (float)(p1 - p0);
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, v[8], k[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (act) unpack8_bf16(*reinterpret_cast<const uint4 *>(z + c8 * 8), k);  // the shift: pixel 0's value
    if (act)
        for (int64_t p = p0 + row; p < p1; p += RP) {
            unpack8_bf16(*reinterpret_cast<const uint4 *>(z + p * C + c8 * 8), v);
#pragma unroll
            for (int j = 0; j < 8; ++j) s[j] += v[j] - k[j];
        }
    const float mu = block_reduce8(red, s, row, col, CW, RP) * inv_n;
    if (tid < CW * 8) bmean[tid] = mu;
    __syncthreads();
    float m[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { m[j] = bmean[col * 8 + j]; s[j] = 0.f; }
    if (act)  // the block was just read: this pass is served by the caches
        for (int64_t p = p0 + row; p < p1; p += RP) {
            unpack8_bf16(*reinterpret_cast<const uint4 *>(z + p * C + c8 * 8), v);
#pragma unroll
            for (int j = 0; j < 8; ++j) { const float d = (v[j] - k[j]) - m[j]; s[j] += d * d; }
        }
    const float m2 = block_reduce8(red, s, row, col, CW, RP);
    const int c = (blockIdx.y * kGroupChunks) * 8 + tid;
    if (tid < CW * 8 && c < C) { slab_mean[(size_t)blockIdx.x * C + c] = mu; slab_m2[(size_t)blockIdx.x * C + c] = m2; }
}

// forward, pass 2: combine the slab (walkers, then the tree) -> mean (shift added back), invstd; running statistics updated in place
__global__ __launch_bounds__(256) void k_bn_stats_final(const unsigned short *__restrict__ z, const float *__restrict__ slab_mean, const float *__restrict__ slab_m2, int nbx,
                                                        int64_t PB, int64_t npix, int C, float eps, float momentum, float *__restrict__ running_mean, float *__restrict__ running_var,
                                                        float *__restrict__ mean, float *__restrict__ invstd) {
    __shared__ float sn[kSlabWalkers][kSlabWalkEl], smu[kSlabWalkers][kSlabWalkEl], sm2[kSlabWalkers][kSlabWalkEl];
    const int cl = threadIdx.x % kSlabWalkEl, w = threadIdx.x / kSlabWalkEl, c = blockIdx.x * kSlabWalkEl + cl;
    float n = 0.f, mu = 0.f, m2 = 0.f;
    if (c < C)
        for (int b = w; b < nbx; b += kSlabWalkers)
            chan_add(n, mu, m2, (float)min(PB, npix - (int64_t)b * PB), slab_mean[(size_t)b * C + c], slab_m2[(size_t)b * C + c]);
    sn[w][cl] = n; smu[w][cl] = mu; sm2[w][cl] = m2;
    for (int st = kSlabWalkers / 2; st >= 1; st >>= 1) {
        __syncthreads();
        if (w < st) {
            chan_add(n, mu, m2, sn[w + st][cl], smu[w + st][cl], sm2[w + st][cl]);
            sn[w][cl] = n; smu[w][cl] = mu; sm2[w][cl] = m2;
        }
    }
    if (w != 0 || c >= C) return;
    const float N = (float)npix, var = m2 / N, mc = bf16_widen(z[c]) + mu;
    mean[c] = mc;
    invstd[c] = 1.0f / sqrtf(var + eps);
    running_mean[c] = (1.0f - momentum) * running_mean[c] + momentum * mc;
    running_var[c] = (1.0f - momentum) * running_var[c] + momentum * (m2 / (N - 1.0f));
}

// forward, pass 3: a = silu(gamma (z - mean) invstd + beta) (ACT; else the BatchNorm output itself), one 16-byte chunk per thread and step
template <bool ACT>
__global__ __launch_bounds__(256) void k_bn_silu_apply(const unsigned short *__restrict__ z, int64_t nchunk, int C8, const float *__restrict__ gamma,
                                                       const float *__restrict__ beta, const float *__restrict__ mean, const float *__restrict__ invstd,
                                                       unsigned short *__restrict__ a) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nchunk; i += (int64_t)gridDim.x * 256) {
        const int c0 = (int)(i % C8) * 8;
        float v[8];
        unpack8_bf16(reinterpret_cast<const uint4 *>(z)[i], v);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float y = gamma[c0 + j] * ((v[j] - mean[c0 + j]) * invstd[c0 + j]) + beta[c0 + j];
            v[j] = ACT ? silu_exact(y) : y;
        }
        reinterpret_cast<uint4 *>(a)[i] = pack8_bf16(v);
    }
}

// g = da silu'(y) (ACT; else g = da) and xhat of the 8 channels of one chunk
template <bool ACT>
__device__ __forceinline__ void bn_bwd_terms(const uint4 zv, const uint4 dav, const float ga[8], const float be[8], const float mu[8], const float is[8],
                                             float g[8], float xh[8]) {
    float zf[8], df[8];
    unpack8_bf16(zv, zf);
    unpack8_bf16(dav, df);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        xh[j] = (zf[j] - mu[j]) * is[j];
        g[j] = ACT ? df[j] * silu_grad_exact(ga[j] * xh[j] + be[j]) : df[j];
    }
}

// backward, pass 1: per pixel block sum g and sum g xhat into the slab
template <bool ACT>
__global__ __launch_bounds__(256) void k_bn_bwd_part(const unsigned short *__restrict__ z, const unsigned short *__restrict__ da, int64_t npix, int C, int64_t PB,
                                                     int CW, int RP, const float *__restrict__ gamma, const float *__restrict__ beta, const float *__restrict__ mean,
                                                     const float *__restrict__ invstd, float *__restrict__ slab_g, float *__restrict__ slab_gx) {
    __shared__ __attribute__((aligned(16))) float red[256 * 8];
    const int tid = threadIdx.x, col = tid % CW, row = tid / CW;
    const int C8 = C / 8, c8 = blockIdx.y * kGroupChunks + col;
    const bool act = row < RP && c8 < C8;
    const int64_t p0 = (int64_t)blockIdx.x * PB, p1 = min(p0 + PB, npix);
    float ga[8], be[8], mu[8], is[8], sg[8], sgx[8], g[8], xh[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int c = act ? c8 * 8 + j : 0;
        ga[j] = gamma[c]; be[j] = beta[c]; mu[j] = mean[c]; is[j] = invstd[c];
        sg[j] = 0.f; sgx[j] = 0.f;
    }
    if (act)
        for (int64_t p = p0 + row; p < p1; p += RP) {
            bn_bwd_terms<ACT>(*reinterpret_cast<const uint4 *>(z + p * C + c8 * 8), *reinterpret_cast<const uint4 *>(da + p * C + c8 * 8), ga, be, mu, is, g, xh);
#pragma unroll
            for (int j = 0; j < 8; ++j) { sg[j] += g[j]; sgx[j] += g[j] * xh[j]; }
        }
    const float tg = block_reduce8(red, sg, row, col, CW, RP);
    const float tgx = block_reduce8(red, sgx, row, col, CW, RP);
    const int c = (blockIdx.y * kGroupChunks) * 8 + tid;
    if (tid < CW * 8 && c < C) { slab_g[(size_t)blockIdx.x * C + c] = tg; slab_gx[(size_t)blockIdx.x * C + c] = tgx; }
}

// backward, pass 2: dbeta = sum of the slab rows of g, dgamma = the same of g xhat (walkers, then the tree)
__global__ __launch_bounds__(256) void k_bn_bwd_final(const float *__restrict__ slab_g, const float *__restrict__ slab_gx, int nbx, int C, float *__restrict__ dgamma,
                                                      float *__restrict__ dbeta) {
    const int c = slab_elem();
    float a[2];
    if (!slab_combine<2>({slab_g, slab_gx}, nbx, C, c, a)) return;
    dbeta[c] = a[0];
    dgamma[c] = a[1];
}

// backward, pass 3: dz = gamma invstd (g - dbeta / N - xhat dgamma / N)
template <bool ACT>
__global__ __launch_bounds__(256) void k_bn_bwd_apply(const unsigned short *__restrict__ z, const unsigned short *__restrict__ da, int64_t nchunk, int C8, float inv_n,
                                                      const float *__restrict__ gamma, const float *__restrict__ beta, const float *__restrict__ mean,
                                                      const float *__restrict__ invstd, const float *__restrict__ dgamma, const float *__restrict__ dbeta,
                                                      unsigned short *__restrict__ dz) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nchunk; i += (int64_t)gridDim.x * 256) {
        const int c0 = (int)(i % C8) * 8;
        float ga[8], be[8], mu[8], is[8], g[8], xh[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) { ga[j] = gamma[c0 + j]; be[j] = beta[c0 + j]; mu[j] = mean[c0 + j]; is[j] = invstd[c0 + j]; }
        bn_bwd_terms<ACT>(reinterpret_cast<const uint4 *>(z)[i], reinterpret_cast<const uint4 *>(da)[i], ga, be, mu, is, g, xh);
#pragma unroll
        for (int j = 0; j < 8; ++j) g[j] = ga[j] * is[j] * (g[j] - dbeta[c0 + j] * inv_n - xh[j] * (dgamma[c0 + j] * inv_n));
        reinterpret_cast<uint4 *>(dz)[i] = pack8_bf16(g);
    }
}

static unsigned elementwise_grid(int64_t nchunk) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv(nchunk, 256), 2048)); }

}  // namespace obb

using namespace obb;

// the bodies of the entry points; act: SiLU after the BatchNorm (the Conv block) or none (Conv(act=False)), a template flag of the kernels
static int bn_fwd_impl(obb_ctx *ctx, const char *fn, bool act, const uint16_t *z, int64_t npix, int32_t C, const float *gamma, const float *beta, float eps,
                       float momentum, float *running_mean, float *running_var, float *mean, float *invstd, uint16_t *a, obb_stream_t s) {
    OBB_REQUIRE(ctx, ctx && C > 0 && C % 8 == 0, "%s: C = %d must be a positive multiple of 8", fn, (int)C);
    OBB_REQUIRE(ctx, npix >= 2 && npix < (1ll << 31), "%s: npix = %lld: training statistics need 2 <= npix < 2^31", fn, (long long)npix);
    OBB_REQUIRE(ctx, eps > 0.f && momentum >= 0.f && momentum <= 1.f, "%s: bad eps / momentum", fn);
    OBB_REQUIRE(ctx, z && gamma && beta && running_mean && running_var && mean && invstd && a, "%s: NULL buffer", fn);
    hipStream_t st = (hipStream_t)s;
    const BnGeo g = bn_geo(npix, C);
    float *slab = (float *)ctx->workspace(WS_TRAIN_E, (size_t)2 * g.nbx * C * 4);
    if (!slab) return set_error(ctx, OBB_ERR_HIP, "%s: workspace allocation failed", fn);
    float *slab_m2 = slab + (size_t)g.nbx * C;
    hipLaunchKernelGGL(k_bn_stats_part, dim3((unsigned)g.nbx, (unsigned)g.ny), dim3(256), 0, st, z, npix, (int)C, g.PB, g.CW, g.RP, slab, slab_m2);
    hipLaunchKernelGGL(k_bn_stats_final, dim3((unsigned)cdiv(C, kSlabWalkEl)), dim3(256), 0, st, z, slab, slab_m2, g.nbx, g.PB, npix, (int)C, eps, momentum, running_mean,
                       running_var, mean, invstd);
    const int64_t nchunk = npix * g.C8;
    if (act)
        hipLaunchKernelGGL(k_bn_silu_apply<true>, dim3(elementwise_grid(nchunk)), dim3(256), 0, st, z, nchunk, g.C8, gamma, beta, mean, invstd, a);
    else
        hipLaunchKernelGGL(k_bn_silu_apply<false>, dim3(elementwise_grid(nchunk)), dim3(256), 0, st, z, nchunk, g.C8, gamma, beta, mean, invstd, a);
    OBB_LAUNCH_CHECK(ctx);
    return OBB_OK;
}

static int bn_bwd_impl(obb_ctx *ctx, const char *fn, bool act, const uint16_t *z, const uint16_t *da, int64_t npix, int32_t C, const float *gamma, const float *beta,
                       const float *mean, const float *invstd, float *dgamma, float *dbeta, uint16_t *dz, obb_stream_t s) {
    OBB_REQUIRE(ctx, ctx && C > 0 && C % 8 == 0, "%s: C = %d must be a positive multiple of 8", fn, (int)C);
    OBB_REQUIRE(ctx, npix >= 2 && npix < (1ll << 31), "%s: npix = %lld: training statistics need 2 <= npix < 2^31", fn, (long long)npix);
    OBB_REQUIRE(ctx, z && da && gamma && beta && mean && invstd && dgamma && dbeta && dz, "%s: NULL buffer", fn);
    hipStream_t st = (hipStream_t)s;
    const BnGeo g = bn_geo(npix, C);
    float *slab = (float *)ctx->workspace(WS_TRAIN_E, (size_t)2 * g.nbx * C * 4);
    if (!slab) return set_error(ctx, OBB_ERR_HIP, "%s: workspace allocation failed", fn);
    float *slab_gx = slab + (size_t)g.nbx * C;
    const dim3 pgrid((unsigned)g.nbx, (unsigned)g.ny);
    if (act)
        hipLaunchKernelGGL(k_bn_bwd_part<true>, pgrid, dim3(256), 0, st, z, da, npix, (int)C, g.PB, g.CW, g.RP, gamma, beta, mean, invstd, slab, slab_gx);
    else
        hipLaunchKernelGGL(k_bn_bwd_part<false>, pgrid, dim3(256), 0, st, z, da, npix, (int)C, g.PB, g.CW, g.RP, gamma, beta, mean, invstd, slab, slab_gx);
    hipLaunchKernelGGL(k_bn_bwd_final, dim3((unsigned)cdiv(C, kSlabWalkEl)), dim3(256), 0, st, slab, slab_gx, g.nbx, (int)C, dgamma, dbeta);
    const int64_t nchunk = npix * g.C8;
    const float inv_n = 1.0f / (float)npix;
    if (act)
        hipLaunchKernelGGL(k_bn_bwd_apply<true>, dim3(elementwise_grid(nchunk)), dim3(256), 0, st, z, da, nchunk, g.C8, inv_n, gamma, beta, mean, invstd, dgamma, dbeta, dz);
    else
        hipLaunchKernelGGL(k_bn_bwd_apply<false>, dim3(elementwise_grid(nchunk)), dim3(256), 0, st, z, da, nchunk, g.C8, inv_n, gamma, beta, mean, invstd, dgamma, dbeta, dz);
    OBB_LAUNCH_CHECK(ctx);
    return OBB_OK;
}

extern "C" {

int obb_bn_silu_fwd_bf16(obb_ctx *ctx, const uint16_t *z, int64_t npix, int32_t C, const float *gamma, const float *beta, float eps, float momentum,
                         float *running_mean, float *running_var, float *mean, float *invstd, uint16_t *a, obb_stream_t s) {
    return bn_fwd_impl(ctx, "obb_bn_silu_fwd_bf16", true, z, npix, C, gamma, beta, eps, momentum, running_mean, running_var, mean, invstd, a, s);
}

int obb_bn_silu_bwd_bf16(obb_ctx *ctx, const uint16_t *z, const uint16_t *da, int64_t npix, int32_t C, const float *gamma, const float *beta, const float *mean,
                         const float *invstd, float *dgamma, float *dbeta, uint16_t *dz, obb_stream_t s) {
    return bn_bwd_impl(ctx, "obb_bn_silu_bwd_bf16", true, z, da, npix, C, gamma, beta, mean, invstd, dgamma, dbeta, dz, s);
}

// act = 1: the two entry points above; act = 0: BatchNorm alone (Conv(act=False): C2PSA's attn.pe)
int obb_bn_fwd_bf16(obb_ctx *ctx, const uint16_t *z, int64_t npix, int32_t C, const float *gamma, const float *beta, float eps, float momentum, float *running_mean,
                    float *running_var, float *mean, float *invstd, uint16_t *a, int32_t act, obb_stream_t s) {
    OBB_REQUIRE(ctx, act == 0 || act == 1, "obb_bn_fwd_bf16: act = %d must be 0 (identity) or 1 (SiLU)", (int)act);
    return bn_fwd_impl(ctx, "obb_bn_fwd_bf16", act == 1, z, npix, C, gamma, beta, eps, momentum, running_mean, running_var, mean, invstd, a, s);
}

int obb_bn_bwd_bf16(obb_ctx *ctx, const uint16_t *z, const uint16_t *da, int64_t npix, int32_t C, const float *gamma, const float *beta, const float *mean,
                    const float *invstd, float *dgamma, float *dbeta, uint16_t *dz, int32_t act, obb_stream_t s) {
    OBB_REQUIRE(ctx, act == 0 || act == 1, "obb_bn_bwd_bf16: act = %d must be 0 (identity) or 1 (SiLU)", (int)act);
    return bn_bwd_impl(ctx, "obb_bn_bwd_bf16", act == 1, z, da, npix, C, gamma, beta, mean, invstd, dgamma, dbeta, dz, s);
}

}  // extern "C"
