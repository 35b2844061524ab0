// Training-step slice: what Ultralytics' trainer does between `loss.backward()` and the next forward besides the
// optimiser arithmetic itself (Train_OBB.py:796-841 -> BaseTrainer.optimizer_step / ModelEMA.update): the global gradient-norm clip, the step of
// all three parameter groups, gradient accumulation and the EMA of weights and BatchNorm running statistics.  A SEGMENT is one flat fp32 buffer
// (train.ParamGroups: three parameter groups and the buffer of running statistics); every kernel here covers up to kMaxSeg segments in ONE
// launch.  The segments travel by value in the kernel arguments (no pointer table in device memory); a workgroup finds its segment from the
// prefix of per-segment block counts.  Plain streaming kernels: float4 per lane with a scalar tail, no atomics, no fences; the clip coefficient
// is produced (k_clip_coef) and consumed (k_*_step_multi) on the device, so an update never reads back to the host.
#include "optim.h"

namespace obb {

constexpr int kMaxSeg = 8;
constexpr int kSlab = 4096;   // elements per workgroup of k_grad_sumsq: 256 lanes x 4 float4
constexpr int kBlk = 1024;    // elements per workgroup of the element-wise kernels: 256 lanes x 1 float4 (as optim.hip)

// NP pointers per segment (p[j][k]: pointer j of segment k), the lengths and the prefix ends of the segments' block ranges: segment k owns
// blocks [end[k - 1], end[k]); an empty segment owns none.  a / b / c: per-segment scalars (lr, weight decay and AdamW's step size).
template <int NP>
struct Segs {
    float *p[NP][kMaxSeg];
    int64_t n[kMaxSeg];
    uint32_t end[kMaxSeg];
    float a[kMaxSeg], b[kMaxSeg], c[kMaxSeg];
};

// arr[k] for a block-uniform k without a dynamic index into the kernel arguments: seven scalar selects
template <typename T>
__device__ __forceinline__ T pick(const T (&arr)[kMaxSeg], int k) {
    T r = arr[0];
#pragma unroll
    for (int j = 1; j < kMaxSeg; ++j)
        if (k == j) r = arr[j];
    return r;
}

// -> the segment of this workgroup; blk0 = its first block.  (Every launched block lies below end[kMaxSeg - 1], the grid size.)
__device__ __forceinline__ int seg_of(const uint32_t (&end)[kMaxSeg], uint32_t &blk0) {
    int k = 0;
    blk0 = 0;
#pragma unroll
    for (int j = 0; j < kMaxSeg - 1; ++j)
        if (blockIdx.x >= end[j]) {
            k = j + 1;
            blk0 = end[j];
        }
    return k;
}

// ---------------------------------------------------------------------------------------------- gradient norm
// One workgroup = one slab of kSlab consecutive elements of one segment -> partial[blockIdx.x] = the sum of their squares, every square and every
// sum in double (an fp32 value squared is exact in double, and neither 1e20^2 nor 1e-25^2 leaves its range).  Lane t adds its (up to) 16 elements
// in index order, then a fixed tree over the 256 lanes: the result depends on nothing but the data.
__global__ __launch_bounds__(256) void k_grad_sumsq(const Segs<1> S, double *__restrict__ partial) {
    __shared__ double red[256];
    uint32_t blk0;
    const int k = seg_of(S.end, blk0);
    const float *__restrict__ g = pick(S.p[0], k);
    const int64_t n = pick(S.n, k);
    const int64_t base = (int64_t)(blockIdx.x - blk0) * kSlab;
    double acc = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t i4 = base + ((int64_t)r * 256 + threadIdx.x) * 4;
        if (i4 + 4 <= n) {
            const float4 v = *reinterpret_cast<const float4 *>(g + i4);
            acc += (double)v.x * (double)v.x;
            acc += (double)v.y * (double)v.y;
            acc += (double)v.z * (double)v.z;
            acc += (double)v.w * (double)v.w;
        } else {
            for (int64_t i = i4; i < n; ++i) acc += (double)g[i] * (double)g[i];
        }
    }
    red[threadIdx.x] = acc;
    __syncthreads();
#pragma unroll
    for (int w = 128; w >= 1; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

// One workgroup: the partials summed in INDEX order in double (staged through LDS 1024 at a time, added by lane 0), total = sqrt(sum) ->
// clip[0] = total_norm, clip[1] = coef = min(1, max_norm / (total + 1e-6)), clip[2] = finite.  A NaN total gives a NaN coef and an infinite one 0
// (torch.nn.utils.clip_grad_norm_ with error_if_nonfinite=False: clamp passes NaN on).
__global__ __launch_bounds__(256) void k_clip_coef(const double *__restrict__ partial, int64_t np, double max_norm, float *__restrict__ clip) {
    __shared__ double stage[1024];
    double sum = 0.0;
    for (int64_t o = 0; o < np; o += 1024) {
        const int m = (int)(np - o < 1024 ? np - o : 1024);
        for (int i = threadIdx.x; i < m; i += 256) stage[i] = partial[o + i];
        __syncthreads();
        if (threadIdx.x == 0)
            for (int i = 0; i < m; ++i) sum += stage[i];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double total = sqrt(sum);
        double c = max_norm / (total + 1e-6);
        if (c > 1.0) c = 1.0;  // (false for NaN: it stays)
        clip[0] = (float)total;
        clip[1] = (float)c;
        clip[2] = isfinite(total) ? 1.0f : 0.0f;
    }
}

// ---------------------------------------------------------------------------------------------- optimiser step of all groups
// g' = g * coef (ONE fp32 multiply; clip == NULL: none), then sgd_one / adamw_one of optim.h: with coef == 1.0f or no clip the result is bit-identical
// to k_sgd_step / k_adamw_step run per group.  Per segment: a = lr, b = weight decay.  The gradient buffer is only read.
__global__ __launch_bounds__(256) void k_sgd_step_multi(const Segs<3> S, float mu, int nesterov, int first, const float *__restrict__ clip) {
    uint32_t blk0;
    const int k = seg_of(S.end, blk0);
    float *__restrict__ p = pick(S.p[0], k);
    const float *__restrict__ g = pick(S.p[1], k);
    float *__restrict__ buf = pick(S.p[2], k);
    const int64_t n = pick(S.n, k);
    const float lr = pick(S.a, k), wd = pick(S.b, k);
    const int64_t i4 = ((int64_t)(blockIdx.x - blk0) * 256 + threadIdx.x) * 4;
    if (i4 >= n) return;
    const bool scale = clip != nullptr;
    const float coef = scale ? clip[1] : 1.0f;
    const bool rd = !first && mu != 0.f;
    if (i4 + 4 <= n) {
        float4 pv = *reinterpret_cast<const float4 *>(p + i4);
        float4 gv = *reinterpret_cast<const float4 *>(g + i4);
        float4 bv = rd ? *reinterpret_cast<const float4 *>(buf + i4) : make_float4(0.f, 0.f, 0.f, 0.f);
        if (scale) gv = make_float4(gv.x * coef, gv.y * coef, gv.z * coef, gv.w * coef);
        sgd_one(pv.x, gv.x, bv.x, lr, mu, wd, nesterov, first);
        sgd_one(pv.y, gv.y, bv.y, lr, mu, wd, nesterov, first);
        sgd_one(pv.z, gv.z, bv.z, lr, mu, wd, nesterov, first);
        sgd_one(pv.w, gv.w, bv.w, lr, mu, wd, nesterov, first);
        *reinterpret_cast<float4 *>(p + i4) = pv;
        if (mu != 0.f) *reinterpret_cast<float4 *>(buf + i4) = bv;
        return;
    }
    for (int64_t i = i4; i < n; ++i) {
        float b = rd ? buf[i] : 0.f;
        sgd_one(p[i], scale ? g[i] * coef : g[i], b, lr, mu, wd, nesterov, first);
        if (mu != 0.f) buf[i] = b;
    }
}

// Per segment: a = lr, b = weight decay, c = the bias-corrected step size of its lr (from the host, as obb_adamw_step computes it).
__global__ __launch_bounds__(256) void k_adamw_step_multi(const Segs<4> S, float omb1, float b2, float omb2, float eps, float sqrt_bc2,
                                                         const float *__restrict__ clip) {
    uint32_t blk0;
    const int k = seg_of(S.end, blk0);
    float *__restrict__ p = pick(S.p[0], k);
    const float *__restrict__ g = pick(S.p[1], k);
    float *__restrict__ m = pick(S.p[2], k);
    float *__restrict__ v = pick(S.p[3], k);
    const int64_t n = pick(S.n, k);
    const float lr = pick(S.a, k), wd = pick(S.b, k), step_size = pick(S.c, k);
    const int64_t i4 = ((int64_t)(blockIdx.x - blk0) * 256 + threadIdx.x) * 4;
    if (i4 >= n) return;
    const bool scale = clip != nullptr;
    const float coef = scale ? clip[1] : 1.0f;
    if (i4 + 4 <= n) {
        float4 pv = *reinterpret_cast<const float4 *>(p + i4), mv = *reinterpret_cast<const float4 *>(m + i4), vv = *reinterpret_cast<const float4 *>(v + i4);
        float4 gv = *reinterpret_cast<const float4 *>(g + i4);
        if (scale) gv = make_float4(gv.x * coef, gv.y * coef, gv.z * coef, gv.w * coef);
        adamw_one(pv.x, gv.x, mv.x, vv.x, lr, omb1, b2, omb2, eps, wd, step_size, sqrt_bc2);
        adamw_one(pv.y, gv.y, mv.y, vv.y, lr, omb1, b2, omb2, eps, wd, step_size, sqrt_bc2);
        adamw_one(pv.z, gv.z, mv.z, vv.z, lr, omb1, b2, omb2, eps, wd, step_size, sqrt_bc2);
        adamw_one(pv.w, gv.w, mv.w, vv.w, lr, omb1, b2, omb2, eps, wd, step_size, sqrt_bc2);
        *reinterpret_cast<float4 *>(p + i4) = pv;
        *reinterpret_cast<float4 *>(m + i4) = mv;
        *reinterpret_cast<float4 *>(v + i4) = vv;
        return;
    }
    for (int64_t i = i4; i < n; ++i) adamw_one(p[i], scale ? g[i] * coef : g[i], m[i], v[i], lr, omb1, b2, omb2, eps, wd, step_size, sqrt_bc2);
}

// ---------------------------------------------------------------------------------------------- accumulation and EMA
// acc = first ? g : acc + g  (`first`: acc is not read, so it needs no zero fill)
__global__ __launch_bounds__(256) void k_grad_accumulate(const Segs<2> S, int first) {
    uint32_t blk0;
    const int k = seg_of(S.end, blk0);
    float *__restrict__ acc = pick(S.p[0], k);
    const float *__restrict__ g = pick(S.p[1], k);
    const int64_t n = pick(S.n, k);
    const int64_t i4 = ((int64_t)(blockIdx.x - blk0) * 256 + threadIdx.x) * 4;
    if (i4 >= n) return;
    if (i4 + 4 <= n) {
        float4 gv = *reinterpret_cast<const float4 *>(g + i4);
        if (!first) {
            const float4 av = *reinterpret_cast<const float4 *>(acc + i4);
            gv = make_float4(av.x + gv.x, av.y + gv.y, av.z + gv.z, av.w + gv.w);
        }
        *reinterpret_cast<float4 *>(acc + i4) = gv;
        return;
    }
    for (int64_t i = i4; i < n; ++i) acc[i] = first ? g[i] : acc[i] + g[i];
}

// ultralytics ModelEMA.update per element, in torch's order: v.mul_(d); v.add_((1 - d) * s) -- three fp32 roundings.  d and omd = 1 - d each arrive
// rounded from double (1.0f - (float)d is 6e-4 off in relative terms at d = 0.9999: cf. omb1 / omb2 in optim.h).
__device__ __forceinline__ float ema_one(float e, float s, float d, float omd) {
    e = e * d;
    return e + omd * s;
}

__global__ __launch_bounds__(256) void k_ema_update(const Segs<2> S, float d, float omd) {
    uint32_t blk0;
    const int k = seg_of(S.end, blk0);
    float *__restrict__ e = pick(S.p[0], k);
    const float *__restrict__ s = pick(S.p[1], k);
    const int64_t n = pick(S.n, k);
    const int64_t i4 = ((int64_t)(blockIdx.x - blk0) * 256 + threadIdx.x) * 4;
    if (i4 >= n) return;
    if (i4 + 4 <= n) {
        const float4 ev = *reinterpret_cast<const float4 *>(e + i4), sv = *reinterpret_cast<const float4 *>(s + i4);
        *reinterpret_cast<float4 *>(e + i4) = make_float4(ema_one(ev.x, sv.x, d, omd), ema_one(ev.y, sv.y, d, omd), ema_one(ev.z, sv.z, d, omd), ema_one(ev.w, sv.w, d, omd));
        return;
    }
    for (int64_t i = i4; i < n; ++i) e[i] = ema_one(e[i], s[i], d, omd);
}

// ---------------------------------------------------------------------------------------------- host: the segment table of a launch
// ptrs[j][k]: pointer j of segment k (NP host arrays of nseg device pointers).  Checks every non-empty segment (non-NULL unless `optional[j]`,
// 16-byte aligned) and fills the table; *blocks = the grid size (0: nothing to launch).  Unused entries keep n = 0 and the last prefix end.
template <int NP>
static int fill_segs(obb_ctx *ctx, const char *fn, Segs<NP> &S, const void *const *const (&ptrs)[NP], const bool (&optional)[NP], const int64_t *n, int32_t nseg, int per_block,
                     int64_t *blocks) {
    OBB_REQUIRE(ctx, ctx && nseg >= 0 && nseg <= kMaxSeg && (nseg == 0 || n), "%s: bad arguments (at most %d segments)", fn, kMaxSeg);
    for (int j = 0; j < NP; ++j) OBB_REQUIRE(ctx, nseg == 0 || ptrs[j], "%s: NULL pointer array", fn);
    int64_t end = 0;
    for (int k = 0; k < kMaxSeg; ++k) {
        const int64_t nk = k < nseg ? n[k] : 0;
        OBB_REQUIRE(ctx, nk >= 0, "%s: segment %d: negative length", fn, k);
        for (int j = 0; j < NP; ++j) {
            void *q = (k < nseg && nk > 0) ? const_cast<void *>(ptrs[j][k]) : nullptr;
            OBB_REQUIRE(ctx, nk == 0 || q || optional[j], "%s: segment %d: NULL buffer", fn, k);
            OBB_REQUIRE(ctx, (uintptr_t)q % 16 == 0, "%s: segment %d: buffers must be 16-byte aligned", fn, k);
            S.p[j][k] = (float *)q;
        }
        S.n[k] = nk;
        end += cdiv(nk, per_block);
        OBB_REQUIRE(ctx, end < (1ll << 31), "%s: too many elements", fn);
        S.end[k] = (uint32_t)end;
        S.a[k] = S.b[k] = S.c[k] = 0.f;
    }
    *blocks = end;
    return OBB_OK;
}

}  // namespace obb

using namespace obb;

extern "C" {

int obb_grad_sumsq_partials(const int64_t *n, int32_t nseg, int64_t *count) {
    if (!count || nseg < 0 || nseg > kMaxSeg || (nseg && !n)) return OBB_ERR_INVALID;
    int64_t c = 0;
    for (int k = 0; k < nseg; ++k) {
        if (n[k] < 0) return OBB_ERR_INVALID;
        c += cdiv(n[k], kSlab);
    }
    *count = c;
    return OBB_OK;
}

int obb_grad_sumsq(obb_ctx *ctx, const float *const *grad, const int64_t *n, int32_t nseg, double *partials, int64_t partials_cap, obb_stream_t s) {
    Segs<1> S;
    int64_t nb;
    const void *const *const ptrs[1] = {(const void *const *)grad};
    const bool opt[1] = {false};
    if (int rc = fill_segs<1>(ctx, "obb_grad_sumsq", S, ptrs, opt, n, nseg, kSlab, &nb)) return rc;
    OBB_REQUIRE(ctx, partials_cap >= nb, "obb_grad_sumsq: the workspace holds %lld partials, %lld needed", (long long)partials_cap, (long long)nb);
    if (nb == 0) return OBB_OK;
    OBB_REQUIRE(ctx, partials && (uintptr_t)partials % 8 == 0, "obb_grad_sumsq: NULL or misaligned workspace");
    hipLaunchKernelGGL(k_grad_sumsq, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)s, S, partials);
    OBB_HIP(ctx, hipGetLastError());
    return OBB_OK;
}

int obb_clip_coef(obb_ctx *ctx, const double *partials, int64_t npartials, double max_norm, float *clip, obb_stream_t s) {
    OBB_REQUIRE(ctx, ctx && npartials >= 0 && clip && (npartials == 0 || partials), "obb_clip_coef: bad arguments");
    OBB_REQUIRE(ctx, (uintptr_t)partials % 8 == 0 && (uintptr_t)clip % 4 == 0, "obb_clip_coef: misaligned buffer");
    hipLaunchKernelGGL(k_clip_coef, dim3(1), dim3(256), 0, (hipStream_t)s, partials, npartials, max_norm, clip);
    OBB_HIP(ctx, hipGetLastError());
    return OBB_OK;
}

int obb_sgd_step_multi(obb_ctx *ctx, float *const *param, const float *const *grad, float *const *momentum_buf, const int64_t *n, const float *lr,
                       const float *weight_decay, int32_t nseg, float momentum, int32_t nesterov, int32_t first_step, const float *clip, obb_stream_t s) {
    Segs<3> S;
    int64_t nb;
    OBB_REQUIRE(ctx, ctx && (nseg == 0 || (lr && weight_decay)), "obb_sgd_step_multi: bad arguments");
    OBB_REQUIRE(ctx, !(nesterov && momentum <= 0.f), "obb_sgd_step_multi: nesterov needs a momentum (as torch.optim.SGD)");
    OBB_REQUIRE(ctx, momentum == 0.f || momentum_buf || nseg == 0, "obb_sgd_step_multi: NULL buffer");
    static float *const none[kMaxSeg] = {};
    const void *const *const ptrs[3] = {(const void *const *)param, (const void *const *)grad, (const void *const *)(momentum_buf ? momentum_buf : none)};
    const bool opt[3] = {false, false, momentum == 0.f};
    if (int rc = fill_segs<3>(ctx, "obb_sgd_step_multi", S, ptrs, opt, n, nseg, kBlk, &nb)) return rc;
    if (nb == 0) return OBB_OK;
    OBB_REQUIRE(ctx, (uintptr_t)clip % 4 == 0, "obb_sgd_step_multi: misaligned clip");
    for (int k = 0; k < nseg; ++k) S.a[k] = lr[k], S.b[k] = weight_decay[k];
    hipLaunchKernelGGL(k_sgd_step_multi, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)s, S, momentum, nesterov, first_step, clip);
    OBB_HIP(ctx, hipGetLastError());
    return OBB_OK;
}

int obb_adamw_step_multi(obb_ctx *ctx, float *const *param, const float *const *grad, float *const *exp_avg, float *const *exp_avg_sq, const int64_t *n,
                         const float *lr, const float *weight_decay, int32_t nseg, int64_t step, double beta1, double beta2, float eps, const float *clip,
                         obb_stream_t s) {
    Segs<4> S;
    int64_t nb;
    OBB_REQUIRE(ctx, ctx && step >= 1 && (nseg == 0 || (lr && weight_decay)), "obb_adamw_step_multi: bad arguments (step counts from 1)");
    const void *const *const ptrs[4] = {(const void *const *)param, (const void *const *)grad, (const void *const *)exp_avg, (const void *const *)exp_avg_sq};
    const bool opt[4] = {false, false, false, false};
    if (int rc = fill_segs<4>(ctx, "obb_adamw_step_multi", S, ptrs, opt, n, nseg, kBlk, &nb)) return rc;
    if (nb == 0) return OBB_OK;
    OBB_REQUIRE(ctx, (uintptr_t)clip % 4 == 0, "obb_adamw_step_multi: misaligned clip");
    const AdamwConsts c = adamw_consts(beta1, beta2, step);
    for (int k = 0; k < nseg; ++k) S.a[k] = lr[k], S.b[k] = weight_decay[k], S.c[k] = c.step_size(lr[k]);
    hipLaunchKernelGGL(k_adamw_step_multi, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)s, S, c.omb1, c.b2, c.omb2, eps, c.sqrt_bc2, clip);
    OBB_HIP(ctx, hipGetLastError());
    return OBB_OK;
}

int obb_grad_accumulate(obb_ctx *ctx, float *const *acc, const float *const *grad, const int64_t *n, int32_t nseg, int32_t first, obb_stream_t s) {
    Segs<2> S;
    int64_t nb;
    const void *const *const ptrs[2] = {(const void *const *)acc, (const void *const *)grad};
    const bool opt[2] = {false, false};
    if (int rc = fill_segs<2>(ctx, "obb_grad_accumulate", S, ptrs, opt, n, nseg, kBlk, &nb)) return rc;
    if (nb == 0) return OBB_OK;
    hipLaunchKernelGGL(k_grad_accumulate, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)s, S, first);
    OBB_HIP(ctx, hipGetLastError());
    return OBB_OK;
}

int obb_ema_update(obb_ctx *ctx, float *const *ema, const float *const *src, const int64_t *n, int32_t nseg, double decay, obb_stream_t s) {
    Segs<2> S;
    int64_t nb;
    const void *const *const ptrs[2] = {(const void *const *)ema, (const void *const *)src};
    const bool opt[2] = {false, false};
    if (int rc = fill_segs<2>(ctx, "obb_ema_update", S, ptrs, opt, n, nseg, kBlk, &nb)) return rc;
    if (nb == 0) return OBB_OK;
    hipLaunchKernelGGL(k_ema_update, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)s, S, (float)decay, (float)(1.0 - decay));
    OBB_HIP(ctx, hipGetLastError());
    return OBB_OK;
}

}  // extern "C"
