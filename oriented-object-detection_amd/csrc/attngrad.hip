// Softmax attention core of C2PSA in training mode (`model.train(...)`, Train_OBB.py:796-841 -> ultralytics
// Attention(dim, num_heads, attn_ratio = 0.5), yolo11 model 10): a forward that keeps what a backward needs, and that backward.  The inference
// kernels (nnops.hip k_attention*) are untouched; the forward here has k_attention_mfma<false>'s structure.
//
//   layout      nnops.hip's: qkv bf16 [B][N][nh * 128], per token [q: nh * 32 | k: nh * 32 | v: nh * 64]; out, dout, dv_add bf16 [B][N][nh * 64];
//               lse fp32 [B][nh][N]; dqkv like qkv.  key_dim 32, head_dim 64, 1 <= N <= 192, scale = (float)(1 / sqrt(32.0)).
//   forward     S = scale q k^T, P = softmax over keys, out = P v, lse[q] = max_k S + log(sum_k exp(S - max)): the only thing kept.
//   backward    P = exp(S - lse) recomputed; dV = P^T dO (+ dv_add), dP = dO V^T, D[q] = sum_d dO O, dS = P o (dP - D), dQ = scale dS K,
//               dK = scale dS^T Q.
//   MFMA        v_mfma_f32_16x16x32_bf16: lane l holds A[row l & 15][k = 8 (l >> 4) + j], B[k = 8 (l >> 4) + j][col l & 15], j = 0..7, and
//               D[row 4 (l >> 4) + r][col l & 15], r = 0..3.  Every score product is computed TRANSPOSED to what its consumer contracts over, so
//               that the 4 x 2 values a lane holds after two 16-row blocks ARE the B operand of the next product (k index 8 g + j <-> row
//               32 st + 16 (j >> 2) + 4 g + (j & 3)); the other operand of that product is staged in LDS in that same order ("fragments").
//   ownership   every output row has ONE owner, no sum crosses a wave: a dQ row belongs to the wave that owns its 16-query block and walks all keys;
//               a dK / dV row to the wave that owns its 16-key block and walks all queries (S and dP are recomputed there: two MFMAs and three
//               at N <= 192).  No atomics, no workspace: bit-reproducible.
//   grid        forward (B nh, ceil(nkb / 4)), backward (B nh, 2 ceil(nkb / 4)), nkb = ceil(N / 16): 4 waves per workgroup, a wave owns one block.
//               The first half of the backward's y range are dQ workgroups, the second half dK / dV workgroups.
//   resident    forward: K rows (80-B pitch) and V^T fragments.  dQ workgroup: K rows, V rows (144-B pitch), K^T fragments, D.  dK / dV
//               workgroup: Q rows, dO rows, Q^T and dO^T fragments, D, lse.  Pitches of 80 and 144 B (odd multiples of 16) make the 16-byte row
//               reads of 16 consecutive rows land on 16 distinct 16-B slots.  At N = 192: 39 / 54.75 / 79.5 KiB.
//   rounding    inputs are bf16 values, products exact in fp32, sums fp32 (MFMA accumulators), exp and log are v_exp_f32 / v_log_f32 on
//               arguments scaled by fp32 log2(e) / ln(2).  P and dS enter their MFMA SPLIT into hi + lo bf16 parts (two MFMAs; what is lost
//               is 2^-16 relative), as in the inference core.  One bf16 rounding at each bf16 store; dv_add is added in fp32 before it.
//   padding     N is padded to 16-row blocks and 32-row steps.  Every staged row past N is ZERO (rows and fragments alike: 0 x garbage would
//               be NaN), every direct load past N is zero-filled, never read.  A padded KEY gets P = dS = 0 in the dQ walk; a padded QUERY gets
//               P = dS = 0 in the dK / dV walk (there it would be ADDED into real rows); padded rows of the owner block are not stored.
#include <cmath>

#include "ctx.h"
#include "halfx.h"
#include "launchcfg.h"

namespace obb {
namespace {

constexpr int kAtKD = 32, kAtHD = 64, kAtMaxN = 192;
constexpr int kAtKPitch = 80, kAtVPitch = 144;  // bytes per staged row of 32 / 64 bf16
constexpr float kLog2e = 1.44269504088896340736f, kLn2 = 0.69314718055994530942f;

typedef HX<false>::vec8 bf8;
typedef HX<false>::elem bfe;
typedef __attribute__((ext_vector_type(4))) float f32x4;

__device__ __forceinline__ float at_exp(float x) { return __builtin_amdgcn_exp2f(x * kLog2e); }
__device__ __forceinline__ float at_log(float x) { return __builtin_amdgcn_logf(x) * kLn2; }
__device__ __forceinline__ bf8 at_zero8() {
    const uint4 z = make_uint4(0, 0, 0, 0);
    return *reinterpret_cast<const bf8 *>(&z);
}
__device__ __forceinline__ bf8 at_ld8(const unsigned short *p, bool ok) { return ok ? *reinterpret_cast<const bf8 *>(p) : at_zero8(); }
__device__ __forceinline__ f32x4 at_mfma(bf8 a, bf8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
// x = hi + lo up to 2^-16 |x|
__device__ __forceinline__ void at_split(float x, bfe &hi, bfe &lo) {
    hi = (bfe)x;
    lo = (bfe)(x - (float)hi);
}

// rows [0, rows_pad) of `src` (row stride `rs` elements, CH 16-byte chunks per row) -> LDS rows of `pitch` bytes; rows >= N are zeros
template <int CH>
__device__ __forceinline__ void at_stage_rows(char *dst, int pitch, const unsigned short *src, int rs, int N, int rows_pad, int tid) {
    for (int i = tid; i < rows_pad * CH; i += 256) {
        const int t = i / CH, c = i - t * CH;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (t < N) v = *reinterpret_cast<const uint4 *>(src + (size_t)t * rs + c * 8);
        *reinterpret_cast<uint4 *>(dst + t * pitch + c * 16) = v;
    }
}
// the same rows TRANSPOSED into A-operand fragments [step][CH / 2][64 lanes][16 B]: element (row t, column d) is element j of lane
// kg * 16 + (d & 15) of fragment (t >> 5, d >> 4), j = ((t >> 4) & 1) * 4 + (t & 3), kg = (t & 15) >> 2; rows >= N are zeros
template <int CH>
__device__ __forceinline__ void at_stage_frags(char *dst, const unsigned short *src, int rs, int N, int rows_pad, int tid) {
    for (int i = tid; i < rows_pad * CH; i += 256) {
        const int t = i / CH, c = i - t * CH;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (t < N) v = *reinterpret_cast<const uint4 *>(src + (size_t)t * rs + c * 8);
        const int st = t >> 5, j = ((t >> 4) & 1) * 4 + (t & 3), kg = (t & 15) >> 2;
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int d = c * 8 + e;
            const unsigned short hv = (unsigned short)(e & 1 ? w[e >> 1] >> 16 : w[e >> 1] & 0xffffu);
            *reinterpret_cast<unsigned short *>(dst + ((st * (CH / 2) + (d >> 4)) * 64 + kg * 16 + (d & 15)) * 16 + j * 2) = hv;
        }
    }
}
// D[q] = sum_d dO[q][d] O[q][d] for q < rows_pad (0 past N): four lanes per query, 16 products each in index order, then (p0 + p1) + (p2 + p3)
__device__ __forceinline__ void at_stage_D(float *sD, const unsigned short *dO, const unsigned short *O, int rs, int N, int rows_pad, int tid) {
    for (int i = tid; i < rows_pad * 4; i += 256) {  // rows_pad * 4 is a multiple of 64: whole waves
        const int q = i >> 2, part = i & 3;
        float a = 0.f;
        if (q < N) {
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                float f[8], o[8];
                unpack8<false>(*reinterpret_cast<const uint4 *>(dO + (size_t)q * rs + part * 16 + c * 8), f);
                unpack8<false>(*reinterpret_cast<const uint4 *>(O + (size_t)q * rs + part * 16 + c * 8), o);
#pragma unroll
                for (int e = 0; e < 8; ++e) a += f[e] * o[e];
            }
        }
        a += __shfl_xor(a, 1);
        a += __shfl_xor(a, 2);
        if (part == 0) sD[q] = a;
    }
}

}  // namespace

// grid (B * nh, ceil(nkb / 4)); LDS: [nks * 32 K rows of 80 B][nks * 4 V^T fragments of 1 KiB]
__global__ __launch_bounds__(256) void k_attn_fwd(const unsigned short *__restrict__ qkv, int N, int nh, float scale, unsigned short *__restrict__ out,
                                                  float *__restrict__ lse) {
    constexpr int KD = kAtKD, HD = kAtHD, MAXKB = kAtMaxN / 16;
    extern __shared__ __attribute__((aligned(16))) char at_sm[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, pl = lane & 15;
    const int nkb = (N + 15) >> 4, nks = (nkb + 1) >> 1, C3 = nh * (2 * KD + HD), Co = nh * HD;
    const int b = blockIdx.x / nh, h = blockIdx.x % nh;
    char *sK = at_sm, *sVt = at_sm + nks * 32 * kAtKPitch;
    const unsigned short *base = qkv + (size_t)b * N * C3;
    at_stage_rows<KD / 8>(sK, kAtKPitch, base + nh * KD + h * KD, C3, N, nks * 32, tid);
    at_stage_frags<HD / 8>(sVt, base + 2 * nh * KD + h * HD, C3, N, nks * 32, tid);
    __syncthreads();
    const int qb = blockIdx.y * 4 + wave;
    if (qb >= nkb) return;
    const int q = qb * 16 + pl;
    const bf8 qf = at_ld8(base + (size_t)q * C3 + h * KD + g * 8, q < N);
    f32x4 s[MAXKB];
    float mx = -INFINITY;
#pragma unroll
    for (int jb = 0; jb < MAXKB; ++jb) {
        if (jb < nkb) s[jb] = at_mfma(*reinterpret_cast<const bf8 *>(sK + (jb * 16 + pl) * kAtKPitch + g * 16), qf, f32x4{0.f, 0.f, 0.f, 0.f});
        else s[jb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float v = (jb * 16 + g * 4 + r < N) ? s[jb][r] * scale : -INFINITY;
            s[jb][r] = v;
            mx = fmaxf(mx, v);
        }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    float den = 0.f;
    f32x4 acc[HD / 16];
#pragma unroll
    for (int db = 0; db < HD / 16; ++db) acc[db] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int st = 0; st < MAXKB / 2; ++st) {
        if (st >= nks) break;
        bf8 phi, plo;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float p = at_exp(s[2 * st + (j >> 2)][j & 3] - mx);  // exp2(-inf) = 0 for the padded keys
            den += p;
            bfe hi, lo;
            at_split(p, hi, lo);
            phi[j] = hi;
            plo[j] = lo;
        }
#pragma unroll
        for (int db = 0; db < HD / 16; ++db) {
            const bf8 vf = *reinterpret_cast<const bf8 *>(sVt + ((st * (HD / 16) + db) * 64 + lane) * 16);
            acc[db] = at_mfma(vf, phi, acc[db]);
            acc[db] = at_mfma(vf, plo, acc[db]);
        }
    }
    den += __shfl_xor(den, 16);
    den += __shfl_xor(den, 32);
    if (q >= N) return;
    const float inv = 1.0f / den;
    unsigned short *op = out + ((size_t)b * N + q) * Co + h * HD + g * 4;
#pragma unroll
    for (int db = 0; db < HD / 16; ++db) {
        uint2 o;
        o.x = HX<false>::pack2(acc[db][0] * inv, acc[db][1] * inv);
        o.y = HX<false>::pack2(acc[db][2] * inv, acc[db][3] * inv);
        *reinterpret_cast<uint2 *>(op + db * 16) = o;
    }
    if (g == 0) lse[((size_t)b * nh + h) * N + q] = mx + at_log(den);
}

// grid (B * nh, 2 * nyq), nyq = ceil(nkb / 4): blockIdx.y < nyq owns dQ blocks, the rest own dK / dV blocks.
// LDS, R = nks * 32 rows, F = nks KiB:  dQ: [K rows R x 80][V rows R x 144][K^T 2 F][D R floats]
//                                       dK / dV: [Q rows R x 80][dO rows R x 144][Q^T 2 F][dO^T 4 F][D R floats][lse R floats]
__global__ __launch_bounds__(256) void k_attn_bwd(const unsigned short *__restrict__ qkv, const unsigned short *__restrict__ o, const float *__restrict__ lse,
                                                  const unsigned short *__restrict__ dout, const unsigned short *__restrict__ dv_add, int N, int nh, float scale,
                                                  unsigned short *__restrict__ dqkv) {
    constexpr int KD = kAtKD, HD = kAtHD;
    extern __shared__ __attribute__((aligned(16))) char at_sm[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, pl = lane & 15;
    const int nkb = (N + 15) >> 4, nks = (nkb + 1) >> 1, R = nks * 32, C3 = nh * (2 * KD + HD), Co = nh * HD, nyq = (nkb + 3) >> 2;
    const int b = blockIdx.x / nh, h = blockIdx.x % nh;
    const unsigned short *qp = qkv + (size_t)b * N * C3 + h * KD, *kp = qp + nh * KD, *vp = qkv + (size_t)b * N * C3 + 2 * nh * KD + h * HD;
    const unsigned short *dop = dout + (size_t)b * N * Co + h * HD, *op = o + (size_t)b * N * Co + h * HD;
    const float *lp = lse + ((size_t)b * nh + h) * N;
    unsigned short *dq = dqkv + (size_t)b * N * C3 + h * KD, *dk = dq + nh * KD, *dv = dqkv + (size_t)b * N * C3 + 2 * nh * KD + h * HD;
    const f32x4 zero4 = f32x4{0.f, 0.f, 0.f, 0.f};

    if ((int)blockIdx.y < nyq) {  // ---------------------------------------------------------------- dQ: the wave owns a query block
        char *sK = at_sm, *sV = sK + R * kAtKPitch, *sKt = sV + R * kAtVPitch;
        float *sD = reinterpret_cast<float *>(sKt + nks * 2048);
        at_stage_rows<KD / 8>(sK, kAtKPitch, kp, C3, N, R, tid);
        at_stage_rows<HD / 8>(sV, kAtVPitch, vp, C3, N, R, tid);
        at_stage_frags<KD / 8>(sKt, kp, C3, N, R, tid);
        at_stage_D(sD, dop, op, Co, N, R, tid);
        __syncthreads();
        const int qb = blockIdx.y * 4 + wave;
        if (qb >= nkb) return;
        const int q = qb * 16 + pl;
        const bool qok = q < N;
        const bf8 qf = at_ld8(qp + (size_t)q * C3 + g * 8, qok);
        const bf8 d0 = at_ld8(dop + (size_t)q * Co + g * 8, qok), d1 = at_ld8(dop + (size_t)q * Co + 32 + g * 8, qok);
        const float lq = qok ? lp[q] : 0.f, Dq = sD[q];
        f32x4 acc[KD / 16] = {zero4, zero4};
        for (int st = 0; st < nks; ++st) {
            bf8 dsh, dsl;
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                const int jb = 2 * st + half;  // (a block past nkb is staged zeros: its keys are masked like any key >= N)
                const char *kr = sK + (jb * 16 + pl) * kAtKPitch, *vr = sV + (jb * 16 + pl) * kAtVPitch;
                const f32x4 s = at_mfma(*reinterpret_cast<const bf8 *>(kr + g * 16), qf, zero4);  // S^T[key 4 g + r][query pl]
                f32x4 dp = at_mfma(*reinterpret_cast<const bf8 *>(vr + g * 16), d0, zero4);      // dP^T, d = 0..31
                dp = at_mfma(*reinterpret_cast<const bf8 *>(vr + 64 + g * 16), d1, dp);           //       d = 32..63
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float p = at_exp(s[r] * scale - lq);
                    const float ds = (jb * 16 + g * 4 + r < N) ? p * (dp[r] - Dq) : 0.f;  // a padded key
                    bfe hi, lo;
                    at_split(ds, hi, lo);
                    dsh[half * 4 + r] = hi;
                    dsl[half * 4 + r] = lo;
                }
            }
#pragma unroll
            for (int cb = 0; cb < KD / 16; ++cb) {  // dQ^T[c][query] += K^T[c][key] dS^T[key][query]
                const bf8 kt = *reinterpret_cast<const bf8 *>(sKt + ((st * (KD / 16) + cb) * 64 + lane) * 16);
                acc[cb] = at_mfma(kt, dsh, acc[cb]);
                acc[cb] = at_mfma(kt, dsl, acc[cb]);
            }
        }
        if (!qok) return;
#pragma unroll
        for (int cb = 0; cb < KD / 16; ++cb) {
            uint2 w;
            w.x = HX<false>::pack2(acc[cb][0] * scale, acc[cb][1] * scale);
            w.y = HX<false>::pack2(acc[cb][2] * scale, acc[cb][3] * scale);
            *reinterpret_cast<uint2 *>(dq + (size_t)q * C3 + cb * 16 + g * 4) = w;
        }
        return;
    }
    // -------------------------------------------------------------------------------------------------- dK, dV: the wave owns a key block
    char *sQ = at_sm, *sDO = sQ + R * kAtKPitch, *sQt = sDO + R * kAtVPitch, *sDOt = sQt + nks * 2048;
    float *sD = reinterpret_cast<float *>(sDOt + nks * 4096), *sL = sD + R;
    at_stage_rows<KD / 8>(sQ, kAtKPitch, qp, C3, N, R, tid);
    at_stage_rows<HD / 8>(sDO, kAtVPitch, dop, Co, N, R, tid);
    at_stage_frags<KD / 8>(sQt, qp, C3, N, R, tid);
    at_stage_frags<HD / 8>(sDOt, dop, Co, N, R, tid);
    at_stage_D(sD, dop, op, Co, N, R, tid);
    for (int i = tid; i < R; i += 256) sL[i] = i < N ? lp[i] : 0.f;
    __syncthreads();
    const int kb = ((int)blockIdx.y - nyq) * 4 + wave;
    if (kb >= nkb) return;
    const int key = kb * 16 + pl;
    const bool kok = key < N;
    const bf8 kf = at_ld8(kp + (size_t)key * C3 + g * 8, kok);
    const bf8 v0 = at_ld8(vp + (size_t)key * C3 + g * 8, kok), v1 = at_ld8(vp + (size_t)key * C3 + 32 + g * 8, kok);
    f32x4 accV[HD / 16] = {zero4, zero4, zero4, zero4}, accK[KD / 16] = {zero4, zero4};
    for (int st = 0; st < nks; ++st) {
        bf8 ph, pw, dsh, dsl;
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const int qb = 2 * st + half;
            const char *qr = sQ + (qb * 16 + pl) * kAtKPitch, *dr = sDO + (qb * 16 + pl) * kAtVPitch;
            const f32x4 s = at_mfma(*reinterpret_cast<const bf8 *>(qr + g * 16), kf, zero4);  // S[query 4 g + r][key pl]
            f32x4 dp = at_mfma(*reinterpret_cast<const bf8 *>(dr + g * 16), v0, zero4);      // dP, d = 0..31
            dp = at_mfma(*reinterpret_cast<const bf8 *>(dr + 64 + g * 16), v1, dp);           //     d = 32..63
            const f32x4 l4 = *reinterpret_cast<const f32x4 *>(sL + qb * 16 + g * 4), D4 = *reinterpret_cast<const f32x4 *>(sD + qb * 16 + g * 4);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool real = qb * 16 + g * 4 + r < N;  // a padded query adds nothing to a real key's row
                const float p = real ? at_exp(s[r] * scale - l4[r]) : 0.f;
                const float ds = real ? p * (dp[r] - D4[r]) : 0.f;
                bfe hi, lo;
                at_split(p, hi, lo);
                ph[half * 4 + r] = hi;
                pw[half * 4 + r] = lo;
                at_split(ds, hi, lo);
                dsh[half * 4 + r] = hi;
                dsl[half * 4 + r] = lo;
            }
        }
#pragma unroll
        for (int db = 0; db < HD / 16; ++db) {  // dV^T[d][key] += dO^T[d][query] P[query][key]
            const bf8 f = *reinterpret_cast<const bf8 *>(sDOt + ((st * (HD / 16) + db) * 64 + lane) * 16);
            accV[db] = at_mfma(f, ph, accV[db]);
            accV[db] = at_mfma(f, pw, accV[db]);
        }
#pragma unroll
        for (int cb = 0; cb < KD / 16; ++cb) {  // dK^T[c][key] += Q^T[c][query] dS[query][key]
            const bf8 f = *reinterpret_cast<const bf8 *>(sQt + ((st * (KD / 16) + cb) * 64 + lane) * 16);
            accK[cb] = at_mfma(f, dsh, accK[cb]);
            accK[cb] = at_mfma(f, dsl, accK[cb]);
        }
    }
    if (!kok) return;
#pragma unroll
    for (int db = 0; db < HD / 16; ++db) {
        float a[4] = {accV[db][0], accV[db][1], accV[db][2], accV[db][3]};
        if (dv_add) {
            const uint2 e = *reinterpret_cast<const uint2 *>(dv_add + ((size_t)b * N + key) * Co + h * HD + db * 16 + g * 4);
            a[0] += HX<false>::lo(e.x); a[1] += HX<false>::hi(e.x); a[2] += HX<false>::lo(e.y); a[3] += HX<false>::hi(e.y);
        }
        uint2 w;
        w.x = HX<false>::pack2(a[0], a[1]);
        w.y = HX<false>::pack2(a[2], a[3]);
        *reinterpret_cast<uint2 *>(dv + (size_t)key * C3 + db * 16 + g * 4) = w;
    }
#pragma unroll
    for (int cb = 0; cb < KD / 16; ++cb) {
        uint2 w;
        w.x = HX<false>::pack2(accK[cb][0] * scale, accK[cb][1] * scale);
        w.y = HX<false>::pack2(accK[cb][2] * scale, accK[cb][3] * scale);
        *reinterpret_cast<uint2 *>(dk + (size_t)key * C3 + cb * 16 + g * 4) = w;
    }
}

namespace {
bool at_aligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }  // (NULL passes)

int at_check(obb_ctx *ctx, const char *fn, int32_t B, int32_t N, int32_t nh) {
    OBB_REQUIRE(ctx, ctx && B >= 1 && nh >= 1, "%s: B = %d, nh = %d must be at least 1", fn, (int)B, (int)nh);
    OBB_REQUIRE(ctx, N >= 1 && N <= kAtMaxN, "%s: N = %d tokens: 1 to %d (the keys of a head are resident in LDS)", fn, (int)N, kAtMaxN);
    OBB_REQUIRE(ctx, (int64_t)B * nh < (1ll << 31) && (int64_t)nh * 128 < (1ll << 24), "%s: B = %d, nh = %d: too large", fn, (int)B, (int)nh);
    return OBB_OK;
}
size_t at_fwd_lds(int nks) { return (size_t)nks * (32 * kAtKPitch + 4 * 1024); }
size_t at_bwd_lds(int nks) { return (size_t)nks * (32 * (kAtKPitch + kAtVPitch) + 6 * 1024 + 2 * 32 * 4); }  // the dK / dV workgroup's, the larger
}  // namespace

}  // namespace obb

using namespace obb;

extern "C" {

int obb_attn_fwd_bf16(obb_ctx *ctx, const uint16_t *qkv, int32_t B, int32_t N, int32_t nh, uint16_t *out, float *lse, obb_stream_t s) {
    if (int rc = at_check(ctx, "obb_attn_fwd_bf16", B, N, nh)) return rc;
    OBB_REQUIRE(ctx, qkv && out && lse, "obb_attn_fwd_bf16: NULL buffer");
    OBB_REQUIRE(ctx, at_aligned(qkv) && at_aligned(out), "obb_attn_fwd_bf16: qkv and out must be 16-byte aligned");
    const int nkb = (N + 15) / 16, nks = (nkb + 1) / 2;
    OBB_HIP(ctx, allow_dyn_lds((const void *)k_attn_fwd, at_fwd_lds(kAtMaxN / 32)));
    const float scale = (float)(1.0 / sqrt((double)kAtKD));
    hipLaunchKernelGGL(k_attn_fwd, dim3((unsigned)(B * nh), (unsigned)cdiv(nkb, 4)), dim3(256), at_fwd_lds(nks), (hipStream_t)s, qkv, (int)N, (int)nh, scale, out, lse);
    OBB_LAUNCH_CHECK(ctx);
    return OBB_OK;
}

int obb_attn_bwd_bf16(obb_ctx *ctx, const uint16_t *qkv, const uint16_t *out, const float *lse, const uint16_t *dout, const uint16_t *dv_add, int32_t B,
                      int32_t N, int32_t nh, uint16_t *dqkv, obb_stream_t s) {
    if (int rc = at_check(ctx, "obb_attn_bwd_bf16", B, N, nh)) return rc;
    OBB_REQUIRE(ctx, qkv && out && lse && dout && dqkv, "obb_attn_bwd_bf16: NULL buffer (only dv_add may be NULL)");
    OBB_REQUIRE(ctx, at_aligned(qkv) && at_aligned(out) && at_aligned(dout) && at_aligned(dv_add) && at_aligned(dqkv),
                "obb_attn_bwd_bf16: qkv, out, dout, dv_add and dqkv must be 16-byte aligned");
    const int nkb = (N + 15) / 16, nks = (nkb + 1) / 2;
    OBB_HIP(ctx, allow_dyn_lds((const void *)k_attn_bwd, at_bwd_lds(kAtMaxN / 32)));  // 79.5 KiB at N = 192: more than the 64 KiB default
    const float scale = (float)(1.0 / sqrt((double)kAtKD));
    hipLaunchKernelGGL(k_attn_bwd, dim3((unsigned)(B * nh), (unsigned)(2 * cdiv(nkb, 4))), dim3(256), at_bwd_lds(nks), (hipStream_t)s, qkv, out, lse, dout, dv_add,
                       (int)N, (int)nh, scale, dqkv);
    OBB_LAUNCH_CHECK(ctx);
    return OBB_OK;
}

}  // extern "C"
