// Validation, the route from the trainer's state into the inference engine: the flat fp32 buffers of train.ParamGroups (conv weights in group 0,
// BatchNorm gamma in group 1, beta and the plain convs' biases in group 2, the running statistics in `buffers`) -> the fp32 data section of an
// "OBBW" weight blob (netplan.hip parse_blob: OIHW weights, then the bias, per record in record order, dense) in ONE launch.
//
// Replaces the per-layer `Net.fold()` (one torch expression chain per Conv block, ~90 blocks) + the host-side blob writer between `ModelEMA` and the
// validator of `model.train(...)` (Train_OBB.py:792-841 validates the EMA model after every epoch).
//
// The launch is described by a device-resident table of int64 words, built once on the host (train.FoldPlan):
//     head   [0] kFoldMagic  [1] records  [2] elements of the output  [3..6] elements the records read up to in w_flat, g_flat, b_flat, buffers  [7] 0
//     record [0] conv weight offset in w_flat  [1] gamma offset in g_flat (unused for a plain conv)  [2] beta / bias offset in b_flat
//            [3] running mean offset  [4] running variance offset in buffers (unused for a plain conv)  [5] destination offset in the output
//            [6] cout | elements per output channel << 32  [7] first workgroup | kind << 32
// Record i owns ceil(cout (per + 1) / 256) workgroups of the launch's index space (its segment of that space starts at a multiple of 256 lanes),
// so a workgroup lies in one record: it finds it by bisection over the records' first workgroups, as k_pack_conv_multi_bf16 does.  The
// destinations themselves are dense (the blob has no padding between records).  Kinds:
//     OBB_FOLD_BN     f = gamma / sqrt(var + eps);  w' = w f;  b' = beta - mean f     -- train._BNBlock.fold() in IEEE fp32, nothing contracted
//     OBB_FOLD_PLAIN  the head's `*.2` outputs: weight and bias copied as they are
//     OBB_FOLD_QKV    OBB_FOLD_BN whose output row c (checkpoint order: [q | k | v] per head, 32 + 32 + 64 rows) is read from the device row
//                     train.qkv_device_order put it in ([q of all heads | k of all heads | v of all heads])
// The head is compared with the launch's own arguments and every record with the head: a table of another plan stores nothing.
#include "ctx.h"

using namespace obb;

namespace {

constexpr int64_t kFoldMagic = 0x4f4242464f4c4431ll;  // "OBBFOLD1"
constexpr int kFoldHead = OBB_FOLD_TABLE_HEAD, kFoldRec = OBB_FOLD_TABLE_REC;

// device row of checkpoint row c of a qkv conv with nh heads (key_dim 32, head_dim 64): the inverse of train.qkv_device_order
__device__ __forceinline__ int qkv_device_row(int c, int nh) {
    const int h = c >> 7, r = c & 127;
    if (r < 32) return h * 32 + r;
    if (r < 64) return nh * 32 + h * 32 + (r - 32);
    return nh * 64 + h * 64 + (r - 64);
}

__global__ __launch_bounds__(256) void k_fold_blob(const float *__restrict__ w, const float *__restrict__ g, const float *__restrict__ b,
                                                  const float *__restrict__ buf, const int64_t *__restrict__ tab, int nrec, float eps,
                                                  float *__restrict__ out, int64_t out_elems) {
    if (tab[0] != kFoldMagic || tab[1] != nrec || tab[2] != out_elems) return;
    int lo = 0, hi = nrec - 1;
    while (lo < hi) {  // the last record whose first workgroup is <= blockIdx.x
        const int mid = (lo + hi + 1) >> 1;
        if ((tab[kFoldHead + (int64_t)mid * kFoldRec + 7] & 0xffffffffll) <= (int64_t)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const int64_t *__restrict__ r = tab + kFoldHead + (int64_t)lo * kFoldRec;
    const int64_t w_off = r[0], g_off = r[1], b_off = r[2], m_off = r[3], v_off = r[4], dst = r[5];
    const int64_t cout = r[6] & 0xffffffffll, per = r[6] >> 32, first = r[7] & 0xffffffffll;
    const int kind = (int)(r[7] >> 32);
    const int64_t nw = cout * per, n = nw + cout;
    const int64_t o = ((int64_t)blockIdx.x - first) * 256 + threadIdx.x;
    if (cout < 1 || per < 1 || o < 0 || o >= n || dst < 0 || dst + n > out_elems) return;
    if (w_off < 0 || w_off + nw > tab[3] || b_off < 0 || b_off + cout > tab[5]) return;
    const bool bn = kind != OBB_FOLD_PLAIN;
    if (bn && (g_off < 0 || g_off + cout > tab[4] || m_off < 0 || m_off + cout > tab[6] || v_off < 0 || v_off + cout > tab[6])) return;
    if (kind != OBB_FOLD_BN && kind != OBB_FOLD_PLAIN && !(kind == OBB_FOLD_QKV && (cout & 127) == 0)) return;
    const int64_t co = o < nw ? o / per : o - nw;
    const int64_t sr = kind == OBB_FOLD_QKV ? (int64_t)qkv_device_row((int)co, (int)(cout >> 7)) : co;  // the row the flat buffers hold it in
    float v;
    if (!bn) {
        v = o < nw ? w[w_off + o] : b[b_off + co];
    } else {
        // sqrtf and / are the correctly rounded IEEE operations (hipcc's default for fp32); the __fsqrt_rn intrinsic is NOT: without
        // OCML_BASIC_ROUNDED_OPERATIONS the HIP headers map it to the native approximation, which misses numpy's float32 fold in the last bit
        const float f = g[g_off + sr] / sqrtf(__fadd_rn(buf[v_off + sr], eps));
        v = o < nw ? __fmul_rn(w[w_off + sr * per + (o - co * per)], f) : __fsub_rn(b[b_off + sr], __fmul_rn(buf[m_off + sr], f));
    }
    out[dst + o] = v;
}

}  // namespace

extern "C" int obb_fold_blob_f32(obb_ctx *ctx, const float *w_flat, const float *g_flat, const float *b_flat, const float *buffers, const int64_t *table,
                                 int64_t table_words, int32_t nrec, float eps, float *out, int64_t out_elems, obb_stream_t s) {
    const char *fn = "obb_fold_blob_f32";
    OBB_REQUIRE(ctx, ctx && w_flat && g_flat && b_flat && buffers && table && out, "%s: NULL buffer", fn);
    OBB_REQUIRE(ctx, nrec >= 1 && table_words == kFoldHead + (int64_t)nrec * kFoldRec, "%s: the table holds %lld words, %lld needed for %d records", fn,
                (long long)table_words, (long long)(kFoldHead + (int64_t)nrec * kFoldRec), (int)nrec);
    OBB_REQUIRE(ctx, eps > 0.0f && out_elems >= 1, "%s: eps must be positive and the output non-empty", fn);
    // a record's last workgroup may be part-filled, so the launch's index space is at most one workgroup per record longer than the output
    const int64_t wgs = cdiv(out_elems, 256) + nrec;
    OBB_REQUIRE(ctx, wgs < (1ll << 31), "%s: %lld workgroups: too many for one launch", fn, (long long)wgs);
    hipLaunchKernelGGL(k_fold_blob, dim3((unsigned)wgs), dim3(256), 0, (hipStream_t)s, w_flat, g_flat, b_flat, buffers, table, (int)nrec, eps, out, out_elems);
    OBB_LAUNCH_CHECK(ctx);
    return OBB_OK;
}
