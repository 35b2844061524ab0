// Model runtime: issues the launch plan of a loaded model (plan.h; built per input shape by netplan.hip).  Sizes the activation slab,
// binds the plan's buffers and the caller's tensors to the launch descriptors of one sub-batch, and runs a round eagerly, as two
// half-batch chains, or as a replayed hipGraph.  Serves the model / forward / debug entry points of the C ABI.
//
// Replaces `YOLO("best416.pt")` + `model(net_input, ...)`'s OBBModel forward (Detect_OBB.py:26, 81-83).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "plan.h"

namespace obb {

static int ensure_capacity(obb_ctx *ctx, Plan &P, int B) {
    if (B <= P.cap) return OBB_OK;
    int cap = std::max(B, 1);
    int64_t off = 0;
    for (Buf &b : P.bufs) {
        b.off = off;
        if (b.virt) continue;
        off += ((int64_t)cap * b.per_img() * (b.f32 ? 4 : 2) + 255) / 256 * 256;
    }
    void *slab = nullptr;
    OBB_HIP(ctx, hipDeviceSynchronize());
    P.drop_graphs();  // captured launches point into the old slab
    if (P.slab) { (void)hipFree(P.slab); P.slab = nullptr; P.cap = 0; }
    OBB_HIP(ctx, hipMalloc(&slab, (size_t)off + 256));
    P.slab = slab;
    P.cap = cap;
    P.bytes_per_img = off / cap;
    for (Buf &b : P.bufs) b.p = (char *)slab + b.off;
    return OBB_OK;
}

static TensorRef tref(const Plan &P, const Slice &s, int boff = 0) {
    TensorRef t;
    if (s.buf < 0) return t;
    const Buf &b = P.bufs[s.buf];
    if (b.blk > 0) {  // [C / blk][cap images][pixel][blk]
        t.p = (char *)b.p + (int64_t)boff * b.H * b.W * b.blk * 2;
        t.bs = (int64_t)b.H * b.W * b.blk; t.cs = b.blk; t.co = s.co;
        t.cpb = b.blk / 8; t.ps = (int64_t)P.cap * b.H * b.W * b.blk;
        return t;
    }
    t.p = (char *)b.p + (int64_t)boff * b.per_img() * (b.f32 ? 4 : 2);  // sub-batch `boff` owns its own image range of every buffer
    t.bs = b.per_img(); t.cs = b.C; t.co = s.co;
    if (b.blk32) { t.cs = b.blk32; t.cpb = b.blk32 / 4; t.ps = (int64_t)b.H * b.W * b.blk32; }  // [image][C / 8][pixel][8]
    return t;
}

static int get_plan(obb_ctx *ctx, int h, int w, Plan **out) {
    if (!ctx->model) return set_error(ctx, OBB_ERR_STATE, "no model loaded (call obb_model_load first)");
    OBB_REQUIRE(ctx, h > 0 && w > 0 && h % 32 == 0 && w % 32 == 0 && h <= 1280 && w <= 1280,
                "input %dx%d unsupported: both sides must be multiples of 32 in [32, 1280]", h, w);
    Model &M = *ctx->model;
    auto key = std::make_pair(h, w);
    auto it = M.plans.find(key);
    if (it == M.plans.end()) {
        std::unique_ptr<Plan> P(new Plan());
        P->h = h; P->w = w;
        int rc = build_plan(ctx, M, *P);
        if (rc) return rc;
        it = M.plans.emplace(key, std::move(P)).first;
    }
    *out = it->second.get();
    return OBB_OK;
}

// per-anchor maximum of the class logits (the gate of obb_decode_nms_gate) for plans whose class tails are not fused
__global__ __launch_bounds__(256) void k_class_max(const float *__restrict__ head, int64_t n, int no_pad, int c0, int nc, float *__restrict__ cmax) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float *r = head + i * no_pad + c0;
    float m = -INFINITY;
    for (int j = 0; j < nc; ++j) m = fmaxf(m, r[j]);
    cmax[i] = m;
}

// rows of pyramid level `level` in the caller's head tensor, from channel `co`
static TensorRef head_ref(const Plan &P, float *head, int level, int co) {
    TensorRef t;
    t.p = head + (int64_t)P.lvl_off[level] * P.no_pad;
    t.bs = (int64_t)P.A * P.no_pad; t.cs = P.no_pad; t.co = co;
    return t;
}

// What a ConvLaunch and a Conv32Launch need bound per sub-batch alike: the input (uint8 tiles, virtual concat or plain slice), the
// residual, the output and the 1-D form of a 1x1 layer.  The output target is the head rows of the op's level or its activation slice.
// A 1-D launch splits its pixel row back into (image, pixel) for head rows; for a slice only where the caller passes `slice_hw`.
// The rows of a fused tail go to tail_out.  What else is bound differs between the two families and is kept as found (the launchers'
// validity checks read these fields):
//   tail_to_slice = false (16-bit): only head rows go to tail_out; a tail with an activation writes its slice through `out` (tail_act16)
//   out_beside_tail = true (fp32): `out` is bound to the same target beside tail_out
template <typename LaunchT>
static void bind_conv(LaunchT &L, const Plan &P, const Model &M, const Op &op, const uint8_t *tiles, float *head, int B, int boff, int slice_hw,
                      bool tail_to_slice, bool out_beside_tail) {
    L.B = B;
    if (op.in.buf == -1) {
        L.in.p = (void *)tiles; L.in.bs = (int64_t)P.h * P.w * M.ch; L.in.cs = M.ch; L.in.co = 0;
    } else if (op.vin) {
        const Buf &vb = P.bufs[op.in.buf];
        L.in = tref(P, Slice{vb.va_buf, vb.va_co, vb.va_C}, boff);
        L.in2 = tref(P, Slice{vb.vb_buf, vb.vb_co, vb.vb_C}, boff);
        L.up_c = vb.va_C; L.up_W = op.W; L.up_HW = op.H * op.W;
    } else L.in = tref(P, op.in, boff);
    const bool to_head = op.head_level >= 0;
    const TensorRef o = to_head ? head_ref(P, head, op.head_level, op.out.co) : tref(P, op.out, boff);
    const int o_hw = to_head ? (op.one_d ? op.Ho * op.Wo : 0) : slice_hw;
    const bool to_tail = L.tail_cout > 0 && (to_head || tail_to_slice);
    if (to_tail) { L.tail_out = o; L.tail_out_hw = o_hw; }
    if (!to_tail || out_beside_tail) { L.out = o; L.out_hw = o_hw; }
    L.res = tref(P, op.res, boff);
    if (op.one_d) {  // 1x1: batch x pixels is one dense pixel row
        const int64_t npx = (int64_t)B * op.Ho * op.Wo;
        L.B = 1; L.Hin = L.Hout = 1; L.Win = L.Wout = (int)npx;
        L.tiles_y = 1; L.tiles_x = (int)((npx + L.TW - 1) / L.TW);
    }
}

// the launches that read the uint8 tiles themselves (Stem32Launch, StemLaunch, FrontLaunch)
template <typename LaunchT>
static LaunchT on_tiles(LaunchT L, const uint8_t *tiles, int B, const TensorRef &out) {
    L.B = B; L.in = tiles; L.out = out;
    return L;
}

// One op on images [boff, boff + B) of every activation buffer
static hipError_t launch_op(const Plan &P, const Model &M, const Op &op, const uint8_t *tiles, int B, float *head, float *cmax, hipStream_t st, int boff) {
    auto T = [&](const Slice &s) { return tref(P, s, boff); };
    switch (op.type) {
        case OP_CONV32: {
            Conv32Launch L = op.c32;
            L.xtile = M.o.xtile;
            const bool emit_cmax = cmax && op.emit_cmax;  // the class logits' maximum instead of the logits' own layer output
            // (a channel-blocked output is per image: the flattened pixel row of a 1-D launch is split back into (image, pixel))
            bind_conv(L, P, M, op, tiles, head, B, boff, op.one_d && op.out.buf >= 0 && P.bufs[op.out.buf].blk32 ? op.Ho * op.Wo : 0, true, !emit_cmax);
            if (emit_cmax) { L.cmax = cmax + P.lvl_off[op.head_level]; L.cmax_bs = P.A; }
            if (op.upacc) {  // the skip member alone; the upsampled member's share arrives as the accumulators' initial value
                L.in = L.in2; L.in2 = TensorRef(); L.up_c = 0;
                L.acc_init = T(op.ini);
            }
            return launch_conv32(L, st);
        }
        case OP_CONV: {
            ConvLaunch L = op.conv;
            bind_conv(L, P, M, op, tiles, head, B, boff, 0, false, false);
            if (!op.one_d && M.o.nitile) {  // the 4 x 4 / 2 x 2 maps of small tiles: several whole images per 64-pixel tile
                const int ni = conv_ni_supported(L);
                if (ni > 1) { L.NI = ni; L.TH = L.Hout; L.TW = L.Wout; L.tiles_x = L.tiles_y = 1; }
            }
            return launch_conv(L, st);
        }
        case OP_PW32: {
            Pw32Launch L = op.pw32;
            L.in = T(op.in); L.out = T(op.out); L.res = T(op.res);
            L.npix = (int64_t)B * op.Ho * op.Wo; L.hw = op.Ho * op.Wo;
            return launch_pw32(L, st);
        }
        case OP_C3K2F32: {
            C3k2F32Launch L = op.c3k2f;
            L.B = B; L.cat = T(op.in); L.out = T(op.out);
            return launch_c3k2f32(L, st);
        }
        case OP_STEM32: return launch_stem32(on_tiles(op.stem32, tiles, B, T(op.out)), st);
        case OP_STEM: return launch_stem(on_tiles(op.stem, tiles, B, T(op.out)), st);
        case OP_FRONT: return launch_front(on_tiles(op.front, tiles, B, T(op.out)), st);
        case OP_C3KIMG: {
            C3kImgLaunch L = op.c3kimg;
            L.B = B; L.in = T(op.in); L.out = T(op.out);
            return launch_c3kimg(L, st);
        }
        case OP_DWPW: {
            DwPwLaunch L = op.dwpw;
            L.B = B; L.in = T(op.in);
            if (op.head_level >= 0) {
                L.tail_out = head_ref(P, head, op.head_level, op.out.co);
                L.sink = (char *)M.lut_dev + 512;
            } else L.out = T(op.out);
            return launch_dwpw(L, st);
        }
        case OP_BNECK: {
            BneckLaunch L = op.bneck;
            L.B = B; L.y1 = T(op.in);
            if (L.CO > 0) {  // closing 1x1 fused: y2 stays in registers; op.out is the block's output, op.res the y0 member
                L.y2 = L.y1; L.y0 = T(op.res); L.out = T(op.out);
            } else L.y2 = T(op.out);
            return launch_bneck(L, st);
        }
        case OP_DW:
            if (M.f32) return launch_dwconv3_f32(T(op.in), T(op.out), T(op.res), op.dw_w32, op.dw_b, B, op.H, op.W, op.in.C, op.act, st);
            return launch_dwconv3(T(op.in), T(op.out), T(op.res), op.dw_w, op.dw_b, B, op.H, op.W, op.in.C, op.act, M.f16, st);
        case OP_SPPF:
            if (M.f32) return launch_sppf_pools_f32(T(op.out), B, op.H, op.W, op.in.C, st);
            return launch_sppf_pools(T(op.out), B, op.H, op.W, op.in.C, M.f16, st);
        case OP_POOL:
            if (M.f32) return launch_maxpool5_f32(T(op.in), T(op.out), B, op.H, op.W, op.in.C, st);
            return launch_maxpool5(T(op.in), T(op.out), B, op.H, op.W, op.in.C, M.f16, st);
        case OP_UP:
            if (M.f32) return launch_upsample2_f32(T(op.in), T(op.out), B, op.H, op.W, op.in.C, st);
            return launch_upsample2(T(op.in), T(op.out), B, op.H, op.W, op.in.C, st);
        case OP_ATTN:
            if (M.f32) return launch_attention_f32(T(op.in), T(op.out), B, op.N, op.nh, op.kd, op.hd, M.o.attn_mfma, st);
            return launch_attention(T(op.in), T(op.out), B, op.N, op.nh, op.kd, op.hd, M.f16, M.o.attn_mfma, st);
    }
    return hipErrorInvalidValue;
}

// One sub-batch: images [boff, boff + B) of every activation buffer, all launches on `st`.
// (Measured and dropped: walking the HBM-bound stride-2 .. stride-8 front of the network in slices of 32 .. 256 tiles so that a layer's
//  output is still in the 256 MiB Infinity Cache when the next layer reads it: 9.41 ms per 1024 tiles without, 9.96 / 9.55 / 9.39 / 9.37 ms
//  with slices of 32 / 64 / 128 / 256.)
static int run_forward(obb_ctx *ctx, Plan &P, const uint8_t *tiles, int B, float *head, float *cmax, hipStream_t st, int boff) {
    Model &M = *ctx->model;
    for (const Op &op : P.ops) {
        const hipError_t e = launch_op(P, M, op, tiles, B, head, cmax, st, boff);
        if (e != hipSuccess) return set_error(ctx, OBB_ERR_HIP, "forward: launch of '%s' failed: %s", op.name.c_str(), hipGetErrorString(e));
    }
    if (cmax && P.cmax_mask != 7) {  // a plan without the fused class tails (16-bit modes, "tail" = 0, small maps): one pass over the head rows
        const int64_t n = (int64_t)B * P.A;
        hipLaunchKernelGGL(k_class_max, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, st, (const float *)head, n, P.no_pad, 4 * kRegMax, M.nc, cmax);
        if (hipGetLastError() != hipSuccess) return set_error(ctx, OBB_ERR_HIP, "forward: launch of the class-maximum pass failed");
    }
    return OBB_OK;
}

// One round (<= max sub-batch) of the forward.  The round is split into `nsplit` independent sub-batches that run concurrently on
// side streams (fork/join around the caller's stream): the ~110 launches of a forward are a dependent chain of short kernels, and
// two chains in flight hide each other's ramp-up, tail and launch latency (measured: 4.64 -> 4.26 ms per 256 tiles with 2).
// "fwd_split" 0 (default) = 2 chains: caller stream + side streams + one more user stream still fit the 4 hardware queues.  (3 / 4
// chains, 1024-tile bench steps: fp16 8.82 -> 9.86 / 10.58 ms; fp32 within the run-to-run noise of 2 -- 34.99 vs 36.05 on one box,
// 35.52 vs 35.14 on the next.)
static int run_round(obb_ctx *ctx, Plan &P, const uint8_t *tiles, int B, float *head, float *cmax, hipStream_t main_st) {
    Model &M = *ctx->model;
    const int nsplit_cfg = ctx->opt.fwd_split > 0 ? std::min(Plan::kLanes, ctx->opt.fwd_split) : 2;
    int ns = (B >= 32 * nsplit_cfg) ? nsplit_cfg : 1;
    if (ns == 1) return run_forward(ctx, P, tiles, B, head, cmax, main_st, 0);
    if (!P.lanes[0]) {
        OBB_HIP(ctx, hipEventCreateWithFlags(&P.ev_fork, hipEventDisableTiming));
        for (int i = 0; i < Plan::kLanes; ++i) {
            OBB_HIP(ctx, hipStreamCreateWithFlags(&P.lanes[i], hipStreamNonBlocking));
            OBB_HIP(ctx, hipEventCreateWithFlags(&P.ev_done[i], hipEventDisableTiming));
        }
    }
    OBB_HIP(ctx, hipEventRecord(P.ev_fork, main_st));
    for (int i = 0; i < ns; ++i) {
        int lo = (int)((int64_t)B * i / ns), hi = (int)((int64_t)B * (i + 1) / ns);
        OBB_HIP(ctx, hipStreamWaitEvent(P.lanes[i], P.ev_fork, 0));
        int rc = run_forward(ctx, P, tiles + (int64_t)lo * P.h * P.w * M.ch, hi - lo, head + (int64_t)lo * P.A * P.no_pad, cmax ? cmax + (int64_t)lo * P.A : nullptr, P.lanes[i], lo);
        if (rc) return rc;
        OBB_HIP(ctx, hipEventRecord(P.ev_done[i], P.lanes[i]));
    }
    for (int i = 0; i < ns; ++i) OBB_HIP(ctx, hipStreamWaitEvent(main_st, P.ev_done[i], 0));  // join
    return OBB_OK;
}

template <bool F16>
__global__ void k_half_slice_to_f32(const bf16_t *__restrict__ src, int64_t bs, int cs, int co, int C, int64_t npix_per_img, int B,
                                    float *__restrict__ dst, int blk, int64_t ps) {
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int64_t total = (int64_t)B * npix_per_img * C;
    if (i >= total) return;
    int c = (int)(i % C) + co;
    int64_t pix = (i / C) % npix_per_img;
    int64_t b = i / ((int64_t)C * npix_per_img);
    dst[i] = HX<F16>::one(blk > 0 ? src[(int64_t)(c / blk) * ps + b * bs + pix * blk + c % blk] : src[b * bs + pix * cs + c]);
}

__global__ void k_f32_slice_copy(const float *__restrict__ src, int64_t bs, int cs, int co, int C, int64_t npix_per_img, int B, float *__restrict__ dst, int blk) {
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)B * npix_per_img * C) return;
    int c = (int)(i % C) + co;
    int64_t pix = (i / C) % npix_per_img;
    int64_t b = i / ((int64_t)C * npix_per_img);
    dst[i] = blk > 0 ? src[b * bs + (int64_t)(c / blk) * npix_per_img * blk + pix * blk + c % blk] : src[b * bs + pix * cs + c];
}

// the boolean engine switch named `k` (obb_set_option / obb_get_option), or nullptr
static bool *switch_of(obb_ctx *ctx, const std::string &k) {
    struct { const char *key; bool *flag; } sw[] = {
        {"tail", &ctx->opt.tail}, {"tail16", &ctx->opt.tail16}, {"bneck", &ctx->opt.bneck}, {"bneck_cv2", &ctx->opt.bneck_cv2},
        {"c3kimg", &ctx->opt.c3kimg}, {"dwpw", &ctx->opt.dwpw}, {"upfold", &ctx->opt.upfold}, {"stem", &ctx->opt.stem}, {"front", &ctx->opt.front}, {"pair", &ctx->opt.pair},
        {"hmerge", &ctx->opt.hmerge}, {"sppf_fuse", &ctx->opt.sppf_fuse}, {"attn_mfma", &ctx->opt.attn_mfma}, {"xtile", &ctx->opt.xtile}, {"nitile", &ctx->opt.nitile}, {"nc2", &ctx->opt.nc2}, {"blk32", &ctx->opt.blk32}, {"c3k2f", &ctx->opt.c3k2f}, {"pw32", &ctx->opt.pw32}, {"upacc", &ctx->opt.upacc}, {"graph", &ctx->opt.graph}};
    for (auto &e : sw)
        if (k == e.key) return e.flag;
    return nullptr;
}

}  // namespace obb

using namespace obb;

extern "C" {

int obb_model_load(obb_ctx *ctx, const void *blob_host, size_t bytes) {
    OBB_REQUIRE(ctx, ctx && blob_host && bytes > 0, "obb_model_load: bad arguments");
    OBB_HIP(ctx, hipSetDevice(ctx->device));
    OBB_HIP(ctx, hipDeviceSynchronize());
    std::shared_ptr<Model> M(new Model());
    M->blob.assign((const char *)blob_host, (const char *)blob_host + bytes);
    int rc = parse_blob(ctx, *M);
    if (rc) return rc;
    M->f16 = ctx->opt_f16;
    M->f32 = ctx->opt_f32;
    M->o = ctx->opt;
    M->o.hmerge = M->o.tail && M->o.hmerge;
    M->o.bneck = M->o.tail && M->o.bneck;  // both swallow intermediate activations ("tail" = 0 keeps every layer observable)
    if (M->f32) {  // `im.float() / 255`: IEEE division, one table entry per byte value
        std::vector<float> lut32(256);
        for (int v = 0; v < 256; ++v) lut32[v] = (float)v / 255.0f;
        OBB_HIP(ctx, hipMalloc((void **)&M->lut32_dev, 1024));
        OBB_HIP(ctx, hipMemcpy(M->lut32_dev, lut32.data(), 1024, hipMemcpyHostToDevice));
    }
    // u8 -> half(v / 255): the predictor's `im.float() / 255` followed by the 16-bit storage rounding, exactly
    std::vector<bf16_t> lut(256);
    for (int v = 0; v < 256; ++v) lut[v] = host_to_half((float)v / 255.0f, M->f16);
    OBB_HIP(ctx, hipMalloc((void **)&M->lut_dev, 512 + 1024));  // + a 1-KiB sink for the stores of lanes without an output pixel (conv.hip EXACT)
    OBB_HIP(ctx, hipMemcpy(M->lut_dev, lut.data(), 512, hipMemcpyHostToDevice));
    ctx->model = M;
    return OBB_OK;
}

int obb_model_unload(obb_ctx *ctx, int32_t slot) {
    OBB_REQUIRE(ctx, ctx && slot >= 0 && slot < 64, "obb_model_unload: bad arguments");
    OBB_HIP(ctx, hipSetDevice(ctx->device));
    OBB_HIP(ctx, hipDeviceSynchronize());  // nothing of the model's plans (slabs, weights, graphs) may still be in flight
    if (slot == ctx->slot) ctx->model.reset();
    ctx->slots.erase(slot);
    return OBB_OK;
}

int obb_set_option(obb_ctx *ctx, const char *key, int64_t value) {
    OBB_REQUIRE(ctx, ctx && key, "obb_set_option: bad arguments");
    std::string k(key);
    if (k == "precision") {  // 16 = fp16 storage (default), 1016 = bf16 storage, 32 = fp32 arithmetic end to end; next obb_model_load
        OBB_REQUIRE(ctx, value == 16 || value == 1016 || value == 32, "obb_set_option: precision must be 16 (fp16), 1016 (bf16) or 32 (fp32)");
        ctx->opt_f16 = (value != 1016);
        ctx->opt_f32 = (value == 32);
        return OBB_OK;
    }
    // engine switches: 1 = the fused form (default), 0 = its separate launches; all apply to the next obb_model_load, except
    // "graph", "fwd_split" and "microbatch", which steer how obb_forward issues its launches from the next call on
    if (bool *flag = switch_of(ctx, k)) { *flag = value != 0; return OBB_OK; }
    if (k == "fuse") return OBB_OK;  // (retired: the LDS-resident layer chains were slower than layer-by-layer on MI355X and are gone)
    if (k == "fwd_split") { OBB_REQUIRE(ctx, value >= 0 && value <= 4, "obb_set_option: fwd_split must be 0 (auto) .. 4"); ctx->opt.fwd_split = (int)value; return OBB_OK; }
    if (k == "microbatch") { OBB_REQUIRE(ctx, value >= 1 && value <= 1024, "obb_set_option: microbatch must be 1..1024"); ctx->opt.microbatch = (int)value; return OBB_OK; }
    if (k == "model_slot") {  // several models per context (dual-scale 128 + 416): select which one load/forward address
        OBB_REQUIRE(ctx, value >= 0 && value < 64, "obb_set_option: model_slot must be in [0, 64)");
        if ((int)value != ctx->slot) {
            ctx->slots[ctx->slot] = ctx->model;
            ctx->model = ctx->slots[(int)value];
            ctx->slot = (int)value;
        }
        return OBB_OK;
    }
    return set_error(ctx, OBB_ERR_INVALID, "obb_set_option: unknown key '%s'", key);
}

int obb_get_option(const obb_ctx *cctx, const char *key, int64_t *value) {
    obb_ctx *ctx = const_cast<obb_ctx *>(cctx);
    OBB_REQUIRE(ctx, ctx && key && value, "obb_get_option: bad arguments");
    std::string k(key);
    if (k == "precision") { *value = ctx->opt_f32 ? 32 : (ctx->opt_f16 ? 16 : 1016); return OBB_OK; }
    if (k == "model_slot") { *value = ctx->slot; return OBB_OK; }
    if (k == "fwd_split") { *value = ctx->opt.fwd_split; return OBB_OK; }
    if (k == "microbatch") { *value = ctx->opt.microbatch; return OBB_OK; }
    if (k == "fuse") { *value = 0; return OBB_OK; }
    if (const bool *flag = switch_of(ctx, k)) { *value = *flag ? 1 : 0; return OBB_OK; }
    return set_error(ctx, OBB_ERR_INVALID, "obb_get_option: unknown key '%s'", key);
}

int obb_model_info(const obb_ctx *cctx, int32_t h, int32_t w, int32_t *nc, int32_t *ch, int32_t *anchors, int32_t *nconv) {
    obb_ctx *ctx = const_cast<obb_ctx *>(cctx);
    OBB_REQUIRE(ctx, ctx, "obb_model_info: NULL context");
    if (!ctx->model) return set_error(ctx, OBB_ERR_STATE, "no model loaded");
    if (nc) *nc = ctx->model->nc;
    if (ch) *ch = ctx->model->ch;
    if (nconv) *nconv = (int32_t)ctx->model->nrec_blob;
    if (anchors) {
        OBB_REQUIRE(ctx, h > 0 && w > 0 && h % 32 == 0 && w % 32 == 0, "obb_model_info: h, w must be multiples of 32");
        *anchors = (h / 8) * (w / 8) + (h / 16) * (w / 16) + (h / 32) * (w / 32);
    }
    return OBB_OK;
}

int obb_forward(obb_ctx *ctx, const uint8_t *tiles, int32_t B, int32_t h, int32_t w, float *head, obb_stream_t s) {
    return obb_forward_gate(ctx, tiles, B, h, w, head, nullptr, s);
}

int obb_forward_gate(obb_ctx *ctx, const uint8_t *tiles, int32_t B, int32_t h, int32_t w, float *head, float *cmax, obb_stream_t s) {
    OBB_REQUIRE(ctx, ctx && B >= 0, "obb_forward: bad arguments");
    if (B == 0) return OBB_OK;
    OBB_REQUIRE(ctx, tiles && head, "obb_forward: NULL buffer");
    Plan *P = nullptr;
    int rc = get_plan(ctx, h, w, &P);
    if (rc) return rc;
    // The batch is walked in sub-batches: bounds the activation slab (and keeps every 1-D launch inside 32-bit buffer offsets)
    // "microbatch" counts 416 x 416 tiles: smaller tiles get proportionally more per round (128 px: 11 264 -- the 10 764 tiles of the dual-scale map are ONE round of two 5382-tile chains --, at most 16 384) -- the same activation bytes and
    // launch sizes, instead of 1024-tile rounds whose 4 x 4 / 8 x 8 levels are 74-WG launches on a 256-CU chip.  (measured at 416 px,
    // B = 1024: rounds of 512 / 1024 -> 91.8 / 94.7 k tiles/s; 128 / 256: 67 / 79 k with the round-1 kernels)
    const int max_mb = (int)std::min<int64_t>(16384, (int64_t)ctx->opt.microbatch * std::max<int64_t>(1, (416 * 416 + (int64_t)h * w - 1) / ((int64_t)h * w)));
    rc = ensure_capacity(ctx, *P, std::min<int>(B, max_mb));
    if (rc) return rc;
    bool use_graph = ctx->opt.graph;
    {   // inside somebody else's capture (torch.cuda.graph around the registered op) the launches simply join that graph
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing((hipStream_t)s, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) use_graph = false;
    }
    hipStream_t st = (hipStream_t)s;
    // (equal rounds: 21 000 tiles of 128 px are 3 x 7000, not 10 240 + 10 240 + 520 -- a short round runs its small-map layers at a fraction of
    // the workgroups the chip holds)
    const int nrounds = (B + max_mb - 1) / max_mb, per_round = (B + nrounds - 1) / nrounds;
    for (int b0 = 0; b0 < B; b0 += per_round) {
        int nb = std::min<int>(per_round, B - b0);
        const uint8_t *tp = tiles + (int64_t)b0 * h * w * ctx->model->ch;
        float *hp = head + (int64_t)b0 * P->A * P->no_pad;
        float *cp = cmax ? cmax + (int64_t)b0 * P->A : nullptr;
        Plan::GraphKey key(nb, (const void *)tp, (void *)hp, (void *)cp);
        auto git = P->graphs.find(key);
        if (use_graph && git != P->graphs.end()) {
            OBB_HIP(ctx, hipGraphLaunch(git->second, st));
            continue;
        }
        if (P->seen.size() > 4096) P->seen.clear();  // keys are (batch, input pointer, output pointer): a caller that never repeats one must not grow this
        bool capture = use_graph && P->seen[key]++ >= 1;
        if (capture && P->graphs.size() >= 64) {  // cache full: drop the oldest half (insertion order), then capture the new key
            OBB_HIP(ctx, hipStreamSynchronize(st));
            while (P->graph_order.size() > 32) {
                auto it = P->graphs.find(P->graph_order.front());
                if (it != P->graphs.end()) { (void)hipGraphExecDestroy(it->second); P->graphs.erase(it); }
                P->graph_order.erase(P->graph_order.begin());
            }
        }
        if (capture && hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed) != hipSuccess) { (void)hipGetLastError(); capture = false; }
        rc = run_round(ctx, *P, tp, nb, hp, cp, st);
        if (capture) {
            hipGraph_t g = nullptr;
            hipError_t e = hipStreamEndCapture(st, &g);
            if (rc == OBB_OK && e == hipSuccess && g) {
                hipGraphExec_t ge = nullptr;
                if (hipGraphInstantiate(&ge, g, nullptr, nullptr, 0) == hipSuccess) {
                    P->graphs[key] = ge;
                    P->graph_order.push_back(key);
                    (void)hipGraphDestroy(g);
                    OBB_HIP(ctx, hipGraphLaunch(ge, st));
                    continue;
                }
                (void)hipGraphDestroy(g);
            }
            (void)hipGetLastError();
            if (rc) return rc;
            rc = run_round(ctx, *P, tp, nb, hp, cp, st);  // capture unavailable: run eagerly
        }
        if (rc) return rc;
    }
    return OBB_OK;
}

int obb_debug_plan(obb_ctx *ctx, int32_t h, int32_t w, char *buf, int64_t buf_bytes, int64_t *needed) {
    OBB_REQUIRE(ctx, ctx && needed, "obb_debug_plan: bad arguments");
    Plan *P = nullptr;
    int rc = get_plan(ctx, h, w, &P);
    if (rc) return rc;
    std::string out;
    char line[512];
    for (const Op &op : P->ops) {
        switch (op.type) {
            case OP_CONV32: {
                const Conv32Launch &L = op.c32;
                snprintf(line, sizeof line, "conv32 %s k%d s%d cin%d cout%d out%dx%d TH%d TW%d NI%d CK%d WC%d NC%d MFM%d dw%d tail%d vcat%d upacc%d lds%d macs%.0f\n", op.name.c_str(), L.ks,
                         L.stride, L.cin, L.cout, op.Ho, op.Wo, L.TH, L.TW, L.NI, L.CK, L.WC, L.NC, L.MFM, L.dw, L.tail_cout, op.vin ? 1 : 0, op.upacc ? 1 : 0, (int)conv32_lds_bytes(L),
                         op.macs);
                break;
            }
            case OP_CONV: {
                const ConvLaunch &L = op.conv;
                const int grid_x = op.one_d ? -(op.Ho * op.Wo) : L.tiles_x * L.tiles_y;  // negative: pixels per image of a 1-D launch
                const int grid_y = (L.cout + 16 * L.NF - 1) / (16 * L.NF);
                const int ni = (!op.one_d && ctx->model->o.nitile) ? conv_ni_supported(L) : 1;  // (decided per launch: images per tile on the small maps)
                snprintf(line, sizeof line, "conv %s k%d s%d cin%d cout%d out%dx%d TH%d TW%d MF%d NF%d CK%d NI%d gx%d gy%d lds%d macs%.0f\n", op.name.c_str(), L.ks,
                         L.stride, L.cin, L.cout, op.Ho, op.Wo, ni > 1 ? op.Ho : L.TH, ni > 1 ? op.Wo : L.TW, L.MF, L.NF, L.CK, ni, grid_x, grid_y, (int)conv_lds_bytes(L), op.macs);
                break;
            }
            case OP_DW: snprintf(line, sizeof line, "dwconv %s c%d out%dx%d macs%.0f\n", op.name.c_str(), op.in.C, op.Ho, op.Wo, op.macs); break;
            case OP_C3KIMG: snprintf(line, sizeof line, "c3kimg %s c%d out%dx%d macs%.0f\n", op.name.c_str(), op.in.C, op.Ho, op.Wo, op.macs); break;
            case OP_DWPW: snprintf(line, sizeof line, "dwpw %s c%d tail%d out%dx%d macs%.0f\n", op.name.c_str(), op.dwpw.cin, op.dwpw.tail_cout, op.Ho, op.Wo, op.macs); break;
            case OP_BNECK: snprintf(line, sizeof line, "bneck %s c%d co%d out%dx%d rows4 macs%.0f\n", op.name.c_str(), op.bneck.C, op.bneck.CO, op.Ho, op.Wo, op.macs); break;
            case OP_SPPF: snprintf(line, sizeof line, "pool %s c%d out%dx%d x3 macs0\n", op.name.c_str(), op.in.C, op.Ho, op.Wo); break;
            case OP_POOL: snprintf(line, sizeof line, "pool %s c%d out%dx%d macs0\n", op.name.c_str(), op.in.C, op.Ho, op.Wo); break;
            case OP_UP: snprintf(line, sizeof line, "upsample %s c%d out%dx%d macs0\n", op.name.c_str(), op.in.C, op.Ho, op.Wo); break;
            case OP_PW32:
                snprintf(line, sizeof line, "pw32 %s k1 s1 cin%d cout%d out%dx%d waves%d raw%d lds%d macs%.0f\n", op.name.c_str(), op.pw32.cin, op.pw32.cout, op.Ho, op.Wo,
                         op.pw32.cin * 256 <= 80 * 1024 ? 8 : 16, op.pw32.raw ? 1 : 0, op.pw32.cin * 256, op.macs);
                break;
            case OP_C3K2F32: {
                int th, tw;
                c3k2f32_tile(op.H, op.W, th, tw);
                snprintf(line, sizeof line, "c3k2f32 %s c%d co%d out%dx%d TH%d TW%d macs%.0f\n", op.name.c_str(), op.c3k2f.C, op.c3k2f.CO, op.Ho, op.Wo, th, tw, op.macs);
                break;
            }
            case OP_STEM32:
                snprintf(line, sizeof line, "stem32 %s k3 s2 cin%d cout%d out%dx%d rows%d macs%.0f\n", op.name.c_str(), op.stem32.cin, op.stem32.cout, op.Ho, op.Wo, 4, op.macs);
                break;
            case OP_STEM:
                snprintf(line, sizeof line, "stem %s k3 s2 cin%d cout%d out%dx%d rows%d macs%.0f\n", op.name.c_str(), op.stem.cin, op.stem.cout, op.Ho, op.Wo, 4, op.macs);
                break;
            case OP_FRONT: snprintf(line, sizeof line, "front %s cin%d out%dx%d macs%.0f\n", op.name.c_str(), op.front.cin, op.Ho, op.Wo, op.macs); break;
            case OP_ATTN: snprintf(line, sizeof line, "attn %s N%d nh%d macs%.0f\n", op.name.c_str(), op.N, op.nh, op.macs); break;
        }
        out += line;
    }
    snprintf(line, sizeof line, "total_macs %.0f bytes_per_img %lld nbufs %zu nops %zu\n", P->macs_per_img, (long long)P->bytes_per_img, P->bufs.size(),
             P->ops.size());
    out += line;
    *needed = (int64_t)out.size() + 1;
    if (buf && buf_bytes >= *needed) memcpy(buf, out.c_str(), out.size() + 1);
    return OBB_OK;
}

int obb_debug_activation(obb_ctx *ctx, int32_t h, int32_t w, int32_t B, const char *name, float *out, int64_t max_elems,
                         int64_t *n_elems, int32_t *shape_hwc_host, obb_stream_t s) {
    OBB_REQUIRE(ctx, ctx && name && n_elems, "obb_debug_activation: bad arguments");
    Plan *P = nullptr;
    int rc = get_plan(ctx, h, w, &P);
    if (rc) return rc;
    auto it = P->named.find(name);
    if (it == P->named.end() || it->second.buf < 0) return set_error(ctx, OBB_ERR_INVALID, "obb_debug_activation: no activation named '%s'", name);
    OBB_REQUIRE(ctx, B <= P->cap, "obb_debug_activation: run obb_forward with B >= %d first", B);
    const Slice &sl = it->second;
    const Buf &b = P->bufs[sl.buf];
    int64_t n = (int64_t)B * b.H * b.W * sl.C;
    *n_elems = n;
    if (shape_hwc_host) { shape_hwc_host[0] = b.H; shape_hwc_host[1] = b.W; shape_hwc_host[2] = sl.C; }
    if (!out) return OBB_OK;
    OBB_REQUIRE(ctx, max_elems >= n, "obb_debug_activation: output too small (%lld < %lld)", (long long)max_elems, (long long)n);
    const int64_t hw = (int64_t)b.H * b.W;
    const int64_t d_bs = b.blk > 0 ? hw * b.blk : b.per_img(), d_ps = b.blk > 0 ? (int64_t)P->cap * hw * b.blk : 0;
    if (b.f32)
        hipLaunchKernelGGL(k_f32_slice_copy, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)s, (const float *)b.p, (int64_t)b.per_img(), b.C, sl.co, sl.C, hw,
                           B, out, b.blk32);
    else if (ctx->model->f16)
        hipLaunchKernelGGL(k_half_slice_to_f32<true>, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)s, (const bf16_t *)b.p, d_bs, b.C,
                           sl.co, sl.C, hw, B, out, b.blk, d_ps);
    else
        hipLaunchKernelGGL(k_half_slice_to_f32<false>, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)s, (const bf16_t *)b.p, d_bs, b.C,
                           sl.co, sl.C, hw, B, out, b.blk, d_ps);
    OBB_LAUNCH_CHECK(ctx);
    return OBB_OK;
}

}  // extern "C"
