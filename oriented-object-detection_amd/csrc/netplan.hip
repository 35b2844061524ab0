// Plan builder: weight-blob parser and the YOLO11-OBB graph (ultralytics==8.3.196 yolo11-obb.yaml) lowered,
// per input shape, to a flat list of fused kernel launches.  Concat/chunk/split never materialise: every producer writes into the
// channel slice of the buffer its consumer reads.  Builder::build() is the topology; one emitter per kernel family chooses the
// launch form of a layer, packs and uploads its weights and records the op (engine.hip binds the buffers and issues it).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "plan.h"

namespace obb {

// ---------------------------------------------------------------------------------------------- blob parsing ("OBBW" v1)
#pragma pack(push, 1)
struct BlobHeader { char magic[4]; uint32_t version, nrec; int32_t nc, ch; float width, depth; int32_t max_ch, reg_max; char scale[8]; };
struct BlobRec { char name[64]; int32_t c1, c2, k, s, g, act; uint64_t w_off, b_off; };
#pragma pack(pop)

int parse_blob(obb_ctx *ctx, Model &M) {
    const size_t n = M.blob.size();
    if (n < sizeof(BlobHeader)) return set_error(ctx, OBB_ERR_FORMAT, "weight blob too small (%zu bytes)", n);
    BlobHeader H;
    memcpy(&H, M.blob.data(), sizeof H);
    if (memcmp(H.magic, "OBBW", 4) != 0 || H.version != 1) return set_error(ctx, OBB_ERR_FORMAT, "bad weight blob magic/version");
    if (H.reg_max != kRegMax) return set_error(ctx, OBB_ERR_FORMAT, "reg_max %d unsupported", H.reg_max);
    if (H.ch != 3 && H.ch != 4) return set_error(ctx, OBB_ERR_FORMAT, "input channels %d unsupported (3 or 4)", H.ch);
    if (H.nc < 1 || H.nc > 1024) return set_error(ctx, OBB_ERR_FORMAT, "nc %d out of range", H.nc);
    M.nc = H.nc; M.ch = H.ch; M.width = H.width; M.depth = H.depth; M.max_ch = H.max_ch;
    M.scale = std::string(H.scale, strnlen(H.scale, 8));
    size_t tbl = sizeof(BlobHeader);
    if ((size_t)H.nrec > (n - tbl) / sizeof(BlobRec)) return set_error(ctx, OBB_ERR_FORMAT, "record table truncated");
    for (uint32_t i = 0; i < H.nrec; ++i) {
        BlobRec R;
        memcpy(&R, M.blob.data() + tbl + i * sizeof(BlobRec), sizeof R);
        ConvRecord c;
        c.name = std::string(R.name, strnlen(R.name, 64));
        c.c1 = R.c1; c.c2 = R.c2; c.k = R.k; c.s = R.s; c.g = R.g; c.act = R.act;
        if (c.c1 <= 0 || c.c2 <= 0 || c.c1 > 8192 || c.c2 > 8192 || (c.k != 1 && c.k != 3) || (c.s != 1 && c.s != 2) || c.g <= 0 || c.c1 % c.g)
            return set_error(ctx, OBB_ERR_FORMAT, "record %s: unsupported conv shape", c.name.c_str());
        const size_t wn = (size_t)c.c2 * (c.c1 / c.g) * c.k * c.k * 4, bn = (size_t)c.c2 * 4;  // <= 8192 * 8192 * 36: no overflow
        // subtraction forms: an offset near 2^64 must not wrap past the end check
        if (R.w_off % 4 || R.b_off % 4 || R.w_off > n || wn > n - R.w_off || R.b_off > n || bn > n - R.b_off)
            return set_error(ctx, OBB_ERR_FORMAT, "record %s: data out of range", c.name.c_str());
        c.w = reinterpret_cast<const float *>(M.blob.data() + R.w_off);
        c.b = reinterpret_cast<const float *>(M.blob.data() + R.b_off);
        M.recs[c.name] = c;
    }
    M.nrec_blob = (int)M.recs.size();
    return OBB_OK;
}

// columns [c0, c0 + nc) of a 1x1 record's [cout][cin] matrix as a dense [cout][nc] one
static std::vector<float> split_cols(const float *w, int cout, int cin, int c0, int nc) {
    std::vector<float> o((size_t)cout * nc);
    for (int co = 0; co < cout; ++co) std::copy(w + (size_t)co * cin + c0, w + (size_t)co * cin + c0 + nc, o.begin() + (size_t)co * nc);
    return o;
}

// ---------------------------------------------------------------------------------------------- graph builder
static int make_divisible(double x, int d) { return (int)std::ceil(x / d) * d; }
static int out_dim(int in, int k, int s) { return (in + 2 * (k / 2) - k) / s + 1; }  // "same" padding k / 2
// an activated stride-1 dense conv of exactly this shape (what the multi-layer kernels are written for)
static bool rec_is(const ConvRecord *q, int k, int c1, int c2) { return q->k == k && q->s == 1 && q->g == 1 && q->act && q->c1 == c1 && q->c2 == c2; }

struct Builder {
    obb_ctx *ctx;
    Model &M;
    Plan &P;
    int err = OBB_OK;
    bool use_front = false;  // model.0 + model.1 + model.2.cv1 run as one launch (front.hip)

    int ch(int c) const { return make_divisible(std::min(c, M.max_ch) * (double)M.width, 8); }
    int reps(int n) const { return n > 1 ? std::max((int)std::lround(n * (double)M.depth), 1) : n; }

    int buf(int H, int W, int C, const std::string &name, bool f32 = false, int blk = 0, bool blk32 = false) {
        Buf b;
        b.H = H; b.W = W; b.C = C; b.f32 = f32 || M.f32; b.name = name;
        if (!M.f32 && blk >= 16 && (blk & (blk - 1)) == 0 && C % blk == 0 && C > blk) b.blk = blk;
        if (M.f32 && blk32 && M.o.blk32 && M.o.tail && C % 8 == 0 && C > 8) b.blk32 = 8;
        P.bufs.push_back(b);
        return (int)P.bufs.size() - 1;
    }
    int vbuf(int H, int W, Slice up_src, Slice skip, const std::string &name) {
        Buf b;
        b.H = H; b.W = W; b.C = up_src.C + skip.C; b.f32 = false; b.name = name; b.virt = true;
        b.va_buf = up_src.buf; b.va_co = up_src.co; b.va_C = up_src.C; b.vb_buf = skip.buf; b.vb_co = skip.co; b.vb_C = skip.C;
        P.bufs.push_back(b);
        return (int)P.bufs.size() - 1;
    }
    Slice whole(int b) const { return Slice{b, 0, P.bufs[b].C}; }
    Slice sub(int b, int co, int C) const { return Slice{b, co, C}; }

    const ConvRecord *rec(const std::string &name) {
        auto it = M.recs.find(name);
        if (it == M.recs.end()) {
            if (!err) err = set_error(ctx, OBB_ERR_FORMAT, "weight blob has no record '%s'", name.c_str());
            return nullptr;
        }
        return &it->second;
    }

    template <typename T>
    T *upload(const std::vector<T> &v) {
        void *d = nullptr;
        if (hipMalloc(&d, v.size() * sizeof(T) + 256) != hipSuccess) {
            if (!err) err = set_error(ctx, OBB_ERR_HIP, "hipMalloc for weights failed");
            return nullptr;
        }
        P.dev_allocs.push_back(d);
        if (hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) {
            if (!err) err = set_error(ctx, OBB_ERR_HIP, "weight upload failed");
            return nullptr;
        }
        return (T *)d;
    }

    // bias of `r` (through `perm`: logical cout -> source row), zero-padded to `floats` (0: the (c2 + 63) / 64 * 64 + 64 rule of the conv
    // families, whose epilogues read whole 64-float groups); kernels that index their bias differently pass the size they expect
    const float *bias_padded(const ConvRecord *r, const int *perm = nullptr, size_t floats = 0) {
        std::vector<float> b(floats ? floats : ((size_t)r->c2 + 63) / 64 * 64 + 64, 0.f);
        for (int c = 0; c < r->c2; ++c) b[c] = r->b[perm ? perm[c] : c];
        return upload(b);
    }
    // depthwise 3x3 taps of `r` as [9][C] (+ 8 elements of padding), 16-bit storage / fp32
    const bf16_t *dw_taps16(const ConvRecord *r, int C) {
        std::vector<bf16_t> w((size_t)9 * C + 8, 0);
        for (int c = 0; c < C; ++c)
            for (int t = 0; t < 9; ++t) w[(size_t)t * C + c] = host_to_half(r->w[(size_t)c * 9 + t], M.f16);
        return upload(w);
    }
    const float *dw_taps32(const ConvRecord *r, int C) {
        std::vector<float> w((size_t)9 * C + 8, 0.f);
        for (int c = 0; c < C; ++c)
            for (int t = 0; t < 9; ++t) w[(size_t)t * C + c] = r->w[(size_t)c * 9 + t];
        return upload(w);
    }

    // records a finished op; `key` (optional): the layer whose activation `s` holds once the op has run (obb_debug_activation)
    void emit(const Op &op, const std::string &key = std::string(), Slice s = Slice()) {
        P.macs_per_img += op.macs;
        P.ops.push_back(op);
        if (!key.empty()) P.named[key] = s;
    }
    // a conv op with its optional fused 1x1 `rt`: the output slice belongs to `rt` if that has an activation (a tensor of the graph), to
    // nobody if it writes head rows, and to the conv itself without a tail
    void emit_conv(const Op &op, const ConvRecord *r, const ConvRecord *rt) { emit(op, !rt ? r->name : rt->act ? rt->name : std::string(), op.out); }

    // true if the 1x1 conv `tail_name`, whose only producer is the conv `name`, can run inside the producer's launch (the producer's own
    // output then never exists).  act16 = false: a plain 1x1 writing head rows (conv.hip TAIL kernels); act16 = true: an activated 1x1
    // with a 16-bit output of its own behind a 3x3 conv that holds all of its output channels in one workgroup (stride-2 backbone
    // conv -> cv1 of the next C3k2 block)
    bool tail_ok(const std::string &name, const std::string &tail_name, int Hin, int Win, bool act16 = false) {
        if (!M.o.tail || (act16 && !M.o.tail16)) return false;
        const ConvRecord *r = rec(name), *r2 = rec(tail_name);
        if (!r || !r2 || err) return false;
        if (r->g != 1 || r2->g != 1 || r2->k != 1 || r2->s != 1 || r2->c1 != r->c2) return false;
        if (act16 ? (r->k != 3 || !r2->act || !r->act) : (r2->act || r->s != 1)) return false;
        const int Ho = out_dim(Hin, r->k, r->s), Wo = out_dim(Win, r->k, r->s);
        if (M.f32) return conv32_tail_supported(plan_conv32(r->k, r->s, r->c1, r->c2, Ho, Wo, false), r->c2, r2->c2);
        ConvTiling t = plan_conv(r->k, r->s, r->c1, r->c2, Ho, Wo, M.o.pair);
        return conv_tail_supported(r->k, t.MF, t.NF, r->c2, r2->c2, act16, act16 ? t.TH : 0);
    }

    // true if model.0 -> model.1 -> model.2.cv1 can run as ONE launch (front.hip): the n-scale widths on tiles whose sides are multiples of 52
    bool front_ok(int h, int w) {
        if (M.f32 || !M.o.front || !M.o.stem || !M.o.tail || !M.o.tail16) return false;
        const ConvRecord *r0 = rec("model.0"), *r1 = rec("model.1"), *r2 = rec("model.2.cv1");
        if (!r0 || !r1 || !r2 || err) return false;
        if (r0->g != 1 || r1->g != 1 || r2->g != 1 || r0->k != 3 || r1->k != 3 || r2->k != 1 || r0->s != 2 || r1->s != 2 || r2->s != 1 || !r0->act || !r1->act || !r2->act) return false;
        if (r0->c1 != M.ch || r1->c1 != r0->c2 || r2->c1 != r1->c2) return false;
        return front_supported(M.ch, r0->c2, r1->c2, r2->c2, h, w) && stem_scale_is_exact(M.f16);
    }
    void front(Slice out, int h, int w) {
        const ConvRecord *r0 = rec("model.0"), *r1 = rec("model.1"), *r2 = rec("model.2.cv1");
        if (!r0 || !r1 || !r2 || err) return;
        Op op;
        op.type = OP_FRONT; op.name = "model.0+model.1+model.2.cv1"; op.in = Slice{-1, 0, M.ch}; op.out = out;
        op.H = h; op.W = w; op.Ho = h / 4; op.Wo = w / 4;
        FrontLaunch &L = op.front;
        L.Hin = h; L.Win = w; L.cin = M.ch; L.f16 = M.f16;
        L.w0 = upload(pack_stem_weights(r0->w, r0->c2, M.ch, M.ch == 3, M.f16));
        const ConvTiling t1{13, 13, 3, 2, 16}, t2{1, 1, 1, 2, 32};
        L.w1 = upload(pack_conv_weights(r1->w, r1->c2, r1->c1, 3, t1, nullptr, 0, M.f16));
        L.w2 = upload(pack_conv_weights(r2->w, r2->c2, r2->c1, 1, t2, nullptr, 0, M.f16));
        L.b0 = bias_padded(r0); L.b1 = bias_padded(r1); L.b2 = bias_padded(r2);
        op.macs = (double)(h / 2) * (w / 2) * r0->c2 * M.ch * 9 + (double)(h / 4) * (w / 4) * ((double)r1->c2 * r1->c1 * 9 + (double)r2->c2 * r2->c1);
        emit(op, "model.2.cv1", out);
    }

    // generic dense conv (groups == 1).  in.buf == -1 -> the uint8 network input.  `tail_name` (optional): the 1x1 conv that runs fused
    // behind this layer (tail_ok): `out` is then the slice the tail writes and this layer's own output is never written.
    // Checks the record against the graph and the layouts the layer may touch, then hands over to the first kernel family that takes it.
    void conv(const std::string &name, Slice in, int Hin, int Win, Slice out, Slice res = Slice(), int head_level = -1,
              const int *perm = nullptr, const char *tail_name = nullptr) {
        const ConvRecord *r = rec(name);
        if (!r || err) return;
        if (use_front && name == "model.1" && tail_name && std::string(tail_name) == "model.2.cv1") { front(out, Hin * 2, Win * 2); return; }
        bool in_u8 = in.buf < 0;
        int cin = in_u8 ? M.ch : in.C;
        if (r->g != 1 || r->c1 != cin || (!tail_name && r->c2 != out.C)) {
            err = set_error(ctx, OBB_ERR_FORMAT, "record %s: shape (%d->%d, g%d) does not match the graph (%d->%d)", name.c_str(), r->c1,
                            r->c2, r->g, cin, out.C);
            return;
        }
        Op op;
        op.type = OP_CONV; op.name = name; op.in = in; op.out = out; op.res = res; op.head_level = head_level;
        if (!in_u8 && P.bufs[in.buf].virt) {
            const Buf &vb = P.bufs[in.buf];
            if (r->k != 1 || in.co != 0 || in.C != vb.C || vb.va_C % 64 || cin < 128) {
                err = set_error(ctx, OBB_ERR_STATE, "layer %s cannot read the virtual concat '%s'", name.c_str(), vb.name.c_str());
                return;
            }
            op.vin = true;
        }
        op.H = Hin; op.W = Win;
        op.Ho = out_dim(Hin, r->k, r->s);
        op.Wo = out_dim(Win, r->k, r->s);
        op.one_d = (r->k == 1);
        op.macs = (double)op.Ho * op.Wo * r->c2 * cin * r->k * r->k;
        const bool stem_in = in_u8 && M.o.stem && !perm && head_level < 0 && !res.C;  // the network input layer, nothing fused around it
        if (M.f32 && stem_in && !tail_name && stem32_supported(cin, r->c2, r->k, r->s, Hin, Win)) return emit_stem32(op, r);
        if (M.f32 && !in_u8 && !op.vin && P.bufs[in.buf].blk32 && r->k != 3) {
            err = set_error(ctx, OBB_ERR_STATE, "layer %s cannot read the channel-blocked buffer '%s'", name.c_str(), P.bufs[in.buf].name.c_str());
            return;
        }
        if (M.f32 && ((res.C && P.bufs[res.buf].blk32) || (tail_name && out.buf >= 0 && P.bufs[out.buf].blk32))) {
            err = set_error(ctx, OBB_ERR_STATE, "layer %s: residual / fused-1x1 output in a channel-blocked buffer", name.c_str());
            return;
        }
        if (op.vin && !perm && !tail_name && head_level < 0 && !res.C && upacc_ok(r, P.bufs[in.buf], Hin, Win)) return emit_upacc(op, r);
        if (M.f32 && M.o.pw32 && r->k == 1 && !in_u8 && !op.vin && !tail_name && head_level < 0 && !P.bufs[in.buf].blk32 && pw32_supported(cin, r->c2) &&
            !(res.C && P.bufs[res.buf].blk32))
            return emit_pw32(op, r, perm);
        if (M.f32) return emit_conv32(op, r, perm, tail_name);
        if (stem_in && stem_supported(cin, r->c2, r->k, r->s, Hin, Win) && r->act && stem_scale_is_exact(M.f16)) return emit_stem16(op, r);
        emit_conv16(op, r, perm, tail_name);
    }

    // The emitters below get the op as conv() validated it (name, slices, dims, one_d, vin, macs of the layer itself); r->c1 is the input
    // channel count (the uint8 tile's M.ch included).
    // fp32 mode, network input layer as row stripes (f32path.hip k_stem_f32)
    void emit_stem32(Op op, const ConvRecord *r) {
        op.type = OP_STEM32;
        Stem32Launch &S = op.stem32;
        S.Hin = op.H; S.Win = op.W; S.cin = r->c1; S.cout = r->c2; S.act = r->act;
        S.wpk = upload(pack_stem32_weights(r->w, r->c2, r->c1, M.ch == 3));
        S.bias = bias_padded(r);
        S.lut = M.lut32_dev;
        emit(op, r->name, op.out);
    }
    // fp32 mode, 1x1 with >= 64 input channels: weights resident in LDS, activations straight from global memory into the MFMA operand (pw32.hip)
    void emit_pw32(Op op, const ConvRecord *r, const int *perm) {
        op.type = OP_PW32;
        Pw32Launch &L = op.pw32;
        L.cin = r->c1; L.cout = r->c2; L.act = r->act;
        L.wpk = upload(pack_pw32_weights(r->w, r->c2, r->c1, perm));  // (k = 1: OIHW is [cout][cin])
        L.bias = bias_padded(r, perm);
        emit(op, r->name, op.out);
    }
    // fp32 mode, the 1x1 `r` over the virtual concat `vb` = [Upsample x2 of va | vb] as TWO launches ("upacc"): a 1x1 commutes with nearest
    // upsampling, so the product over va's channels is computed once per coarse pixel and the fine launch starts its accumulators from it
    // (bit for bit what the one-launch VCAT form computes: see AINIT in k_conv_f32).  The shapes that have both kernels:
    bool upacc_ok(const ConvRecord *r, const Buf &vb, int H, int W) const {
        if (!M.f32 || !M.o.upacc || !M.o.pw32 || !M.o.nc2 || r->k != 1 || vb.va_C % 16 || (H & 1) || (W & 1) || P.bufs[vb.va_buf].blk32) return false;
        if (!pw32_supported(vb.va_C, r->c2) || vb.vb_C < 64 || r->c2 % 32) return false;
        const Conv32Tiling t = plan_conv32(1, 1, vb.vb_C, r->c2, H, W, false, false, true);
        return t.NC == 2 && t.WC == 2 && t.MFM == 3 && vb.vb_C % t.CK == 0;
    }
    void emit_upacc(Op op, const ConvRecord *r) {
        const Buf vb = P.bufs[op.in.buf];
        const int up_c = vb.va_C, sk = vb.vb_C, Hc = op.H / 2, Wc = op.W / 2;
        const int part = buf(Hc, Wc, r->c2, r->name + ".up", true);  // the raw fp32 accumulators, plain NHWC at the coarse resolution
        Op oc;
        oc.type = OP_PW32; oc.name = r->name + ".up"; oc.in = Slice{vb.va_buf, vb.va_co, up_c}; oc.out = whole(part);
        oc.H = oc.Ho = Hc; oc.W = oc.Wo = Wc; oc.one_d = true;
        oc.pw32.cin = up_c; oc.pw32.cout = r->c2; oc.pw32.act = 0; oc.pw32.raw = true;
        oc.pw32.wpk = upload(pack_pw32_weights(split_cols(r->w, r->c2, r->c1, 0, up_c).data(), r->c2, up_c, nullptr));
        oc.macs = (double)Hc * Wc * r->c2 * up_c;
        emit(oc);
        op.type = OP_CONV32; op.upacc = true; op.ini = whole(part);
        op.macs = (double)op.Ho * op.Wo * r->c2 * sk;
        Conv32Launch &L = op.c32;
        const Conv32Tiling t = plan_conv32(1, 1, sk, r->c2, op.Ho, op.Wo, false, false, true);
        L.ks = 1; L.stride = 1; L.cin = sk; L.cout = r->c2; L.act = r->act;
        L.set_tiling(t);
        L.Hin = L.Hout = op.H; L.Win = L.Wout = op.W; L.tiles_y = 1; L.tiles_x = 1;  // (1-D: bound per sub-batch)
        L.wpk = upload(pack_conv32_weights(split_cols(r->w, r->c2, r->c1, up_c, sk).data(), r->c2, sk, 1, t, nullptr, false));
        L.bias = bias_padded(r);
        emit(op, r->name, op.out);
    }

    // fp32-arithmetic mode: exact-f32 MFMA kernels (f32path.hip)
    void emit_conv32(Op op, const ConvRecord *r, const int *perm, const char *tail_name) {
        const bool in_u8 = op.in.buf < 0;
        op.type = OP_CONV32;
        Conv32Launch &L = op.c32;
        const Conv32Tiling t = plan_conv32(r->k, r->s, r->c1, r->c2, op.Ho, op.Wo, in_u8, op.vin, M.o.nc2 && !tail_name);
        L.ks = r->k; L.stride = r->s; L.cin = r->c1; L.cout = r->c2; L.act = r->act; L.in_u8 = in_u8; L.flip_bgr = (in_u8 && M.ch == 3);
        L.set_tiling(t); L.NC = std::max(1, t.NC);
        L.Hin = op.H; L.Win = op.W; L.Hout = op.Ho; L.Wout = op.Wo;
        L.tiles_y = (op.Ho + t.TH - 1) / t.TH; L.tiles_x = (op.Wo + t.TW - 1) / t.TW;
        if (op.vin && (P.bufs[op.in.buf].va_C % t.CK || (t.WC != 4 && t.NC != 2))) { err = set_error(ctx, OBB_ERR_STATE, "layer %s cannot read the virtual concat in fp32 mode", op.name.c_str()); return; }
        L.wpk = upload(pack_conv32_weights(r->w, r->c2, r->c1, r->k, t, perm, in_u8));
        L.bias = bias_padded(r, perm);
        L.lut = M.lut32_dev;
        const ConvRecord *r2 = tail_name ? rec(tail_name) : nullptr;
        if (tail_name) {  // `out` is the slice the tail writes (head rows, or the cv1 output of a C3k2 block)
            if (!r2 || err) return;
            if (!conv32_tail_supported(t, r->c2, r2->c2) || (r2->act && (r2->c2 != op.out.C || op.head_level >= 0))) {
                err = set_error(ctx, OBB_ERR_STATE, "fused 1x1 %s: no fp32 kernel for this pair", tail_name);
                return;
            }
            attach_tail32(op, r2);
        }
        emit_conv(op, r, r2);
    }
    // fused trailing 1x1 `rt` behind a k_conv_f32 launch (plain or depthwise-prologue form); the caller has checked that the pair has a kernel
    void attach_tail32(Op &op, const ConvRecord *rt) {
        Conv32Launch &L = op.c32;
        const Conv32Tiling t2{1, 1, L.cout, 1, 1, 1};
        L.tail_w = upload(pack_conv32_weights(rt->w, rt->c2, L.cout, 1, t2, nullptr, false));
        L.tail_b = bias_padded(rt);
        L.tail_cout = rt->c2; L.tail_act = rt->act;
        op.name += "+" + rt->name;
        if (op.head_level >= 0 && op.out.buf == -2 && op.out.co == 4 * kRegMax && rt->c2 <= 16 && !rt->act) { op.emit_cmax = true; P.cmax_mask |= 1 << op.head_level; }
        op.macs += (double)op.Ho * op.Wo * rt->c2 * L.cout;
    }
    // 16-bit modes, network input layer as row stripes (stem.hip)
    void emit_stem16(Op op, const ConvRecord *r) {
        op.type = OP_STEM;
        StemLaunch &S = op.stem;
        S.Hin = op.H; S.Win = op.W; S.cin = r->c1; S.cout = r->c2; S.act = r->act; S.f16 = M.f16;
        S.wpk = upload(pack_stem_weights(r->w, r->c2, r->c1, M.ch == 3, M.f16));
        S.bias = bias_padded(r);
        emit(op, r->name, op.out);
    }
    // 16-bit modes: implicit-GEMM MFMA kernels (conv.hip)
    void emit_conv16(Op op, const ConvRecord *r, const int *perm, const char *tail_name) {
        const bool in_u8 = op.in.buf < 0;
        ConvTiling t = plan_conv(r->k, r->s, r->c1, r->c2, op.Ho, op.Wo, M.o.pair);
        if (in_u8) t.CK = 8;
        ConvLaunch &L = op.conv;
        L.ks = r->k; L.stride = r->s; L.cin = r->c1; L.cout = r->c2; L.act = r->act;
        L.in_u8 = in_u8; L.out_f32 = op.head_level >= 0 && !tail_name; L.flip_bgr = (in_u8 && M.ch == 3); L.f16 = M.f16;
        L.TH = t.TH; L.TW = t.TW; L.MF = t.MF; L.NF = t.NF; L.CK = t.CK;
        L.Hin = op.H; L.Win = op.W; L.Hout = op.Ho; L.Wout = op.Wo;
        L.tiles_y = (op.Ho + t.TH - 1) / t.TH; L.tiles_x = (op.Wo + t.TW - 1) / t.TW;
        L.wpk = upload(pack_conv_weights(r->w, r->c2, r->c1, r->k, t, perm, in_u8, M.f16));
        L.bias = bias_padded(r, perm);
        L.lut = M.lut_dev;
        const ConvRecord *r2 = tail_name ? rec(tail_name) : nullptr;
        if (tail_name) {  // `out` is the head slice of the tail's output, or (tail with SiLU: cv1 of a C3k2 block) its 16-bit output
            if (!r2 || err) return;
            if (r2->act && (r2->c2 != op.out.C || op.head_level >= 0)) {
                err = set_error(ctx, OBB_ERR_STATE, "fused cv1 %s: output slice does not match", tail_name);
                return;
            }
            attach_tail16(op, r2);
        }
        emit_conv(op, r, r2);
    }
    void attach_tail16(Op &op, const ConvRecord *rt) {
        ConvLaunch &L = op.conv;
        L.tail_act16 = rt->act != 0;  // cv1 of a C3k2 block: SiLU, 16-bit output of its own in `out`
        const int nf2 = rt->c2 <= 16 ? 1 : (L.tail_act16 && rt->c2 <= 32 ? 2 : 4);
        ConvTiling t2{1, 1, 1, nf2, L.cout};
        L.tail_wpk = upload(pack_conv_weights(rt->w, rt->c2, L.cout, 1, t2, nullptr, 0, M.f16));
        L.tail_bias = bias_padded(rt);
        L.tail_cout = rt->c2;
        op.name += "+" + rt->name;
        op.macs += (double)op.Ho * op.Wo * rt->c2 * L.cout;
    }

    void dwconv(const std::string &name, Slice in, int H, int W, Slice out, Slice res = Slice()) {
        const ConvRecord *r = rec(name);
        if (!r || err) return;
        if (r->g != r->c1 || r->c1 != r->c2 || r->k != 3 || r->s != 1 || r->c1 != in.C || out.C != in.C) {
            err = set_error(ctx, OBB_ERR_FORMAT, "record %s: not a depthwise 3x3 matching the graph", name.c_str());
            return;
        }
        if (M.f32 && (P.bufs[in.buf].blk32 || P.bufs[out.buf].blk32)) { err = set_error(ctx, OBB_ERR_STATE, "depthwise layer %s on a channel-blocked buffer", name.c_str()); return; }
        const int C = in.C;
        Op op;
        op.type = OP_DW; op.name = name; op.in = in; op.out = out; op.res = res; op.H = H; op.W = W; op.Ho = H; op.Wo = W;
        op.act = r->act;
        if (M.f32) op.dw_w32 = dw_taps32(r, C);
        else op.dw_w = dw_taps16(r, C);
        op.dw_b = bias_padded(r, nullptr, (size_t)C + 8);  // (k_dwconv3: 8 channels per lane)
        op.macs = (double)H * W * C * 9;
        emit(op, name, out);
    }

    // what the two fused DWConv 3x3 `rd` -> Conv 1x1 `rp` [-> plain 1x1 `rt` into the head rows] forms ask of records and slices alike
    bool dwpw_shapes_ok(const ConvRecord *rd, const ConvRecord *rp, const ConvRecord *rt, Slice in, Slice out, int head_level) const {
        if (in.buf < 0 || P.bufs[in.buf].virt || rd->g != rd->c1 || rd->c1 != rd->c2 || rd->k != 3 || rd->s != 1 || rd->c1 != in.C || rp->g != 1 || rp->k != 1 || rp->s != 1 ||
            rp->c1 != in.C)
            return false;
        if (rt && (rt->g != 1 || rt->k != 1 || rt->s != 1 || rt->act || rt->c1 != rp->c2 || head_level < 0)) return false;
        return rt || (out.buf >= 0 && !P.bufs[out.buf].virt && out.C == rp->c2);
    }

    // fp32 mode: the pair (or triple) as ONE launch of k_conv_f32 (DW variant: the depthwise output exists only in LDS)
    bool dwpw32(const ConvRecord *rd, const ConvRecord *rp, const ConvRecord *rt, Op op) {
        const int H = op.H, W = op.W, C = op.in.C;
        const Conv32Tiling t = plan_dwpw32(C, rp->c2, H, W);
        if (t.TH == 0 || (rt && !conv32_tail_supported(t, rp->c2, rt->c2)) || (rt && rt->c2 > 16)) return false;
        op.type = OP_CONV32;
        Conv32Launch &L = op.c32;
        L.ks = 1; L.stride = 1; L.cin = C; L.cout = rp->c2; L.act = rp->act; L.dw = 1; L.dw_act = rd->act;
        L.set_tiling(t);
        L.Hin = L.Hout = H; L.Win = L.Wout = W;
        L.tiles_y = (H + t.TH - 1) / t.TH; L.tiles_x = 1;
        L.wpk = upload(pack_dwpw32_weights(rp->w, rp->c2, C, rd->w, rd->b, t));
        L.bias = bias_padded(rp);
        if (rt) attach_tail32(op, rt);
        emit_conv(op, rp, rt);
        return true;
    }

    // DWConv 3x3 `dwname` -> Conv 1x1 `pwname` [-> plain 1x1 `tailname` into the head tensor] as one launch: a stripe kernel (dwpw.hip)
    // in the 16-bit modes, dwpw32 in fp32 mode.  Returns false (nothing emitted) if the shapes have no kernel.
    bool dwpw(const std::string &dwname, const std::string &pwname, Slice in, int H, int W, Slice out, const char *tailname = nullptr, int head_level = -1) {
        const ConvRecord *rd = rec(dwname), *rp = rec(pwname), *rt = tailname ? rec(tailname) : nullptr;
        if (!(M.o.tail && M.o.dwpw) || !rd || !rp || (tailname && !rt) || err) return false;
        if (!dwpw_shapes_ok(rd, rp, rt, in, out, head_level)) return false;
        const int C = in.C;
        Op op;
        op.name = dwname + "+" + pwname; op.in = in; op.out = out;
        op.H = H; op.W = W; op.Ho = H; op.Wo = W; op.head_level = rt ? head_level : -1;
        op.macs = (double)H * W * (9.0 * C + (double)C * rp->c2);
        if (M.f32) return dwpw32(rd, rp, rt, op);
        if (P.bufs[in.buf].blk || (!rt && P.bufs[out.buf].blk) || !rd->act || !rp->act || !dwpw_supported(C, rp->c2, H, W, rt ? rt->c2 : 0)) return false;
        op.type = OP_DWPW;
        DwPwLaunch &L = op.dwpw;
        L.H = H; L.W = W; L.cin = C; L.f16 = M.f16;
        L.dw_w = dw_taps16(rd, C); L.dw_b = bias_padded(rd, nullptr, (size_t)C + 8);
        ConvTiling tp{1, 1, 1, 4, C};
        L.pw_w = upload(pack_conv_weights(rp->w, rp->c2, C, 1, tp, nullptr, 0, M.f16));
        L.pw_b = bias_padded(rp, nullptr, 64 + 64);  // (k_dwpw: at most 64 couts, read as whole 64-float groups)
        if (rt) {
            L.tail_cout = rt->c2;
            L.tail_w = upload(pack_dwpw_tail(rt->w, rt->c2, M.f16));
            L.tail_b = bias_padded(rt, nullptr, 64);  // (k_dwpw tail: at most 64 class logits)
            op.name += std::string("+") + tailname;
            op.macs += (double)H * W * rt->c1 * rt->c2;
        }
        emit_conv(op, rp, rt);
        return true;
    }

    void pool(Slice in, int H, int W, Slice out) {
        Op op; op.type = OP_POOL; op.name = "maxpool5"; op.in = in; op.out = out; op.H = H; op.W = W; op.Ho = H; op.Wo = W;
        emit(op);
    }
    void upsample(Slice in, int H, int W, Slice out) {
        Op op; op.type = OP_UP; op.name = "upsample2"; op.in = in; op.out = out; op.H = H; op.W = W; op.Ho = 2 * H; op.Wo = 2 * W;
        emit(op);
    }

    // Two sibling convs of the same kind on the same input (same k, stride, activation) as ONE conv whose weights are concatenated along
    // cout: `out` = [outputs of a | outputs of b].  Returns the name of the synthesised record ("" if the pair does not qualify).
    std::string merged_record(const std::string &na, const std::string &nb) {
        if (!M.o.hmerge) return "";
        const ConvRecord *a = rec(na), *b = rec(nb);
        if (!a || !b || err) return "";
        if (a->g != 1 || b->g != 1 || a->k != b->k || a->s != b->s || a->act != b->act || a->c1 != b->c1) return "";
        const std::string nm = na + "|" + nb;
        if (!M.recs.count(nm)) {
            auto &st = M.merged[nm];
            const size_t wa = (size_t)a->c2 * a->c1 * a->k * a->k, wb = (size_t)b->c2 * b->c1 * b->k * b->k;
            st.first.assign(a->w, a->w + wa);
            st.first.insert(st.first.end(), b->w, b->w + wb);
            st.second.assign(a->b, a->b + a->c2);
            st.second.insert(st.second.end(), b->b, b->b + b->c2);
            ConvRecord r = *a;
            r.name = nm; r.c2 = a->c2 + b->c2; r.w = st.first.data(); r.b = st.second.data();
            M.recs[nm] = r;
        }
        return nm;
    }

    // cv2name (optional): the closing 1x1 of the surrounding C3k2 block (over [y0 | in | out] of the concat buffer -> cv2out); returns
    // true if that conv was fused behind the Bottleneck (the caller then must not emit it)
    bool bottleneck(const std::string &name, Slice in, int H, int W, Slice out, double e, const char *cv2name = nullptr, Slice y0 = Slice(),
                    Slice cv2out = Slice()) {
        int c_ = (int)(out.C * e);
        if (M.o.bneck && in.buf >= 0 && in.buf == out.buf && P.bufs[in.buf].blk == in.C && in.C == out.C && c_ * 2 == in.C &&
            bneck_supported(in.C, H, W)) {
            const ConvRecord *r1 = rec(name + ".cv1"), *r2 = rec(name + ".cv2");
            if (!r1 || !r2 || err) return false;
            if (r1->k == 3 && r2->k == 3 && r1->s == 1 && r2->s == 1 && r1->g == 1 && r2->g == 1 && r1->act && r2->act && r1->c1 == in.C &&
                r1->c2 == c_ && r2->c1 == c_ && r2->c2 == in.C) {
                Op op;
                op.type = OP_BNECK; op.name = name; op.in = in; op.out = out; op.H = H; op.W = W; op.Ho = H; op.Wo = W;
                BneckLaunch &L = op.bneck;
                L.H = H; L.W = W; L.C = in.C; L.f16 = M.f16;
                ConvTiling t1{1, 1, 1, 1, in.C}, t2{1, 1, 1, in.C / 16, c_};
                L.w1pk = upload(pack_conv_weights(r1->w, c_, in.C, 3, t1, nullptr, 0, M.f16));
                L.w2pk = upload(pack_conv_weights(r2->w, in.C, c_, 3, t2, nullptr, 0, M.f16));
                L.bias1 = bias_padded(r1, nullptr, 128); L.bias2 = bias_padded(r2, nullptr, 128);  // (k_bneck: 128 floats each)
                op.macs = (double)H * W * 9.0 * in.C * c_ * 2;
                bool fused_cv2 = false;
                const ConvRecord *rc = cv2name ? rec(cv2name) : nullptr;
                if (rc && M.o.bneck_cv2 && rc->k == 1 && rc->s == 1 && rc->g == 1 && rc->act && rc->c1 == 3 * in.C && rc->c2 == cv2out.C && cv2out.buf >= 0 &&
                    !P.bufs[cv2out.buf].virt && y0.buf == in.buf && y0.C == in.C && y0.co + in.C == in.co && in.co + in.C == out.co &&
                    bneck_cv2_supported(in.C, rc->c2)) {
                    ConvTiling tc{1, 1, 1, rc->c2 / 16, in.C == 32 ? 96 : 32};
                    L.CO = rc->c2;
                    L.wc32pk = upload(pack_conv_weights(rc->w, rc->c2, rc->c1, 1, tc, nullptr, 0, M.f16));
                    if (in.C == 16) L.wc16pk = upload(pack_bneck_k16(rc->w, rc->c2, rc->c1, 32, M.f16));
                    L.biasc = bias_padded(rc, nullptr, 128 + 64);  // (k_bneck closing 1x1: up to 128 couts, read as whole 64-float groups)
                    op.name = name + "+" + cv2name;
                    op.out = cv2out; op.res = y0;  // res carries the y0 slice to the launch
                    op.macs += (double)H * W * rc->c1 * rc->c2;
                    fused_cv2 = true;
                }
                emit(op, fused_cv2 ? std::string(cv2name) : name + ".cv2", op.out);
                return fused_cv2;
            }
        }
        int t = buf(H, W, c_, name + ".t");
        conv(name + ".cv1", in, H, W, whole(t));
        conv(name + ".cv2", whole(t), H, W, out, in);  // shortcut add (c1 == c2)
        return false;
    }

    void c3k(const std::string &name, Slice in, int H, int W, Slice out, int n) {
        int c_ = out.C / 2;
        const bool img_on = M.o.hmerge && M.o.c3kimg && !M.f32;
        if (img_on && in.buf >= 0 && out.buf >= 0 && !P.bufs[in.buf].blk && !P.bufs[in.buf].virt && !P.bufs[out.buf].blk &&
            c3kimg_supported(H, W, in.C, c_, out.C, n)) {
            // the whole block in one launch: weight stream = the six layers' MFMA fragments back to back
            const std::string names[6] = {name + ".cv1", name + ".cv2", name + ".m.0.cv1", name + ".m.0.cv2", name + ".m.1.cv1", name + ".m.1.cv2"};
            const ConvRecord *r[7];
            bool ok = true;
            for (int i = 0; i < 6; ++i) { r[i] = rec(names[i]); ok = ok && r[i]; }
            r[6] = rec(name + ".cv3"); ok = ok && r[6];
            if (!ok || err) return;
            if (rec_is(r[0], 1, in.C, c_) && rec_is(r[1], 1, in.C, c_) && rec_is(r[2], 3, c_, c_) && rec_is(r[3], 3, c_, c_) && rec_is(r[4], 3, c_, c_) &&
                rec_is(r[5], 3, c_, c_) && rec_is(r[6], 1, 2 * c_, out.C)) {
                std::vector<bf16_t> stream;
                std::vector<float> bias(6 * 128, 0.f);  // (k_c3kimg: one 128-float row per layer, [cv1 | cv2] sharing the first)
                auto add = [&](const float *w, int cout, int cin, int ks) {
                    ConvTiling t{1, 1, 1, 4, cin};
                    std::vector<bf16_t> pk = pack_conv_weights(w, cout, cin, ks, t, nullptr, 0, M.f16);
                    stream.insert(stream.end(), pk.begin(), pk.end());
                };
                std::vector<float> w01((size_t)2 * c_ * in.C);
                std::copy(r[0]->w, r[0]->w + (size_t)c_ * in.C, w01.begin());
                std::copy(r[1]->w, r[1]->w + (size_t)c_ * in.C, w01.begin() + (size_t)c_ * in.C);
                add(w01.data(), 2 * c_, in.C, 1);
                for (int c = 0; c < c_; ++c) { bias[c] = r[0]->b[c]; bias[c_ + c] = r[1]->b[c]; }
                for (int i = 2; i < 6; ++i) {
                    add(r[i]->w, c_, c_, 3);
                    for (int c = 0; c < c_; ++c) bias[(i - 1) * 128 + c] = r[i]->b[c];
                }
                add(r[6]->w, out.C, 2 * c_, 1);
                for (int c = 0; c < out.C; ++c) bias[5 * 128 + c] = r[6]->b[c];
                if ((int)(stream.size() / 8) != c3kimg_pieces()) { err = set_error(ctx, OBB_ERR_STATE, "c3k image kernel: weight stream has %zu pieces", stream.size() / 8); return; }
                Op op;
                op.type = OP_C3KIMG; op.name = name; op.in = in; op.out = out; op.H = H; op.W = W; op.Ho = H; op.Wo = W;
                op.c3kimg.wts = upload(stream); op.c3kimg.bias = upload(bias); op.c3kimg.f16 = M.f16;
                op.macs = (double)H * W * ((double)in.C * 2 * c_ + 4.0 * 9 * c_ * c_ + 2.0 * c_ * out.C);
                emit(op, name + ".cv3", out);
                return;
            }
        }
        // the n Bottlenecks in a row from `cur`, the last one writing the first member of the concat buffer `cat`
        auto chain = [&](Slice cur, int cat) {
            for (int i = 0; i < n; ++i) {
                Slice dst = (i == n - 1) ? sub(cat, 0, c_) : whole(buf(H, W, c_, name + ".m" + std::to_string(i)));
                bottleneck(name + ".m." + std::to_string(i), cur, H, W, dst, 1.0);
                cur = dst;
            }
        };
        const std::string mn = n >= 2 ? merged_record(name + ".cv1", name + ".cv2") : std::string();
        if (!mn.empty()) {
            // cv1 and cv2 read the same tensor: one launch writes [a | b]; the last Bottleneck later overwrites the (then dead) `a` member, so
            // the same buffer is cv3's concat input.  Members are dense blocks (channel-blocked buffer).
            int ab = buf(H, W, 2 * c_, name + ".cat", false, c_);
            conv(mn, in, H, W, whole(ab));
            P.named[name + ".cv1"] = sub(ab, 0, c_);
            chain(sub(ab, 0, c_), ab);
            P.named[name + ".cv2"] = sub(ab, c_, c_);
            conv(name + ".cv3", whole(ab), H, W, out);
            return;
        }
        if (err) return;
        int cat = buf(H, W, 2 * c_, name + ".cat");
        int a = buf(H, W, c_, name + ".a");
        conv(name + ".cv1", in, H, W, whole(a));
        chain(whole(a), cat);
        conv(name + ".cv2", in, H, W, sub(cat, c_, c_));
        conv(name + ".cv3", whole(cat), H, W, out);
    }

    // `prod` (optional): the conv whose only consumer is this block, not yet emitted, reading `pin` (pH x pW): if the pair has a
    // kernel (tail_ok, act16) this block's cv1 runs inside the producer's launch and the producer's output tensor never exists
    void c3k2(int li, Slice in, int H, int W, Slice out, int n, bool use_c3k, double e, const char *prod = nullptr, Slice pin = Slice(), int pH = 0,
              int pW = 0) {
        std::string name = "model." + std::to_string(li);
        int c = (int)(out.C * e);
        // [y0 | y1 | y2 ...]: the bottleneck reads / writes single members of this concat -> one dense block per member
        int cat = buf(H, W, (2 + n) * c, name + ".cat", false, use_c3k ? 0 : c);
        if (prod) conv(prod, pin, pH, pW, sub(cat, 0, 2 * c), Slice(), -1, nullptr, (name + ".cv1").c_str());
        else conv(name + ".cv1", in, H, W, sub(cat, 0, 2 * c));
        if (n == 1 && !use_c3k) {  // one Bottleneck: the forms that take the closing 1x1 into its launch
            if (c3k2_f32(name, cat, c, H, W, out)) return;
            if (bottleneck(name + ".m.0", sub(cat, c, c), H, W, sub(cat, 2 * c, c), 0.5, (name + ".cv2").c_str(), sub(cat, 0, c), out)) return;
        } else {
            for (int i = 0; i < n; ++i) {
                Slice src = sub(cat, (1 + i) * c, c), dst = sub(cat, (2 + i) * c, c);
                if (use_c3k) c3k(name + ".m." + std::to_string(i), src, H, W, dst, 2);
                else bottleneck(name + ".m." + std::to_string(i), src, H, W, dst, 0.5);
            }
        }
        conv(name + ".cv2", whole(cat), H, W, out);
    }
    // fp32 mode: Bottleneck (3x3, 3x3, shortcut) + closing 1x1 of a C3k2 block with one Bottleneck as ONE launch (c3k2f32.hip); false: not emitted
    bool c3k2_f32(const std::string &name, int cat, int c, int H, int W, Slice out) {
        if (!M.f32 || !M.o.tail || !M.o.c3k2f || out.buf < 0 || P.bufs[out.buf].virt || P.bufs[cat].blk32 || !c3k2f32_supported(c, out.C, H, W)) return false;
        const ConvRecord *r1 = rec(name + ".m.0.cv1"), *r2 = rec(name + ".m.0.cv2"), *rc = rec(name + ".cv2");
        if (!r1 || !r2 || !rc || err) return false;
        if (!rec_is(r1, 3, c, c / 2) || !rec_is(r2, 3, c / 2, c) || !rec_is(rc, 1, 3 * c, out.C)) return false;
        const std::vector<int> perm = c3k2f32_cout_perm(out.C);
        const Conv32Tiling t1{1, 1, c, 1, 1, 1, 1}, t2{1, 1, c / 2, 1, 1, 1, 1}, tc{1, 1, 3 * c, out.C / 16, 1, 1, 1};
        std::vector<float> wall = pack_conv32_weights(r1->w, c / 2, c, 3, t1, nullptr, false);  // [W1 | W2 | WC | bc]: the kernel's LDS image
        const std::vector<float> w2 = pack_conv32_weights(r2->w, c, c / 2, 3, t2, nullptr, false), wc = pack_conv32_weights(rc->w, out.C, 3 * c, 1, tc, perm.data(), false);
        wall.insert(wall.end(), w2.begin(), w2.end());
        wall.insert(wall.end(), wc.begin(), wc.end());
        for (int i = 0; i < out.C; ++i) wall.push_back(rc->b[perm[i]]);
        if (wall.size() != (size_t)(9 * 256 + 4 * 256 + 2 * 64 + (out.C / 16) * 3 * 256 + out.C)) { err = set_error(ctx, OBB_ERR_STATE, "c3k2 fp32 kernel: weight image has %zu floats", wall.size()); return false; }
        Op op;
        op.type = OP_C3K2F32; op.name = name + ".m.0+" + name + ".cv2"; op.in = sub(cat, 0, 2 * c); op.out = out; op.H = H; op.W = W; op.Ho = H; op.Wo = W;
        C3k2F32Launch &L = op.c3k2f;
        L.H = H; L.W = W; L.C = c; L.CO = out.C;
        L.w1 = upload(wall); L.b1 = bias_padded(r1, nullptr, 64); L.b2 = bias_padded(r2, nullptr, 64);  // (k_c3k2_f32: 64 floats each)
        op.macs = (double)H * W * (9.0 * c * (c / 2) * 2 + 3.0 * c * out.C);
        emit(op, name + ".cv2", out);
        return true;
    }

    // last two layers of a head branch at pyramid level `level`: `conv1` reading `in`, then the plain 1x1 `conv2` into the rows `head_slice`
    // of the head tensor -- fused behind conv1 where the pair has a kernel, else through the intermediate buffer `tmp`
    void head_tail(const std::string &conv1, const std::string &conv2, Slice in, int level, int H, int W, int tmp, Slice head_slice) {
        if (tail_ok(conv1, conv2, H, W)) return conv(conv1, in, H, W, head_slice, Slice(), level, nullptr, conv2.c_str());
        conv(conv1, in, H, W, whole(tmp));
        conv(conv2, whole(tmp), H, W, head_slice, Slice(), level);
    }

    int build() {
        const int h = P.h, w = P.w;
        const bool big = M.scale == "m" || M.scale == "l" || M.scale == "x";
        const int n2 = reps(2);
        const int c64 = ch(64), c128 = ch(128), c256 = ch(256), c512 = ch(512), c1024 = ch(1024);
        const int H2 = h / 2, W2 = w / 2, H4 = h / 4, W4 = w / 4, H8 = h / 8, W8 = w / 8, H16 = h / 16, W16 = w / 16, H32 = h / 32, W32 = w / 32;
        // concat buffers that later layers read: producers write straight into their slices
        // [up(x10), x6] and [up(x13), x4] feed 1x1 convs only: with `fold` neither Upsample nor Concat is materialised, the 1x1 reads both
        // sources in place (4x fewer bytes for the upsampled half, no copy kernels)
        const bool fold = M.o.upfold && c1024 % 64 == 0 && c512 % 64 == 0 && c1024 + c512 >= 128 && !big;
        int cat13 = -1, cat16 = -1;
        if (!fold) {
            cat13 = buf(H16, W16, c1024 + c512, "cat13");  // [up(x10), x6]
            cat16 = buf(H8, W8, c512 + c512, "cat16");     // [up(x13), x4]
        }
        int cat19 = buf(H16, W16, c256 + c512, "cat19");   // [x17, x13]
        int cat22 = buf(H32, W32, c512 + c1024, "cat22");  // [x20, x10]
        // fp32 mode: tensors whose consumers are 3x3 convs in 8- / 16-channel stages (stride-2 backbone convs, first head convs), depthwise
        // prologues or the skip half of a virtual concat live in 8-channel blocks per image (Buf::blk32): a stage then reads dense runs
        Slice x4 = fold ? whole(buf(H8, W8, c512, "x4", false, 0, true)) : sub(cat16, c512, c512), x6 = fold ? whole(buf(H16, W16, c512, "x6", false, 0, true)) : sub(cat13, c1024, c512);
        Slice x10 = sub(cat22, c512, c1024), x13 = sub(cat19, c256, c512);

        const bool t1 = tail_ok("model.1", "model.2.cv1", H2, W2, true), t3 = tail_ok("model.3", "model.4.cv1", H4, W4, true);
        use_front = t1 && front_ok(h, w);  // model.0 + model.1 + model.2.cv1 as one launch: x0 never exists
        int b0 = use_front ? -1 : buf(H2, W2, c64, "x0");
        if (!use_front) conv("model.0", Slice{-1, 0, M.ch}, h, w, whole(b0));
        int b1 = t1 ? -1 : buf(H4, W4, c128, "x1");
        if (!t1) conv("model.1", whole(b0), H2, W2, whole(b1));
        int b2 = buf(H4, W4, c256, "x2", false, 16, true);  // consumed by a 3x3 stride-2 conv in 16-channel (fp32: 8-channel) stages
        if (t1) c3k2(2, Slice(), H4, W4, whole(b2), n2, big, 0.25, "model.1", use_front ? Slice{-1, 0, c64} : whole(b0), H2, W2);
        else c3k2(2, whole(b1), H4, W4, whole(b2), n2, big, 0.25);
        int b3 = t3 ? -1 : buf(H8, W8, c256, "x3");
        if (!t3) conv("model.3", whole(b2), H4, W4, whole(b3));
        if (t3) c3k2(4, Slice(), H8, W8, x4, n2, big, 0.25, "model.3", whole(b2), H4, W4);
        else c3k2(4, whole(b3), H8, W8, x4, n2, big, 0.25);
        int b5 = buf(H16, W16, c512, "x5");
        conv("model.5", x4, H8, W8, whole(b5));
        c3k2(6, whole(b5), H16, W16, x6, n2, true, 0.5);
        int b7 = buf(H32, W32, c1024, "x7");
        conv("model.7", x6, H16, W16, whole(b7));
        int b8 = buf(H32, W32, c1024, "x8");
        c3k2(8, whole(b7), H32, W32, whole(b8), n2, true, 0.5);
        // SPPF
        int c_ = c1024 / 2;
        int cat9 = buf(H32, W32, 4 * c_, "cat9");
        conv("model.9.cv1", whole(b8), H32, W32, sub(cat9, 0, c_));
        if (M.o.sppf_fuse && c_ % 32 == 0 && (size_t)H32 * W32 * (M.f32 ? 256 : 128) <= 64 * 1024) {  // the three pools in one launch, planes resident in LDS
            Op op; op.type = OP_SPPF; op.name = "sppf.pools"; op.in = sub(cat9, 0, c_); op.out = whole(cat9); op.H = H32; op.W = W32; op.Ho = H32; op.Wo = W32;
            emit(op);
        } else {
            for (int i = 0; i < 3; ++i) pool(sub(cat9, i * c_, c_), H32, W32, sub(cat9, (i + 1) * c_, c_));
        }
        int b9 = buf(H32, W32, c1024, "x9");
        conv("model.9.cv2", whole(cat9), H32, W32, whole(b9));
        // C2PSA
        int cp = c1024 / 2, nh = cp / 64, hd = cp / nh, kd = hd / 2;
        int t10 = buf(H32, W32, 2 * cp, "psa.ab");
        conv("model.10.cv1", whole(b9), H32, W32, whole(t10));
        Slice bsl = sub(t10, cp, cp);
        int qkvb = buf(H32, W32, cp + 2 * nh * kd, "psa.qkv"), ao = buf(H32, W32, cp, "psa.attn"), po = buf(H32, W32, cp, "psa.pe"),
            ff = buf(H32, W32, 2 * cp, "psa.ffn");
        // qkv output channels re-ordered [q_h0..q_h(nh-1) | k_h0.. | v_h0..] so that v is one contiguous slice
        std::vector<int> perm(cp + 2 * nh * kd);
        for (int hh = 0; hh < nh; ++hh) {
            int src0 = hh * (2 * kd + hd);
            for (int d = 0; d < kd; ++d) { perm[hh * kd + d] = src0 + d; perm[nh * kd + hh * kd + d] = src0 + kd + d; }
            for (int d = 0; d < hd; ++d) perm[2 * nh * kd + hh * hd + d] = src0 + 2 * kd + d;
        }
        for (int i = 0; i < n2; ++i) {
            std::string nm = "model.10.m." + std::to_string(i);
            conv(nm + ".attn.qkv", bsl, H32, W32, whole(qkvb), Slice(), -1, perm.data());
            Op at; at.type = OP_ATTN; at.name = nm + ".attn"; at.in = whole(qkvb); at.out = whole(ao); at.H = H32; at.W = W32; at.Ho = H32; at.Wo = W32;
            at.N = H32 * W32; at.nh = nh; at.kd = kd; at.hd = hd;
            at.macs = (double)nh * ((double)at.N * at.N * kd + (double)at.N * at.N * hd);
            emit(at, nm + ".attn", whole(ao));
            dwconv(nm + ".attn.pe", sub(qkvb, 2 * nh * kd, cp), H32, W32, whole(po), whole(ao));
            conv(nm + ".attn.proj", whole(po), H32, W32, bsl, bsl);  // x = x + attn(x), in place on the b half
            conv(nm + ".ffn.0", bsl, H32, W32, whole(ff));
            conv(nm + ".ffn.1", whole(ff), H32, W32, bsl, bsl);      // x = x + ffn(x)
        }
        conv("model.10.cv2", whole(t10), H32, W32, x10);
        if (fold) cat13 = vbuf(H16, W16, x10, x6, "cat13");
        else upsample(x10, H32, W32, sub(cat13, 0, c1024));
        c3k2(13, whole(cat13), H16, W16, x13, n2, big, 0.5);
        if (fold) cat16 = vbuf(H8, W8, x13, x4, "cat16");
        else upsample(x13, H16, W16, sub(cat16, 0, c512));
        // (the pyramid levels are also read by the class branch's depthwise conv: blocked only where that runs as a prologue (dwpw32))
        auto feat_blk = [&](int C, int H, int W) { return M.f32 && M.o.tail && M.o.dwpw && plan_dwpw32(C, std::max(c256, std::min(M.nc, 100)), H, W).TH > 0; };
        int b16 = buf(H8, W8, c256, "x16", false, 0, feat_blk(c256, H8, W8));
        c3k2(16, whole(cat16), H8, W8, whole(b16), n2, big, 0.5);
        conv("model.17", whole(b16), H8, W8, sub(cat19, 0, c256));
        int b19 = buf(H16, W16, c512, "x19", false, 0, feat_blk(c512, H16, W16));
        c3k2(19, whole(cat19), H16, W16, whole(b19), n2, big, 0.5);
        conv("model.20", whole(b19), H16, W16, sub(cat22, 0, c512));
        int b22 = buf(H32, W32, c1024, "x22");
        c3k2(22, whole(cat22), H32, W32, whole(b22), n2, true, 0.5);
        // OBB head
        const int chs[3] = {c256, c512, c1024};
        const int feats[3] = {b16, b19, b22};
        const int Hs[3] = {H8, H16, H32}, Ws[3] = {W8, W16, W32};
        int c2 = std::max(std::max(16, chs[0] / 4), kRegMax * 4), c3 = std::max(chs[0], std::min(M.nc, 100)), c4 = std::max(chs[0] / 4, 1);
        P.no = 4 * kRegMax + M.nc + 1;
        P.no_pad = (P.no + 3) / 4 * 4;  // head rows padded to 16 B so that every lane stores whole float4s
        int off = 0;
        for (int i = 0; i < 3; ++i) { P.lvl_off[i] = off; off += Hs[i] * Ws[i]; }
        P.A = off;
        Slice u1s[3];  // first conv of the angle branch, when it ran merged with the box branch's first conv
        for (int i = 0; i < 3; ++i) {
            std::string p = "model.23.cv2." + std::to_string(i), p4 = "model.23.cv4." + std::to_string(i);
            // (only where a layer is one tile per image and therefore latency-bound: at the larger levels the padded second cout block costs
            //  more MFMA time than the saved launch and input read are worth -- measured)
            //  -- except where k_conv3_pair takes the merged 64 + 16 couts as ONE group of five fragments (64 input channels, 13 x 13 tiles):
            //  no padded block there, and the feature map is read once instead of twice)
            const bool pair80 = M.o.pair && !M.f32 && P.bufs[feats[i]].C == 64 && c2 == 64 && c4 == 16 && Hs[i] % 13 == 0 && Ws[i] % 13 == 0;
            // (fp32 mode: never -- the exact-f32 MFMA is the bound there and the merged 80 couts would pad to two 64-cout blocks)
            const std::string mn = (!M.f32 && c2 % 16 == 0 && c4 % 16 == 0 && (Hs[i] * Ws[i] <= 256 || pair80)) ? merged_record(p + ".0", p4 + ".0") : std::string();
            if (err) return err;
            int t2 = buf(Hs[i], Ws[i], c2, p + ".t2");
            Slice t1;
            if (!mn.empty()) {  // box and angle branch start with a 3x3 conv on the same feature map: one launch, [t1 | u1] in 16-channel blocks
                int hb = buf(Hs[i], Ws[i], c2 + c4, p + ".t1u1", false, pair80 ? 0 : 16);  // (the pair kernel reads whole 128-B pixel rows: plain NHWC there)
                conv(mn, whole(feats[i]), Hs[i], Ws[i], whole(hb));
                P.named[p + ".0"] = t1 = sub(hb, 0, c2);
                P.named[p4 + ".0"] = u1s[i] = sub(hb, c2, c4);
            } else {
                t1 = whole(buf(Hs[i], Ws[i], c2, p + ".t1", false, 0, true));
                conv(p + ".0", whole(feats[i]), Hs[i], Ws[i], t1);
            }
            head_tail(p + ".1", p + ".2", t1, i, Hs[i], Ws[i], t2, Slice{-2, 0, 4 * kRegMax});
        }
        for (int i = 0; i < 3; ++i) {
            std::string p = "model.23.cv3." + std::to_string(i);
            const Slice logits{-2, 4 * kRegMax, M.nc};
            int e1 = buf(Hs[i], Ws[i], c3, p + ".e1");
            if (!dwpw(p + ".0.0", p + ".0.1", whole(feats[i]), Hs[i], Ws[i], whole(e1))) {
                int d1 = buf(Hs[i], Ws[i], chs[i], p + ".d1");
                dwconv(p + ".0.0", whole(feats[i]), Hs[i], Ws[i], whole(d1));
                conv(p + ".0.1", whole(d1), Hs[i], Ws[i], whole(e1));
            }
            if (err) return err;
            if (dwpw(p + ".1.0", p + ".1.1", whole(e1), Hs[i], Ws[i], logits, (p + ".2").c_str(), i)) continue;
            if (err) return err;
            int d2 = buf(Hs[i], Ws[i], c3, p + ".d2"), e2 = buf(Hs[i], Ws[i], c3, p + ".e2");
            dwconv(p + ".1.0", whole(e1), Hs[i], Ws[i], whole(d2));
            head_tail(p + ".1.1", p + ".2", whole(d2), i, Hs[i], Ws[i], e2, logits);
        }
        for (int i = 0; i < 3; ++i) {
            std::string p = "model.23.cv4." + std::to_string(i);
            int u2 = buf(Hs[i], Ws[i], c4, p + ".u2");
            Slice u1 = u1s[i];
            if (u1.buf < 0) {
                u1 = whole(buf(Hs[i], Ws[i], c4, p + ".u1"));
                conv(p + ".0", whole(feats[i]), Hs[i], Ws[i], u1);
            }
            head_tail(p + ".1", p + ".2", u1, i, Hs[i], Ws[i], u2, Slice{-2, 4 * kRegMax + M.nc, 1});
        }
        for (const char *nm : {"x0", "x1", "x2", "x3", "x5", "x7", "x8", "x9", "x16", "x19", "x22"})
            for (size_t b = 0; b < P.bufs.size(); ++b)
                if (P.bufs[b].name == nm) P.named[nm] = whole((int)b);
        P.named["x4"] = x4; P.named["x6"] = x6; P.named["x10"] = x10; P.named["x13"] = x13;
        return err;
    }
};

int build_plan(obb_ctx *ctx, Model &M, Plan &P) { return Builder{ctx, M, P}.build(); }

}  // namespace obb

// Host only: the packed fp32 weights of columns [c0, c0 + nc) of the 1x1 matrix w[cout][cin], as the plan builder packs them for
// form 0: k_pw_f32 (the coarse partial product of "upacc"), 1: the plain two-fragment k_conv_f32 form (its fine remainder), 2: the VCAT form
// over the whole virtual concat.  tiling_host (optional) receives {CK, WC, NC} of forms 1 / 2.
extern "C" int obb_debug_pack_1x1(int32_t form, const float *w, int32_t cout, int32_t cin, int32_t c0, int32_t nc, float *out, int64_t max_floats, int64_t *needed,
                                  int32_t *tiling_host) {
    using namespace obb;
    if (!w || !needed || form < 0 || form > 2 || cout < 1 || cin < 1 || c0 < 0 || nc < 1 || c0 + nc > cin) return OBB_ERR_INVALID;
    const std::vector<float> m = split_cols(w, cout, cin, c0, nc);
    std::vector<float> pk;
    if (form == 0) {
        if (!pw32_supported(nc, cout)) return OBB_ERR_INVALID;
        pk = pack_pw32_weights(m.data(), cout, nc, nullptr);
    } else {
        const Conv32Tiling t = plan_conv32(1, 1, nc, cout, 2, 2, false, form == 2, true);
        if (tiling_host) { tiling_host[0] = t.CK; tiling_host[1] = t.WC; tiling_host[2] = std::max(1, t.NC); }
        pk = pack_conv32_weights(m.data(), cout, nc, 1, t, nullptr, false);
    }
    *needed = (int64_t)pk.size();
    if (out && max_floats >= *needed) memcpy(out, pk.data(), pk.size() * sizeof(float));
    return OBB_OK;
}
