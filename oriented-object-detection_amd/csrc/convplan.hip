// Host half of the 16-bit conv family (k_conv_igemm, k_conv3_pair in conv.hip): tile planner, weight packer, and the argument checks +
// kernel parameters + kernel variant of a launch.  No kernel, no launch and no HIP runtime call: the file also builds as plain C++ with
// the host compiler (tests/host/convplan_main.cpp links it without a GPU runtime).
#include "conv.h"
#include "convgeom.h"
#include "convparams.h"
#include "convvariants.h"

#include <algorithm>
#include <cstdlib>

namespace obb {

static int ilog2(int v) { int s = 0; while ((1 << s) < v) ++s; return s; }

int conv_ksteps(int ks, int CK) { return c16::ksteps(ks, CK); }

ConvTiling plan_conv(int ks, int stride, int cin, int cout, int Hout, int Wout, bool pair) {
    ConvTiling t;
    t.NF = cout <= 16 ? 1 : (cout <= 32 ? 2 : 4);
    if (ks == 1) {
        // 1x1: the whole batch is one long pixel row (caller passes Hout = 1, Wout = B*H*W)
        static const int ck1 = getenv("OBB_CK1") ? atoi(getenv("OBB_CK1")) : 64;
        t.TH = 1; t.MF = 2; t.TW = 64 * t.MF;
        t.CK = cin >= 128 ? std::min(ck1, 64) : (cin >= 64 ? 64 : 32);
        return t;
    }
    int cin8 = (cin + 7) / 8 * 8;
    if (Hout % 13 == 0 && Wout % 13 == 0) { t.TH = 13; t.TW = 13; t.MF = 3; }
    else if (Hout >= 16 && Wout >= 16) { t.TH = 8; t.TW = 16; t.MF = 2; }
    else { t.TH = 8; t.TW = 8; t.MF = 1; }
    static const int ck3 = getenv("OBB_CK3") ? std::min(atoi(getenv("OBB_CK3")), 16) : 16;  // weights stage = 5 * NF KiB
    int ck = 1;
    while (ck * 2 <= cin8 && ck * 2 <= ck3) ck *= 2;  // power of two <= min(cin8, ck3)
    if (ck < 8) ck = 8;
    if (stride == 2 && ck > 16) ck = 16;             // keep the (2T+1)^2 halo tile small enough for several groups per CU
    t.CK = ck;
    // weights-resident single-stage form (WRES): 3x3 stride 1 on 13 x 13 tiles with 32 or 64 input channels
    // (measured per 256 tiles: 64 -> 16 couts at 52^2 60.9 -> 50.4 us, 64 -> 32 at 26^2 24.6 -> 23.6 us; the 64-cout groups (104 KiB of LDS, one
    //  group per CU) gained nothing -- 112.6 -> 115.7 us -- so they keep the 16-channel stages: their k loop is bound by LDS operand
    //  reads, 7 KiB per 12 MFMAs and wave, not by the per-stage global-memory latency)
    if (stride == 1 && t.MF == 3 && (cin == 32 || cin == 64) && (t.NF == 2 || t.NF == 1)) t.CK = cin;
    // 64 -> 64-cout groups: the same single-stage packing, run by k_conv3_pair (two half-groups per CU sharing the resident weights)
    if (pair && stride == 1 && t.MF == 3 && cin == 64 && t.NF == 4) t.CK = 64;
    // stride 2, 64 input channels: 4-row stripes of 13 outputs per half-group (one fragment per wave), same packing
    if (pair && stride == 2 && cin == 64 && t.NF == 4 && Wout % 13 == 0 && Hout >= 4) { t.TH = 4; t.TW = 13; t.MF = 1; t.CK = 64; }
    return t;
}

int64_t conv_packed_elems(int cout, int cin, int ks, const ConvTiling &t, int in_u8) {
    return c16::packed_elems(cout, cin, ks, t.NF, t.CK, in_u8 != 0);
}

std::vector<bf16_t> pack_conv_weights(const float *w, int cout, int cin, int ks, const ConvTiling &t, const int *perm, int in_u8, bool f16) {
    const int CK = t.CK, NF = t.NF, cpk = CK / 8;
    const int nstage = c16::stages(cin, CK, in_u8 != 0);
    const int kst = c16::ksteps(ks, CK);
    const int ncb = c16::cout_blocks(cout, NF);
    const int taps = ks * ks;
    std::vector<bf16_t> out((size_t)conv_packed_elems(cout, cin, ks, t, in_u8), 0);
    size_t o = 0;
    for (int cb = 0; cb < ncb; ++cb)
        for (int st = 0; st < nstage; ++st)
            for (int k = 0; k < kst; ++k)
                for (int f = 0; f < NF; ++f)
                    for (int lane = 0; lane < 64; ++lane) {
                        int r = lane & 15, gq = lane >> 4;
                        int co = cb * 16 * NF + (r >> 2) * 4 * NF + f * 4 + (r & 3);
                        int q = k * 4 + gq;
                        int tap = (ks == 3) ? q / cpk : 0;
                        int c0 = (ks == 3) ? (q % cpk) * 8 : q * 8;
                        for (int j = 0; j < 8; ++j, ++o) {
                            int c = st * CK + c0 + j;
                            bool ok = co < cout && c < cin && tap < taps && (ks == 3 || c0 < CK);
                            if (!ok) continue;
                            int src = perm ? perm[co] : co;
                            out[o] = host_to_half(w[((size_t)src * cin + c) * taps + tap], f16);
                        }
                    }
    return out;
}

static bool conv_multi_stage(const ConvLaunch &L) { return (L.in_u8 ? 8 : L.cin) > L.CK; }
static bool conv_wres(const ConvLaunch &L) { return L.ks == 3 && L.CK > 16; }
static int tail_nf(int cout2);
// k_conv3_pair's shapes (plan_conv gives them CK = 64): everything else with CK = 64 stays on the one-group WRES form of k_conv_igemm
static bool conv_pair(const ConvLaunch &L) {
    if (L.ks != 3 || L.NF != 4 || L.CK != 64 || L.cin != 64 || L.TW != 13 || L.in_u8 || L.out_f32 || L.res.p || L.up_c != 0) return false;
    if (L.cout == 80) return L.stride == 1 && L.MF == 3 && L.TH == 13 && L.tail_cout == 0;  // two merged siblings, 64 + 16 couts: one group of five fragments
    if (L.cout % 64) return false;
    if (L.stride == 1)
        return L.MF == 3 && L.TH == 13 && (L.tail_cout == 0 || (!L.tail_act16 && tail_nf(L.tail_cout) == 4 && L.cout == 64 && L.tail_cout % 4 == 0 && L.tail_out_hw == 0 &&
                                                                ((L.tail_out.cs | L.tail_out.co) & 3) == 0));
    return L.stride == 2 && L.MF == 1 && L.TH == 4 && (L.tail_cout == 0 || (L.tail_act16 && L.tail_cout == 64 && L.cout == 64));
}

// LDS layout (convgeom.h): [input tile (one channel stage) | weights of the stage | weights of a fused tail]
static size_t conv_act_bytes(const ConvLaunch &L) {
    return (size_t)c16::act_bytes(L.NI, L.TH, L.TW, L.stride, L.ks, L.CK, L.in_u8 != 0, conv_multi_stage(L), L.MF, L.NF, L.out_f32 != 0);
}

static size_t conv_main_lds(const ConvLaunch &L) { return (size_t)c16::main_lds((int64_t)conv_act_bytes(L), L.ks, L.CK, L.MF, L.NF, L.out_f32 != 0); }

static int tail_nf(int cout2) { return cout2 <= 16 ? 1 : (cout2 <= 32 ? 2 : 4); }

size_t conv_lds_bytes(const ConvLaunch &L) {
    return conv_main_lds(L) + (L.tail_cout > 0 ? (size_t)c16::tail_weight_bytes(L.NF, tail_nf(L.tail_cout)) : 0);  // tail weights behind everything else
}

int conv_ni_supported(const ConvLaunch &L) {
    // the register-direct store path of k_conv_igemm (64-cout groups, no tail, 16-bit plain-NHWC output) on the one-fragment-per-wave tile
    if (L.ks != 3 || L.NF != 4 || L.MF != 1 || L.in_u8 || L.out_f32 || L.tail_cout > 0 || L.up_c > 0 || L.CK > 16) return 1;  // (channel-blocked slices included: an image is one stride inside every block plane)
    if (L.Hout != L.Wout || (L.Hout != 4 && L.Hout != 2)) return 1;
    return 64 / (L.Hout * L.Wout);
}

bool conv_tail_supported(int ks, int MF, int NF, int cout1, int cout2, bool act16, int TH) {
    if (cout1 != 16 * NF || cout2 < 1 || cout2 > 64) return false;
    const int nf2 = tail_nf(cout2);
    if (act16 && ks == 3 && MF == 1 && NF == 4 && TH == 4) return cout2 == 64;  // k_conv3_pair, stride-2 stripes
    if (act16) return ks == 3 && MF == 3 && (NF == 2 || NF == 4) && nf2 == NF && cout2 == 16 * nf2;  // whole 16-bit rows of the staging area
    return (ks == 3 && MF == 3 && NF == 4 && nf2 == 4) || (ks == 3 && MF == 3 && NF == 1 && nf2 == 1) || (ks == 1 && MF == 2 && NF == 4 && nf2 == 1);
}

// the check that refused this thread's last conv_params call (convparams.h)
static thread_local const char *g_refusal = "";
static hipError_t refuse(const char *check) { g_refusal = check; return hipErrorInvalidValue; }
const char *conv_params_refusal() { return g_refusal; }

hipError_t conv_params(const ConvLaunch &L, ConvParams &P, ConvVariant &V, unsigned &grid_x, unsigned &threads, size_t &lds) {
    V = ConvVariant();
    g_refusal = "";
    P.in = L.in.p; P.in_bs = L.in.bs; P.in_cs = L.in.cs; P.in_co = L.in.co;
    P.out = L.out.p; P.out_bs = L.out.bs; P.out_cs = L.out.cs; P.out_co = L.out.co;
    P.res = (const bf16_t *)L.res.p; P.res_bs = L.res.bs; P.res_cs = L.res.cs; P.res_co = L.res.co;
    P.in_bsh = P.out_bsh = P.res_bsh = 31;
    P.in_bmask = P.out_bmask = P.res_bmask = 0x7fffffff;
    P.in_ps2 = 0; P.out_ps = 0; P.res_ps = 0;
    int64_t in_block_span = 0;  // blocked input: elements from the slice's first block to the end of its last block (one image)
    {
        auto blocked = [](const TensorRef &T, int C, int &bsh, int &bmask, int64_t &ps, int &co, int &cs, int64_t *span) -> bool {
            if (T.cpb <= 0) return true;
            const int blk = 8 * T.cpb;
            if ((T.cpb & (T.cpb - 1)) || T.co % blk || T.cs != blk) return false;
            bsh = 0;
            while ((1 << bsh) < T.cpb) ++bsh;
            bmask = T.cpb - 1;
            ps = T.ps;
            if (span) *span = (int64_t)((C + blk - 1) / blk - 1) * T.ps;
            co = 0;  // the slice offset is a whole number of blocks: folded into the base pointer by the caller below
            return true;
        };
        int64_t ps_in = 0;
        int co_in = P.in_co, cs_in = P.in_cs;
        if (!L.in_u8) {
            if (!blocked(L.in, L.cin, P.in_bsh, P.in_bmask, ps_in, co_in, cs_in, &in_block_span)) return refuse("in_blocked");
            if (L.in.cpb > 0) {
                if (ps_in * 2 >= (1ll << 32)) return refuse("in_block_stride");
                P.in = (const bf16_t *)L.in.p + (int64_t)(L.in.co / (8 * L.in.cpb)) * L.in.ps;
                P.in_co = 0;
                P.in_ps2 = (unsigned)(ps_in * 2);
            }
        } else if (L.in.cpb > 0) return refuse("u8_blocked");
        int co_out = P.out_co, cs_out = P.out_cs;
        if (!blocked(L.out, L.cout, P.out_bsh, P.out_bmask, P.out_ps, co_out, cs_out, nullptr) || (L.out.cpb > 0 && L.out_f32)) return refuse("out_blocked");
        if (L.out.cpb > 0) { P.out = (bf16_t *)L.out.p + (int64_t)(L.out.co / (8 * L.out.cpb)) * L.out.ps; P.out_co = 0; }
        int co_res = P.res_co, cs_res = P.res_cs;
        if (L.res.p) {
            if (!blocked(L.res, L.cout, P.res_bsh, P.res_bmask, P.res_ps, co_res, cs_res, nullptr)) return refuse("res_blocked");
            if (L.res.cpb > 0) { P.res = (const bf16_t *)L.res.p + (int64_t)(L.res.co / (8 * L.res.cpb)) * L.res.ps; P.res_co = 0; }
        }
    }
    if (!L.lut) return refuse("lut");  // also the sink of the unconditional stores (lut + 512 B .. + 1.5 KiB): never NULL
    P.wpk = L.wpk; P.bias = L.bias; P.lut = L.lut;
    P.Hin = L.Hin; P.Win = L.Win; P.Hout = L.Hout; P.Wout = L.Wout;
    P.cin = L.cin; P.cout = L.cout; P.stride = L.stride; P.act = L.act; P.flip_bgr = L.flip_bgr;
    P.TH = L.TH; P.TW = L.TW; P.CK = L.CK; P.sh = ilog2(L.CK / 8);
    P.tiles_x = L.tiles_x; P.tiles_y = L.tiles_y; P.out_hw = L.out_hw; P.act_bytes = (int)conv_act_bytes(L);
    const int NI = std::max(1, L.NI);
    P.NI = NI; P.B = L.B;
    if (NI > 1 && (NI != conv_ni_supported(L) || L.TH != L.Hout || L.TW != L.Wout || L.tiles_x != 1 || L.tiles_y != 1 || L.out_hw)) return refuse("ni");
#if defined(OBB_STAMPS) || defined(OBB_DIAG)  // timing-only ablations exist in the diagnostic build alone (tools/stamp_conv.sh): the product library ignores the variable
    static const int dbg = getenv("OBB_CONV_DBG") ? atoi(getenv("OBB_CONV_DBG")) : 0;
    P.dbg = dbg;
#else
    P.dbg = 0;
#endif
    P.stamps = nullptr;  // (diagnostic build: launch_conv owns the buffer)
    P.in2 = L.in2.p; P.in2_cs = L.in2.cs; P.in2_co = L.in2.co; P.up_c = L.up_c; P.up_W = L.up_W; P.up_HW = L.up_HW; P.in2_span_bytes = 0;
    if (L.up_c > 0) {  // virtual [upsample | skip] concat: 1-D 1x1 launches over plain NHWC sources only
        if (L.ks != 1 || L.in_u8 || L.B != 1 || L.Hin != 1 || L.in.cpb || L.in2.cpb || !L.in2.p || L.up_c % L.CK || L.up_c >= L.cin || (L.up_W & 1) ||
            (L.up_HW % L.up_W) || ((L.up_HW / L.up_W) & 1) || L.Win % L.up_HW)
            return refuse("vcat_args");
        int64_t s2 = ((int64_t)L.Win * L.in2.cs - L.in2.co) * 2, s1 = ((int64_t)(L.Win / 4) * L.in.cs - L.in.co) * 2;
        if (s1 <= 0 || s2 <= 0 || s1 >= (1ll << 32) - 65536 || s2 >= (1ll << 32) - 65536) return refuse("vcat_span");
        P.in2_span_bytes = (unsigned)s2;
    }
    P.w2pk = L.tail_wpk; P.bias2 = L.tail_bias; P.out2 = (float *)L.tail_out.p; P.out2_bs = L.tail_out.bs; P.out2_cs = L.tail_out.cs;
    P.out2_co = L.tail_out.co; P.out2_hw = L.tail_out_hw; P.cout2 = L.tail_cout; P.kst2 = c16::tail_ksteps(L.NF);
    P.w2_off = (int)conv_main_lds(L);
    if (L.tail_cout > 0 && (!conv_tail_supported(L.ks, L.MF, L.NF, L.cout, L.tail_cout, L.tail_act16, L.TH) || !L.tail_wpk || !L.tail_bias || (!L.tail_act16 && !L.tail_out.p))) return refuse("tail");

    P.nstage = c16::stages(L.cin, L.CK, L.in_u8 != 0);
    P.kst = c16::ksteps(L.ks, L.CK);
    {
        int64_t span = ((int64_t)L.Hin * L.Win * L.in.cs - L.in.co) * 2;  // from the slice's first element to the end of the image
        if (L.in.cpb > 0) span = (in_block_span + (int64_t)L.Hin * L.Win * L.in.cs) * 2;  // ... to the end of the slice's last block
        if (L.up_c > 0) span = ((int64_t)(L.Win / 4) * L.in.cs - L.in.co) * 2;  // the low-res source of a virtual concat
        span += (int64_t)(NI - 1) * L.in.bs * 2;  // a multi-image tile reads up to the end of its last image
        const int64_t wb = c16::packed_elems(L.cout, L.cin, L.ks, L.NF, L.CK, L.in_u8 != 0) * (int64_t)sizeof(bf16_t);
        if (span <= 0 || span >= (1ll << 32) - 65536 || wb >= (1ll << 31)) return refuse("span");  // 32-bit buffer offsets
        P.in_span_bytes = (unsigned)span;
        P.w_bytes = (unsigned)wb;
        if (conv_wres(L) && !conv_pair(L) && (L.stride != 1 || L.MF != 3 || L.CK != L.cin || (L.cin != 32 && L.cin != 64) || L.in_u8 || L.out_f32 || L.up_c > 0)) return refuse("wres_shape");
    }
    const int TWin = c16::tile_in(L.TW, L.stride, L.ks);
    P.inv_twin = 1.0f / (float)TWin;
    P.inv_tw = 1.0f / (float)L.TW;
    if ((1 << P.sh) != L.CK / 8 || NI * L.TH * L.TW > 64 * L.MF || L.MF < 1 || L.MF > 3) return refuse("tile");
    if (!L.in_u8 && c16::stage_chunks(NI, L.TH, L.TW, L.stride, L.ks, L.CK) > c16::chunk_cap(conv_wres(L), L.ks)) return refuse("staging");  // staging plan: chunks per thread
    if (L.ks == 1 && L.CK > 64) return refuse("ck_1x1");
    int ncb = c16::cout_blocks(L.cout, L.NF);
    int64_t ntiles = NI > 1 ? ((int64_t)L.B + NI - 1) / NI : (int64_t)L.B * L.tiles_y * L.tiles_x;
    if (ntiles >= (1ll << 31)) return refuse("ntiles");
    P.ntiles = (int)ntiles;
    if (conv_pair(L)) {  // one 512-thread workgroup per CU, its two halves walking alternate tiles
        const int nf5 = L.cout == 80 ? 1 : 0;
        if (nf5) ncb = 1;
        const int64_t groups = std::max<int64_t>(1, 256 / ncb);
        P.tpw = (int)std::max<int64_t>(2, (ntiles + groups - 1) / groups);
        P.gx = (int)((ntiles + P.tpw - 1) / P.tpw); P.ncb = ncb;
        lds = (size_t)c16::pair_lds(P.act_bytes, P.kst, L.NF + nf5, L.tail_cout > 0);
        // (conv_pair already asks for ks 3, CK = cin = 64 and one of the two tile shapes: a guard that no ConvLaunch reaches)
        if (P.kst != c16::ksteps(3, 64) || P.nstage != 1 || lds > (size_t)c16::kLdsPair) return refuse("pair_layout");
        grid_x = (unsigned)((P.gx + 7) / 8 * 8 * ncb);
        threads = 512;
        V.pair = true; V.F16 = L.f16 != 0; V.S = L.stride;
        V.NF = nf5 ? 5 : 4;
        V.TAIL = L.tail_cout > 0 ? (L.stride == 2 ? 16 : 4) : 0;
        return conv_variant_lds_cap(V) ? hipSuccess : refuse("variant");
    }
    // tiles per workgroup: keep >= ~8 groups per CU in flight, walk up to 8 consecutive tiles per group beyond that
    static const int tpw_max = getenv("OBB_TPW") ? atoi(getenv("OBB_TPW")) : 8;
    int64_t tpw = ntiles * ncb / (256 * 8);
    P.tpw = (int)std::max<int64_t>(1, std::min<int64_t>(tpw, tpw_max));
    if (conv_wres(L)) P.tpw = (int)std::max<int64_t>(1, std::min<int64_t>(ntiles * ncb / (256 * 2), 16));  // one group per CU: two rounds of groups, <= 16 tiles each
    P.gx = (int)((ntiles + P.tpw - 1) / P.tpw); P.ncb = ncb;
    grid_x = (unsigned)((P.gx + 7) / 8 * 8 * ncb);  // 1-D: see the XCD-aware decoding at the top of the kernel
    threads = 256;
    lds = conv_lds_bytes(L);
    if (lds > (size_t)(conv_wres(L) ? c16::kLdsWres : c16::kLdsDefault)) return refuse("lds_cap");
    // the kernel variant.  Which forms exist is convvariants.h's to say; what is decided here is which form a launch asks for, and the
    // combinations that no form takes whatever its shape
    V.KS = L.ks; V.MF = L.MF; V.NF = L.NF; V.F16 = L.f16 != 0;
    if (L.ks == 3 && L.MF == 3 && conv_wres(L)) {  // weights-resident single-stage form: plain / fp32 head tail
        if (L.tail_cout > 0 && L.tail_act16) return refuse("wres_t16");  // (the fused cv1 sits behind stride-2 convs only)
        V.WRES = true;
        if (L.tail_cout > 0) V.TAIL = L.NF == 4 ? 4 : 1;
    } else if (L.tail_cout > 0 && L.tail_act16) {  // stride-2 backbone conv + the cv1 of the following C3k2 block
        V.T16 = true; V.TAIL = L.NF;
    } else if (L.tail_cout > 0) {  // the fp32 rows of the OBB head
        V.TAIL = (L.ks == 3 && L.MF == 3 && L.NF == 4) ? 4 : 1;
    } else if (L.up_c > 0) V.VCAT = true;  // virtual upsample-concat input (the 1x1 convs behind Upsample + Concat in the neck)
    else if (L.in_u8) V.IN_U8 = true;
    else if (L.out_f32) V.OUT_F32 = true;
    else if (P.NI > 1) V.NIT = true;
    // (conv_tail_supported above has let no other tail width through: a guard, as in the launch ladder this replaces)
    if (V.TAIL > 0 && tail_nf(L.tail_cout) != V.TAIL) return refuse("tail_nf");
    if ((V.TAIL > 0 || V.VCAT) && !V.WRES && (L.in_u8 || L.out_f32)) return refuse("tail_io");
    return conv_variant_lds_cap(V) ? hipSuccess : refuse("variant");
}

}  // namespace obb
