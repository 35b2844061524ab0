// Host half of the fp32 conv family (k_conv_f32 in f32path.hip): tile planner, weight packers, and the argument checks + kernel
// parameters of a launch.  No kernel, no launch and no HIP runtime call: the file also builds as plain C++ with the host compiler
// (tests/host/f32plan_main.cpp links it without a GPU runtime).
#include "c32geom.h"
#include "c32params.h"
#include "f32path.h"

#include <algorithm>
#include <cstring>

namespace obb {

static int ilog2_(int v) { int s = 0; while ((1 << s) < v) ++s; return s; }

static Conv32Tiling plan_conv32_nc(int ks, int stride, int cin, int cout, int Hout, int Wout, bool in_u8, bool vcat, int NC, int64_t *cost_out);

Conv32Tiling plan_conv32(int ks, int stride, int cin, int cout, int Hout, int Wout, bool in_u8, bool vcat, bool nc2) {
    int64_t c1 = 0, c2 = 0;
    const Conv32Tiling t1 = plan_conv32_nc(ks, stride, cin, cout, Hout, Wout, in_u8, vcat, 1, &c1);
    if (!nc2 || in_u8 || cout < 64 || cout % 32 || t1.NI > 1 || cin < 64) return t1;  // (48-channel concats: HBM-bound, measured 4 % worse)
    const Conv32Tiling t2 = plan_conv32_nc(ks, stride, cin, cout, Hout, Wout, in_u8, vcat, 2, &c2);
    // (costs in MFMA groups of the busiest wave per tile; the two-fragment form may cost a few percent more of them: it reads a third less LDS)
    // (measured: forcing the form onto the 52 x 52 layers -- 13 fragments in 16 slots -- costs cv2.0.0 903 -> 984 us, onto the 13 x 13 ones 4-8 %)
    return (ks == 1 || c2 * 100 <= c1 * 97) ? t2 : t1;
}

static Conv32Tiling plan_conv32_nc(int ks, int stride, int cin, int cout, int Hout, int Wout, bool in_u8, bool vcat, int NC, int64_t *cost_out) {
    Conv32Tiling t;
    t.NC = NC;
    t.WC = NC == 2 ? 2 : (cout >= 64 ? 4 : (cout >= 32 ? 2 : 1));
    if (in_u8) t.WC = 1;  // the uint8 form exists with one cout fragment per workgroup only (launch32_f): 32 couts (the s widths) are two cout blocks
    if (in_u8) t.CK = 4;
    else {
        // (1x1: 64-channel stages = half the barriers and LDS commits of 32: 18.40 -> 18.27 ms per 512 tiles, the 13 x 13 layers 4-6 %)
        const int cap = ks == 1 ? (vcat ? 32 : 64) : (stride == 2 ? 8 : 16);  // (1x1 with 64-channel stages: measured, no gain -- 18.05 -> 18.22 ms per 512 tiles)
        int ck = 4;
        while (ck * 2 <= cap && cin % (ck * 2) == 0) ck *= 2;
        if (ks == 1 && !vcat && ck == 16 && cin % 48 == 0) ck = 48;  // 48- / 96-channel concats: one stage of three 16-channel groups instead of three stages of one k step
        t.CK = ck;
    }
    // (NC = 2, 1x1: 3 fragments per wave = 192-pixel tiles with 64-channel stages and no spill; 4 = 256 pixels forces 32-channel stages and
    // spills 44 bytes per lane -- same-box A/B over the forward: 17.84 ms with NC = 1, 17.59 with 4, 17.36 with 3)
    const int WP = c32::kNW / t.WC, MFMX = (NC == 2 && ks == 1) ? 3 : c32::mfm_max(t.WC, NC), MFMN = c32::mfm_min(t.WC, NC);
    const int maxpix = c32::tile_pixels(t.WC, MFMX);
    const int chunk_cap = c32::chunk_cap(in_u8, false, vcat, false, ks);  // 16-B chunks one stage may hold
    if (ks == 1) {  // 1-D: the caller flattens batch x pixels
        while (t.CK > 4 && (c32::stage_chunks(maxpix, t.CK, false) > chunk_cap || c32::lds_plan(maxpix, 1, t.CK, t.WC, NC) > c32::kPlanBudget)) t.CK /= 2;
        t.TH = 1; t.TW = maxpix; t.MFM = MFMX; t.NI = 1;
        if (cost_out) *cost_out = 0;
        return t;
    }
    t.TW = std::min(Wout, maxpix);
    const auto fits = [&](int th, int tw) {  // the staged input tile of th x tw outputs within the LDS and the staging plan
        const int64_t in_px = c32::tile_in_px(th, tw, stride, ks);
        return !(c32::lds_plan(in_px, ks, t.CK, t.WC, NC) > c32::kPlanBudget || c32::stage_chunks(in_px, t.CK, in_u8) > chunk_cap);
    };
    // (rows wider than one row's tile budget -- the uint8 input layer of a 1280-px side, stride 2: 3 x 1025 staged pixels: narrower
    //  column tiles of whole fragments; a row that fits keeps its width, so no 416- / 128-px plan moves)
    while (t.TW > 16 && !fits(1, t.TW)) t.TW = (t.TW - 1) / 16 * 16;
    const int tiles_x = (Wout + t.TW - 1) / t.TW;
    int best_th = 1;
    int64_t best_cost = -1;
    for (int th = 1; th <= std::min(Hout, maxpix / t.TW); ++th) {
        if (!fits(th, t.TW)) break;
        // time ~ tiles x (fragments of the busiest wave + the fixed cost of a stage: barriers + LDS commit, about one fragment's MFMAs)
        const int mfm = std::max(((th * t.TW + 15) / 16 + WP - 1) / WP, MFMN);
        const int64_t cost = (int64_t)((Hout + th - 1) / th) * tiles_x * (mfm * NC + 1);
        if (best_cost < 0 || cost <= best_cost) { best_cost = cost; best_th = th; }
    }
    t.TH = best_th;
    t.NI = 1;
    if (cost_out) *cost_out = best_cost;
    if (NC == 1 && !in_u8 && t.TH == Hout && t.TW == Wout && Hout * Wout * 2 <= maxpix) {
        // a small map (the 128-px scale's 8 x 8 / 4 x 4 levels): one tile = NI whole images, as many as the fragment budget, the LDS
        // tile and the staging plan take -- a tile of ONE such map would leave most of the workgroup's fragments empty
        const int64_t in1 = c32::tile_in_px(Hout, Wout, stride, ks);
        int ni = maxpix / (Hout * Wout);
        while (ni > 1 && (c32::lds_plan(ni * in1, ks, t.CK, t.WC, 1) > c32::kPlanBudget || c32::stage_chunks(ni * in1, t.CK, false) > chunk_cap)) --ni;
        t.NI = ni;
    }
    t.MFM = std::max(((t.NI * t.TH * t.TW + 15) / 16 + WP - 1) / WP, MFMN);
    return t;
}

bool conv32_tail_supported(const Conv32Tiling &t, int cout1, int cout2) {
    if (cout1 != 16 * t.WC || (cout1 != 16 && cout1 != 32 && cout1 != 64)) return false;  // the whole producer in one workgroup
    if (cout2 < 1 || cout2 > 64) return false;
    return c32::tail_bytes(t.WC, t.MFM, cout1) <= c32::kLaunchCap;
}

Conv32Tiling plan_dwpw32(int cin, int cout, int H, int W) {
    Conv32Tiling t{0, 0, 16, 4, 0, 1, 1};
    if (cin % 16 || cout % 64 || W > 224) return t;
    const int WP = c32::kNW / t.WC, maxpix = c32::tile_pixels(t.WC, c32::mfm_max(t.WC));
    t.TW = W;
    int best = 0;
    int64_t best_cost = -1;
    for (int th = 1; th <= std::min(H, maxpix / W); ++th) {
        const int64_t in_px = c32::tile_in_px(th, W, 1, 3);
        if (c32::lds_dw(in_px, (int64_t)th * W, t.CK, t.WC) > c32::kPlanBudget || c32::stage_chunks(in_px, t.CK, false) > c32::chunk_cap(false, true, false, false, 1)) break;
        const int mfm = std::max(((th * W + 15) / 16 + WP - 1) / WP, c32::mfm_min(t.WC));
        const int64_t cost = (int64_t)((H + th - 1) / th) * (mfm + 1);
        if (best_cost < 0 || cost <= best_cost) { best_cost = cost; best = th; }
    }
    // (a tile is whole rows of ONE image: the 8 x 8 / 4 x 4 maps of the 128-px scale would fill 64 / 16 of a workgroup's >= 128 pixel slots
    // -- measured 8192 tiles: 452 us at 10.8 TFLOP/s for the 4 x 4 pair -- and keep their separate depthwise + flattened 1x1 launches)
    if (!best || best * W < 112) return t;
    t.TH = best;
    t.MFM = std::max(((t.TH * W + 15) / 16 + WP - 1) / WP, c32::mfm_min(t.WC));
    return t;
}

std::vector<float> pack_dwpw32_weights(const float *pw, int cout, int cin, const float *dw_c9, const float *dw_bias, const Conv32Tiling &t) {
    const int CK = t.CK, nstage = cin / CK, ncb = cout / (16 * t.WC);
    const std::vector<float> base = pack_conv32_weights(pw, cout, cin, 1, t, nullptr, false);  // [cb][stage][wc][kst][lane][4]
    const size_t blk = (size_t)t.WC * c32::wfloats(1, CK), dwn = (size_t)c32::dw_taps_bytes(CK) / 4;
    std::vector<float> out((size_t)ncb * nstage * (blk + dwn), 0.f);
    for (int cb = 0; cb < ncb; ++cb)
        for (int st = 0; st < nstage; ++st) {
            float *dst = out.data() + ((size_t)cb * nstage + st) * (blk + dwn);
            std::copy(base.begin() + ((size_t)cb * nstage + st) * blk, base.begin() + ((size_t)cb * nstage + st + 1) * blk, dst);
            for (int c = 0; c < CK; ++c) {
                for (int tp = 0; tp < 9; ++tp) dst[blk + (size_t)tp * CK + c] = dw_c9[(size_t)(st * CK + c) * 9 + tp];
                dst[blk + (size_t)9 * CK + c] = dw_bias[st * CK + c];
            }
        }
    return out;
}

std::vector<float> pack_conv32_weights(const float *w, int cout, int cin, int ks, const Conv32Tiling &t, const int *perm, bool in_u8) {
    const int CK = t.CK, cpk = CK / 4;
    const int cin_eff = in_u8 ? 4 : cin;
    const int nstage = (cin_eff + CK - 1) / CK;
    const int kst = c32::kfull(ks, CK), krem = c32::krem(ks, CK);
    const int NC = std::max(1, t.NC), nfb = t.WC * NC;  // fragments per cout block
    const int nf = (cout + 15) / 16;
    const int nfp = (nf + nfb - 1) / nfb * nfb;  // whole cout blocks
    const int taps = ks * ks;
    std::vector<float> out((size_t)nfp * nstage * c32::wfloats(ks, CK), 0.f);
    size_t o = 0;
    auto wat = [&](int co, int st, int q, int s) -> float {  // weight of cout co for channel s of the stage's chunk q
        const int tap = q / cpk, c = st * CK + (q % cpk) * 4 + s;
        if (co >= cout || c >= cin || q >= taps * cpk) return 0.f;
        return w[((size_t)(perm ? perm[co] : co) * cin + c) * taps + tap];
    };
    // cout of accumulator row r (= lane & 15) of the block's fragment f: one fragment per wave -> 16 f + r; two (NC = 2) -> the wave's 32 couts
    // interleaved so that a lane's 4 + 4 rows (g * 4 + j of both fragments) are 8 consecutive couts: 32 (f / 2) + (r >> 2) * 8 + (f & 1) * 4 + (r & 3)
    auto cout_of = [&](int cb, int f, int r) { return cb * nfb * 16 + (NC == 2 ? 32 * (f >> 1) + (r >> 2) * 8 + (f & 1) * 4 + (r & 3) : 16 * f + r); };
    // [cout block][stage][fragment of the block]{[piece][lane][4], [remainder chunk][lane]}: a workgroup's stage is one contiguous run
    for (int cb = 0; cb < nfp / nfb; ++cb)
        for (int st = 0; st < nstage; ++st)
            for (int f = 0; f < nfb; ++f) {
                for (int k = 0; k < kst; ++k)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int s = 0; s < 4; ++s) out[o++] = wat(cout_of(cb, f, lane & 15), st, k * 4 + (lane >> 4), s);
                for (int r = 0; r < krem; ++r)
                    for (int lane = 0; lane < 64; ++lane) out[o++] = wat(cout_of(cb, f, lane & 15), st, kst * 4 + r, lane >> 4);
            }
    return out;
}

size_t conv32_lds_bytes(const Conv32Launch &L) {
    const int sks = L.dw ? 3 : L.ks;  // staged halo
    const int64_t in_px = std::max(1, L.NI) * c32::tile_in_px(L.TH, L.TW, L.stride, sks);
    const int64_t lds = L.dw ? c32::lds_dw(in_px, (int64_t)L.TH * L.TW, L.CK, L.WC) : c32::lds_conv(in_px, L.ks, L.CK, L.WC, std::max(1, L.NC));  // activation tile(s) + stage weights
    return (size_t)(L.tail_cout > 0 ? std::max(lds, c32::tail_bytes(L.WC, L.MFM, L.cout)) : lds);
}

hipError_t conv32_params(const Conv32Launch &L, C32Params *P_out, dim3 *grid_out, size_t *lds_out, int *tail_wc2_out) {
    if (L.res.cpb || L.tail_out.cpb) return hipErrorInvalidValue;  // plain NHWC only
    {   // channel-blocked (by 8) tensors: see C32Params
        auto blk8 = [](const TensorRef &t) { return t.cpb == 2 && t.cs == 8 && t.co % 8 == 0 && t.ps > 0 && t.ps < (1ll << 28); };
        if (L.in.cpb && (!blk8(L.in) || L.in_u8 || L.up_c > 0 || (L.ks != 3 && !L.dw && !L.acc_init.p) || L.CK % 8 || L.cin % 8)) return hipErrorInvalidValue;
        if (L.in2.cpb && (!blk8(L.in2) || L.up_c <= 0 || L.CK % 8)) return hipErrorInvalidValue;
        // (1x1 layers are issued over the flattened batch: their blocked output needs the per-image split of out_hw)
        if (L.out.cpb && (!blk8(L.out) || L.tail_cout > 0 || L.cout % 8 || (L.ks == 1 && !L.dw && L.out_hw <= 0))) return hipErrorInvalidValue;
    }
    if ((L.ks != 1 && L.ks != 3) || (L.WC != 1 && L.WC != 2 && L.WC != 4) || (L.NC != 1 && L.NC != 2)) return hipErrorInvalidValue;
    if (L.NC == 2 && (L.cout % 32 || L.tail_cout > 0 || L.dw || L.in_u8 || L.NI > 1)) return hipErrorInvalidValue;
    C32Params &P = *P_out;
    memset(&P, 0, sizeof P);
    P.in = L.in.p; P.in_bs = L.in.bs; P.in_cs = L.in.cs; P.in_co = L.in.co;
    P.out = (float *)L.out.p; P.out_bs = L.out.bs; P.out_cs = L.out.cs; P.out_co = L.out.co;
    if (L.in.cpb) { P.in_blk = 1; P.in_ps = (int)L.in.ps; P.in = (const float *)L.in.p + (int64_t)(L.in.co >> 3) * L.in.ps; P.in_co = 0; }
    if (L.out.cpb) { P.out_blk = 1; P.out_ps = (int)L.out.ps; }
    P.in_sadd = L.in.cpb ? (unsigned)((int64_t)(L.CK / 8) * L.in.ps * 4) : (unsigned)(L.CK * 4);
    P.res = (const float *)L.res.p; P.res_bs = L.res.bs; P.res_cs = L.res.cs; P.res_co = L.res.co;
    P.wpk = L.wpk; P.bias = L.bias; P.lut = L.lut;
    P.Hin = L.Hin; P.Win = L.Win; P.Hout = L.Hout; P.Wout = L.Wout; P.cin = L.cin; P.cout = L.cout; P.stride = L.stride; P.act = L.act;
    P.flip_bgr = L.flip_bgr;
    P.TH = L.TH; P.TW = L.TW; P.CK = L.CK; P.sh = ilog2_(L.CK / 4);
    if ((4 << P.sh) != L.CK && !(L.ks == 1 && L.CK == 48 && !L.up_c && !L.in_u8)) return hipErrorInvalidValue;
    const int NI = std::max(1, L.NI);
    if (L.MFM < 1 || L.MFM > c32::mfm_max(L.WC, L.NC) || NI * L.TH * L.TW > c32::tile_pixels(L.WC, L.MFM) || L.TH < 1 || L.TW < 1) return hipErrorInvalidValue;
    if (NI > 1 && (L.ks != 3 || L.in_u8 || L.up_c || L.tiles_x != 1 || L.tiles_y != 1 || L.TH != L.Hout || L.TW != L.Wout || L.out_hw || L.tail_out_hw)) return hipErrorInvalidValue;
    P.NI = NI; P.B = L.B; P.dw_act = L.dw_act;
    if (L.dw && (L.ks != 1 || L.stride != 1 || L.in_u8 || L.up_c || NI != 1 || L.WC != 4 || L.CK != 16 || L.out_hw || L.tail_out_hw || L.Hin != L.Hout || L.Win != L.Wout || L.TW != L.Wout ||
                 L.tiles_x != 1)) return hipErrorInvalidValue;
    const int cin_eff = L.in_u8 ? 4 : L.cin;
    if (!L.in_u8 && (L.cin % L.CK || (L.in.cs & 3) || (L.in.co & 3))) return hipErrorInvalidValue;
    if (L.in_u8 && (L.CK != 4 || (L.cin != 3 && L.cin != 4) || !L.lut)) return hipErrorInvalidValue;
    if (L.res.p && ((L.res.cs | L.res.co) & 3)) return hipErrorInvalidValue;
    P.nstage = (cin_eff + L.CK - 1) / L.CK;
    P.kst = c32::kfull(L.ks, L.CK); P.krem = c32::krem(L.ks, L.CK); P.wcb = c32::wfloats(L.ks, L.CK) * 4;
    P.tiles_x = L.tiles_x; P.tiles_y = L.tiles_y; P.out_hw = L.out_hw;
    const int64_t ntiles = NI > 1 ? ((int64_t)L.B + NI - 1) / NI : (int64_t)L.B * L.tiles_y * L.tiles_x;
    P.ncb = (L.cout + 16 * L.WC * L.NC - 1) / (16 * L.WC * L.NC);
    if (ntiles < 1 || (ntiles + 7) / 8 * 8 * P.ncb >= (1ll << 31)) return hipErrorInvalidValue;
    P.ntiles = (int)ntiles;
    const int sks = L.dw ? 3 : L.ks;  // staged halo
    const int TWin = c32::tile_in(L.TW, L.stride, sks), THin = c32::tile_in(L.TH, L.stride, sks);
    P.inv_twin = 1.0f / (float)TWin;
    P.inv_tw = 1.0f / (float)L.TW;
    {
        int64_t span = ((int64_t)L.Hin * L.Win * L.in.cs - L.in.co) * 4 + (int64_t)(NI - 1) * L.in.bs * 4;  // from the slice's first element to the end of the (last) image
        if (L.in.cpb) span = (L.in.bs - (int64_t)(L.in.co >> 3) * L.in.ps) * 4 + (int64_t)(NI - 1) * L.in.bs * 4;
        if (L.up_c > 0) {  // virtual [upsample | skip] concat: 1-D 1x1 launches over plain NHWC sources only
            if (L.ks != 1 || L.in_u8 || L.B != 1 || L.Hin != 1 || !L.in2.p || L.up_c % L.CK || L.up_c >= L.cin || (L.up_W & 1) || (L.up_HW % L.up_W) ||
                ((L.up_HW / L.up_W) & 1) || L.Win % L.up_HW || (L.in2.cs & 3) || (L.in2.co & 3))
                return hipErrorInvalidValue;
            span = ((int64_t)(L.Win / 4) * L.in.cs - L.in.co) * 4;  // the low-resolution source
            int64_t s2 = ((int64_t)L.Win * L.in2.cs - L.in2.co) * 4;
            P.in2 = L.in2.p; P.in2_cs = L.in2.cs; P.in2_co = L.in2.co;
            P.in2_bs = (int64_t)L.up_HW * L.in2.cs; P.in2_sadd = (unsigned)(L.CK * 4);
            if (L.in2.cpb) {  // the skip tensor in 8-channel blocks per image
                P.in2_blk = 1; P.in2_ps = (int)L.in2.ps; P.in2_bs = L.in2.bs;
                P.in2 = (const float *)L.in2.p + (int64_t)(L.in2.co >> 3) * L.in2.ps; P.in2_co = 0;
                P.in2_sadd = (unsigned)((int64_t)(L.CK / 8) * L.in2.ps * 4);
                s2 = ((int64_t)(L.Win / L.up_HW) * L.in2.bs - (int64_t)(L.in2.co >> 3) * L.in2.ps) * 4;
            }
            if (s2 <= 0 || s2 >= (1ll << 32) - 65536) return hipErrorInvalidValue;
            P.in2_span_bytes = (unsigned)s2;
            P.up_c = L.up_c; P.up_W = L.up_W; P.up_HW = L.up_HW; P.up_stages = L.up_c / L.CK;
        }
        if (L.acc_init.p) {  // (see AINIT in k_conv_f32) 1-D 1x1 over the skip tensor of `Win / up_HW` whole images
            if (L.ks != 1 || L.in_u8 || L.dw || L.up_c || L.tail_cout > 0 || L.B != 1 || L.Hin != 1 || NI != 1 || L.NC != 2 || L.cout % 32 || L.up_W < 2 || (L.up_W & 1) ||
                L.up_HW < 4 || (L.up_HW % L.up_W) || ((L.up_HW / L.up_W) & 1) || L.Win % L.up_HW || L.acc_init.cpb || ((L.acc_init.cs | L.acc_init.co) & 3) ||
                L.acc_init.cs < L.acc_init.co + L.cout)
                return hipErrorInvalidValue;
            const int64_t nimg = L.Win / L.up_HW;
            if (L.in.cpb) span = (nimg * L.in.bs - (int64_t)(L.in.co >> 3) * L.in.ps) * 4;
            else if (L.in.bs != (int64_t)L.up_HW * L.in.cs) return hipErrorInvalidValue;  // dense images: the flattened pixel row
            const int64_t si = (nimg * (L.up_HW / 4) * L.acc_init.cs - L.acc_init.co) * 4;
            if (si <= 0 || si >= (1ll << 32) - 65536) return hipErrorInvalidValue;
            P.ini = (const float *)L.acc_init.p + L.acc_init.co; P.ini_cs = L.acc_init.cs; P.ini_span_bytes = (unsigned)si;
            P.up_W = L.up_W; P.up_HW = L.up_HW;
        }
        if (!L.in_u8 && (span <= 0 || span >= (1ll << 32) - 65536)) return hipErrorInvalidValue;  // 32-bit buffer offsets
        P.in_span_bytes = L.in_u8 ? 0u : (unsigned)span;
    }
    if (c32::stage_chunks((int64_t)NI * THin * TWin, L.CK, L.in_u8) > c32::chunk_cap(L.in_u8, L.dw, L.up_c > 0, L.acc_init.p != nullptr, L.ks)) return hipErrorInvalidValue;  // staging plan: chunks per thread
    int tail_wc2 = 0;
    if (L.tail_cout > 0) {
        const Conv32Tiling t{L.TH, L.TW, L.CK, L.WC, L.MFM, NI};
        if (!conv32_tail_supported(t, L.cout, L.tail_cout) || P.ncb != 1 || !L.tail_w || !L.tail_b || !L.tail_out.p || L.res.p) return hipErrorInvalidValue;
        tail_wc2 = L.tail_cout > 32 ? 4 : (L.tail_cout > 16 ? 2 : 1);
        if (L.WC == 1 && tail_wc2 != 1) return hipErrorInvalidValue;
        if (L.WC == 2 && tail_wc2 != 2) { if (tail_wc2 == 1) tail_wc2 = 2; else return hipErrorInvalidValue; }  // (a 16-cout tail behind a 32-cout layer: the second fragment is empty)
        P.w2 = L.tail_w; P.b2 = L.tail_b; P.out2 = (float *)L.tail_out.p; P.out2_bs = L.tail_out.bs; P.out2_cs = L.tail_out.cs; P.out2_co = L.tail_out.co;
        P.out2_hw = L.tail_out_hw; P.cout2 = L.tail_cout; P.act2 = L.tail_act; P.kst2 = L.cout / 16;
        if (L.cmax) {
            if (tail_wc2 != 1 || L.tail_act) return hipErrorInvalidValue;  // (one cout fragment holds all the logits; plain outputs)
            P.cmax = L.cmax; P.cmax_bs = L.cmax_bs;
        }
    }
    P.tstep = L.xtile ? 1 : 0;
    const size_t lds = conv32_lds_bytes(L);
    if (lds > (size_t)c32::kLaunchCap || P.kst > c32::kfull_max(L.ks)) return hipErrorInvalidValue;  // (kst bound: the weight-fetch plan of the kernel, MAXW)
    *grid_out = dim3((unsigned)((ntiles + 7) / 8 * 8 * P.ncb));
    *lds_out = lds;
    *tail_wc2_out = tail_wc2;
    return hipSuccess;
}

// [fragment nf][k step t][lane]: weight of cout 16 nf + (lane & 15) for k = 4 t + (lane >> 4), k = (ky * 3 + kx) * cin + c over the
// channels AS STORED in the tile (flip_bgr: stored BGR, the conv's channel order is RGB)
std::vector<float> pack_stem32_weights(const float *w, int cout, int cin, bool flip_bgr) {
    const int K = 9 * cin, KST = (K + 3) / 4, NF = cout / 16;
    std::vector<float> out((size_t)NF * KST * 64, 0.f);
    for (int nf = 0; nf < NF; ++nf)
        for (int t = 0; t < KST; ++t)
            for (int lane = 0; lane < 64; ++lane) {
                const int k = 4 * t + (lane >> 4), co = nf * 16 + (lane & 15);
                if (k >= K) continue;
                const int tap = k / cin, c = k % cin;
                const int cs = (flip_bgr && c < 3) ? 2 - c : c;
                out[((size_t)nf * KST + t) * 64 + lane] = w[((size_t)co * cin + cs) * 9 + tap];
            }
    return out;
}

}  // namespace obb
