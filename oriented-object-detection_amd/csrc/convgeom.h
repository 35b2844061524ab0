// Tile geometry of the 16-bit conv family (k_conv_igemm, k_conv3_pair: conv.hip), stated once for the kernels, the planner, the
// packer and the launch checks (convplan.hip: plan_conv, pack_conv_weights, conv_params, conv_lds_bytes).  Plain constexpr
// arithmetic for host and device code; compiles with the host compiler alone (tests/host/convplan_main.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define C16_HD __host__ __device__
#else
#define C16_HD
#endif

namespace obb {
namespace c16 {

constexpr int kNT = 256;        // threads of a k_conv_igemm workgroup, and of each half-group of k_conv3_pair
constexpr int kFragBytes = 1024;  // one MFMA A-operand fragment (16 couts x 32 k): 64 lanes x 16 B

// Dynamic-LDS caps of a launch.  A kernel runs with up to kLdsDefault without further ado; the weights-resident rows of
// convvariants.h have their limit raised first (allow_dyn_lds).  The CU has 160 KiB: what the raised caps leave is for the kernels'
// static arrays -- k_conv_igemm: two bias blocks and the uint8 table; k_conv3_pair: two bias blocks.
constexpr int kLdsDefault = 64 * 1024;
constexpr int kLdsWres = 152 * 1024;
constexpr int kLdsPair = 158 * 1024;

C16_HD constexpr int64_t round16(int64_t bytes) { return (bytes + 15) / 16 * 16; }

// bytes per staged pixel: CK 16-bit channels + 16 B (the pad spreads consecutive pixels over the LDS banks); the 8-channel uint8 input
// layer packs its pixels densely (twice the groups per CU)
C16_HD constexpr int pix_pitch(bool in_u8, int CK) { return in_u8 ? 16 : CK * 2 + 16; }

// input rows / columns staged for t output rows / columns
C16_HD constexpr int tile_in(int t, int stride, int ks) { return (t - 1) * stride + ks; }

// 16-byte chunks a thread may stage per channel stage (the kernels' MAXLD); a stage holds at most that many x kNT chunks of 8 channels
C16_HD constexpr int maxld(bool wres, int ks) { return wres ? 8 : (ks == 1 ? 4 : 6); }
C16_HD constexpr int chunk_cap(bool wres, int ks) { return maxld(wres, ks) * kNT; }
C16_HD constexpr int64_t stage_chunks(int NI, int TH, int TW, int stride, int ks, int CK) { return (int64_t)NI * tile_in(TH, stride, ks) * tile_in(TW, stride, ks) * (CK / 8); }

// 32-deep MFMA steps of one channel stage: k = taps x CK channels in chunks of 8, four chunks per step, the last step zero-padded
C16_HD constexpr int ksteps(int ks, int CK) { return ((ks == 3 ? 9 : 1) * (CK / 8) + 3) / 4; }
// bytes of one stage's weights of a workgroup (NF cout fragments per step)
C16_HD constexpr int stage_weight_bytes(int kst, int NF) { return kst * NF * kFragBytes; }

// the 16-bit output tile staged for the coalesced write-out: a row of 16 * NF halves + 16 B pad per pixel, 64 * MF pixels
C16_HD constexpr int out_row_bytes(int NF) { return 32 * NF + 16; }
C16_HD constexpr int64_t out_tile_bytes(int MF, int NF, bool out_f32) { return out_f32 ? 0 : (int64_t)64 * MF * out_row_bytes(NF); }

// LDS layout: [input tile (one channel stage) | weights of the stage | weights of a fused tail].  The epilogue's output staging starts
// at offset 0; for multi-stage layers it may run over the weights as well (they are re-staged at every stage anyway), single-stage
// layers keep their weights resident across tiles, so there the staging area must fit in front of them.
C16_HD constexpr int64_t act_bytes(int NI, int TH, int TW, int stride, int ks, int CK, bool in_u8, bool multi_stage, int MF, int NF, bool out_f32) {
    const int64_t in_tile = (int64_t)(NI > 1 ? NI : 1) * tile_in(TH, stride, ks) * tile_in(TW, stride, ks) * pix_pitch(in_u8, CK);
    const int64_t out_tile = out_tile_bytes(MF, NF, out_f32);
    return round16(multi_stage ? in_tile : (in_tile > out_tile ? in_tile : out_tile));
}
C16_HD constexpr int64_t main_lds(int64_t act, int ks, int CK, int MF, int NF, bool out_f32) {
    const int64_t a = act + stage_weight_bytes(ksteps(ks, CK), NF), out_tile = out_tile_bytes(MF, NF, out_f32);
    return round16(a > out_tile ? a : out_tile);
}
// a fused trailing 1x1 over the 16 * NF staged channels, nf2 cout fragments
C16_HD constexpr int tail_ksteps(int NF) { return ksteps(1, 16 * NF); }
C16_HD constexpr int tail_weight_bytes(int NF, int nf2) { return stage_weight_bytes(tail_ksteps(NF), nf2); }
// k_conv3_pair: [input tile of half 0 | of half 1 | the resident weights, nf fragments per step | the tail's 2 steps x 4 fragments]
C16_HD constexpr int64_t pair_lds(int64_t act, int kst, int nf, bool tail) { return 2 * act + stage_weight_bytes(kst, nf) + (tail ? tail_weight_bytes(4, 4) : 0); }

// elements of a layer's packed weights: [cout block][stage][k step][NF fragments][64 lanes][8]
C16_HD constexpr int cout_blocks(int cout, int NF) { return (cout + 16 * NF - 1) / (16 * NF); }
C16_HD constexpr int stages(int cin, int CK, bool in_u8) { return ((in_u8 ? 8 : cin) + CK - 1) / CK; }
C16_HD constexpr int64_t packed_elems(int cout, int cin, int ks, int NF, int CK, bool in_u8) {
    return (int64_t)cout_blocks(cout, NF) * stages(cin, CK, in_u8) * ksteps(ks, CK) * NF * 64 * 8;
}

// The two-waves-per-SIMD register class of k_conv_igemm: the 64-cout 3x3 variants need ~210 VGPRs; everything else fits 168 without
// spills, which is the difference between two and three resident waves per SIMD (allocation granule 8: 170 registers already drop to
// two).  The class has the registers for two operand sets in the k loop (DBUF).
C16_HD constexpr bool two_waves(int KS, int MF, int NF) { return NF == 4 && (KS == 3 ? MF >= 2 : MF == 3); }

}  // namespace c16
}  // namespace obb
