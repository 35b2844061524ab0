// Tile geometry of the fp32 conv family (k_conv_f32, f32path.hip), stated once for the kernel, the planner (f32plan.hip:
// plan_conv32, plan_dwpw32), the packers and the launch checks (conv32_params, conv32_lds_bytes).  Plain constexpr arithmetic for
// host and device code; compiles with the host compiler alone (tests/host/f32plan_main.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define C32_HD __host__ __device__
#else
#define C32_HD
#endif

namespace obb {
namespace c32 {

constexpr int kNW = 8;        // waves per workgroup
constexpr int kNT = kNW * 64;  // threads per workgroup

// Two LDS limits, both kept as they are: the planner sizes a tile on the UNROUNDED sum of activation tile and stage weights against
// kPlanBudget; the launch rounds the activation tile up to whole KiB (the weights start on a KiB boundary behind it) and refuses above
// kLaunchCap (two workgroups per CU).  The 2 KiB between them cover that rounding, so a planned tile always launches.
constexpr int kPlanBudget = 78 * 1024;
constexpr int kLaunchCap = 80 * 1024;

template <class T>
C32_HD constexpr T round_kib(T bytes) { return (bytes + 1023) & ~(T)1023; }

// bytes per staged pixel: CK channels (+16 B spreads consecutive pixels over the banks); per pixel of a fused tail's [pixel][cout] tile
C32_HD constexpr int pix_pitch(int CK) { return CK * 4 + 16; }
C32_HD constexpr int tail_pitch(int cout) { return cout * 4 + 16; }

// input rows / columns staged for t output rows / columns (sks = 3 with a depthwise prologue, else the kernel size)
C32_HD constexpr int tile_in(int t, int stride, int sks) { return (t - 1) * stride + sks; }
C32_HD constexpr int64_t tile_in_px(int th, int tw, int stride, int sks) { return (int64_t)tile_in(th, stride, sks) * tile_in(tw, stride, sks); }

// a stage's k = taps x CK channels in 4-channel chunks: kfull pieces of 4 chunks (four MFMAs behind one ds_read_b128 per operand) + krem
// single chunks (one MFMA each); wfloats = weights of one cout fragment and stage
// (1x1: whole pieces only, the last one zero-padded -- no 1x1 layer of the network has fewer than 16 input channels, and the remainder
// loop's registers are what the 1x1 forms at 7 fragments per wave do not have)
C32_HD constexpr int kfull(int ks, int CK) { return ks == 3 ? (9 * (CK / 4)) / 4 : (CK / 4 + 3) / 4; }
C32_HD constexpr int krem(int ks, int CK) { return ks == 3 ? (9 * (CK / 4)) % 4 : 0; }
C32_HD constexpr int wfloats(int ks, int CK) { return kfull(ks, CK) * 256 + krem(ks, CK) * 64; }
C32_HD constexpr int kfull_max(int ks) { return ks == 3 ? 9 : 4; }  // the kernel's weight-fetch plan (MAXW) holds that many pieces per fragment

// 16-byte chunks a thread may stage per channel stage (the kernel's MAXLD; AINIT: 192 pixels x 64 channels); a stage holds at most
// that many x kNT chunks.  (Only 1x1 launches have the dw / vcat / ainit forms.)
C32_HD constexpr int maxld(bool in_u8, bool dw, bool vcat, bool ainit, int ks) { return in_u8 ? 3 : (dw ? 3 : (vcat ? 4 : (ks == 3 ? 5 : (ainit ? 6 : 7)))); }
C32_HD constexpr int chunk_cap(bool in_u8, bool dw, bool vcat, bool ainit, int ks) { return maxld(in_u8, dw, vcat, ainit, ks) * kNT; }
C32_HD constexpr int64_t stage_chunks(int64_t in_px, int CK, bool in_u8) { return in_px * (in_u8 ? 1 : CK / 4); }

// pixel fragments (16 pixels) per wave: the largest and the smallest instantiated count (smaller tiles run it partly empty) for WC waves
// along cout and NC cout fragments per wave; a tile holds 16 * (kNW / WC) * MFM pixels (224 / 256 / 512 with NC = 1)
C32_HD constexpr int mfm_max(int WC, int NC = 1) { return NC == 2 ? 4 : (WC == 4 ? 7 : 4); }
C32_HD constexpr int mfm_min(int WC, int NC = 1) { return NC == 2 ? 3 : (WC == 4 ? 4 : (WC == 2 ? 2 : 1)); }
C32_HD constexpr int tile_pixels(int WC, int MFM) { return 16 * (kNW / WC) * MFM; }

// LDS bytes: the activation tile of in_px staged pixels; the depthwise form's second tile (its outputs, npix pixels) and the taps block
// (9 taps + bias of the stage's channels) behind the stage weights; one stage's weights of a workgroup; the fused tail's tile
C32_HD constexpr int64_t act_bytes(int64_t in_px, int CK) { return in_px * pix_pitch(CK); }
C32_HD constexpr int64_t act_bytes_kib(int64_t in_px, int CK) { return round_kib(act_bytes(in_px, CK)); }
C32_HD constexpr int64_t dw_taps_bytes(int CK) { return 10 * CK * 4; }
C32_HD constexpr int64_t weight_bytes(int ks, int CK, int WC, int NC) { return (int64_t)WC * NC * wfloats(ks, CK) * 4; }
C32_HD constexpr int64_t tail_bytes(int WC, int MFM, int cout) { return (int64_t)tile_pixels(WC, MFM) * tail_pitch(cout); }

// whole launches: what the planner budgets (unrounded), what the plain / VCAT / AINIT / uint8 forms and the depthwise form allocate
C32_HD constexpr int64_t lds_plan(int64_t in_px, int ks, int CK, int WC, int NC) { return act_bytes(in_px, CK) + weight_bytes(ks, CK, WC, NC); }
C32_HD constexpr int64_t lds_conv(int64_t in_px, int ks, int CK, int WC, int NC) { return act_bytes_kib(in_px, CK) + weight_bytes(ks, CK, WC, NC); }
C32_HD constexpr int64_t lds_dw(int64_t in_px, int64_t npix, int CK, int WC) { return act_bytes_kib(in_px, CK) + act_bytes_kib(npix, CK) + weight_bytes(1, CK, WC, 1) + dw_taps_bytes(CK); }

}  // namespace c32
}  // namespace obb
