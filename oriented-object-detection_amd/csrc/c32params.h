// Kernel parameters of k_conv_f32 (f32path.hip), filled by conv32_params (f32plan.hip) from a Conv32Launch.
#pragma once
#include "f32path.h"

namespace obb {

struct C32Params {
    const void *in; int64_t in_bs; int in_cs, in_co;
    const void *in2; int in2_cs, in2_co; unsigned in2_span_bytes; int up_c, up_W, up_HW;  // VCAT: second source of a virtual [upsample | skip] concat
    float *out; int64_t out_bs; int out_cs, out_co;
    const float *res; int64_t res_bs; int res_cs, res_co;
    const float *wpk, *bias, *lut;
    const float *w2, *b2; float *out2; int64_t out2_bs; int out2_cs, out2_co, out2_hw, cout2, act2, kst2;  // TAIL: fused trailing 1x1
    float *cmax; int64_t cmax_bs;  // TAIL = 1 over the class logits: per-anchor maximum of the tail's outputs (nullptr: none)
    int Hin, Win, Hout, Wout, cin, cout, stride, act, flip_bgr;
    int TH, TW, CK, sh /*log2(CK/4)*/, tiles_x, tiles_y, ntiles, nstage, kst, out_hw, ncb;
    int krem, wcb;  // 4-channel chunks of a stage beyond the kst whole pieces (0..3: one MFMA each); bytes of one cout fragment's stage weights
    int dbg;    // diagnostic build (-DOBB_DIAG) only: timing ablations, see launch_conv32
    int tstep;  // > 0: resident workgroups, each walks the tiles t, t + tstep, ... (see XT in k_conv_f32)
    int dw_act;  // DW: SiLU behind the depthwise conv
    int NI, B;  // NI > 1: a tile = NI whole images of a small map (TH x TW = the map), B images in all
    float inv_twin, inv_tw;
    unsigned in_span_bytes;  // buffer-descriptor range of one image's input slice (its check returns zeros past the end)
    // channel-blocked tensors (TensorRef::cpb = 2: blocks of 8 channels, per image [C / 8][pixel][8], so that an 8- or 16-channel stage of a
    // 3x3 layer reads whole dense runs instead of 32- / 64-byte pieces of wide pixel rows -- measured x3.75 HBM re-read on model.3 with plain
    // NHWC): element (b, pixel, c) = b * bs + (c >> 3) * ps + pixel * 8 + (c & 7); cs = 8.  in: 2-D launches (3x3 / depthwise prologue);
    // in2: the skip source of a virtual concat; out: the layer's own output (not the TAIL's)
    int in_blk, in2_blk, out_blk, in_ps, in2_ps, out_ps, up_stages;
    int64_t in2_bs;
    unsigned in_sadd, in2_sadd;  // bytes from one channel stage to the next
    // AINIT: the accumulators of fine pixel (image, y, x) start from ini[(image, y >> 1, x >> 1)][cout] (plain NHWC at half the resolution;
    // up_W / up_HW = the fine level's width and pixels per image) instead of zero
    const float *ini; int ini_cs; unsigned ini_span_bytes;
};

// Everything launch_conv32 does before it picks a kernel: checks the launch (hipErrorInvalidValue if no kernel takes it) and fills the
// kernel parameters, the grid, the dynamic LDS size and the waves along cout of a fused tail (0: none).  Pure host arithmetic.
hipError_t conv32_params(const Conv32Launch &L, C32Params *P, dim3 *grid, size_t *lds, int *tail_wc2);

}  // namespace obb
