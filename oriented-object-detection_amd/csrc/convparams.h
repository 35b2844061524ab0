// Kernel parameters of k_conv_igemm / k_conv3_pair (conv.hip) and the kernel variant of a launch, both filled by conv_params
// (convplan.hip) from a ConvLaunch.
#pragma once
#include "conv.h"

namespace obb {

struct ConvParams {
    const void *in; int64_t in_bs; int in_cs, in_co;
    void *out; int64_t out_bs; int out_cs, out_co;
    const bf16_t *res; int64_t res_bs; int res_cs, res_co;
    // channel-blocked addressing (TensorRef::cpb): chunk cc of a pixel lives at (cc >> bsh) * ps + pixel * pp + (cc & bmask) * 8 elements;
    // plain NHWC is the degenerate case bsh = 31, bmask = ~0, pp = cs
    int in_bsh, in_bmask; unsigned in_ps2 /*bytes*/;
    int out_bsh, out_bmask; int64_t out_ps;
    int res_bsh, res_bmask; int64_t res_ps;
    const bf16_t *wpk; const float *bias; const bf16_t *lut;
    int Hin, Win, Hout, Wout, cin, cout, stride, act, flip_bgr;
    int TH, TW, CK, sh /*log2(CK/8)*/, tiles_x, tiles_y, nstage, kst, out_hw, act_bytes;
    int tpw, ntiles;  // consecutive pixel tiles per workgroup; total pixel tiles (batch included)
    int NI, B;        // NI > 1: a tile = NI whole images of a small map (TH x TW = the map: the 4 x 4 level of the 128-px scale), B images in all
    int gx, ncb;      // workgroups along the tile axis; cout blocks
    unsigned in_span_bytes, w_bytes;  // buffer-descriptor ranges: bytes of one image's input slice span; bytes of the packed weights
    // 1x1 over a virtual concat [nearest-x2 upsample of a low-res tensor | full-res tensor] (1-D launches only): channels [0, up_c) come
    // from `in` (low-res NHWC slice, pixel (b, y/2, x/2)), the rest from `in2`; neither the upsampled tensor nor the concat is ever stored
    const void *in2; int in2_cs, in2_co; unsigned in2_span_bytes; int up_c, up_W, up_HW;
    // fused trailing 1x1 conv (TAIL): out2[pixel][cout2] = W2 . y[pixel][0 .. 16*NF) + bias2, fp32 rows of the head tensor
    const bf16_t *w2pk; const float *bias2; float *out2; int64_t out2_bs; int out2_cs, out2_co, out2_hw, cout2, kst2, w2_off;
    unsigned long long *stamps;  // diagnostic build (-DOBB_STAMPS) only
    int dbg;  // timing experiments only (OBB_CONV_DBG): 1 skip MFMA loop, 2 skip activation loads, 4 skip SiLU, 8 skip stores, 16 skip weight loads
    float inv_twin, inv_tw;
};

// The kernel instantiation a launch runs: k_conv_igemm's template arguments, or (pair) those of k_conv3_pair -- (F16, TAIL, S, NF), the
// other fields zero.  convvariants.h lists the ones the library builds.
struct ConvVariant {
    bool pair = false;
    int KS = 0, MF = 0, NF = 0;
    bool IN_U8 = false, OUT_F32 = false, F16 = false;
    int TAIL = 0;
    bool VCAT = false, T16 = false, WRES = false, NIT = false;
    int S = 0;  // k_conv3_pair: stride
};

// Everything launch_conv does before it picks a kernel: checks the launch (hipErrorInvalidValue if no kernel takes it) and fills the
// kernel parameters, the variant, the 1-D grid, the workgroup size and the dynamic LDS size.  Pure host arithmetic.
hipError_t conv_params(const ConvLaunch &L, ConvParams &P, ConvVariant &V, unsigned &grid_x, unsigned &threads, size_t &lds);
// Name of the check that refused the calling thread's last conv_params call ("" after an accepted one): one name per refusing return,
// e.g. "lut", "staging", "variant" (no row in convvariants.h).  For error messages and for tests/host/convplan_main.cpp.
const char *conv_params_refusal();

}  // namespace obb
