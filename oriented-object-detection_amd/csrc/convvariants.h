// The kernels of the 16-bit conv family that the library builds, as data: one X() per k_conv_igemm instantiation and one per
// k_conv3_pair instantiation (114 + 10).  conv.hip expands the lists into the map variant -> kernel pointer (which is what instantiates the
// kernels: a row added here is a kernel built, a row removed one gone); conv_params (convplan.hip) refuses a launch whose variant has no
// row.  Plain C++: compiles with the host compiler alone (tests/host/convplan_main.cpp).
#pragma once
#include <cstdint>

#include "convgeom.h"
#include "convparams.h"

// X(KS, MF, NF, IN_U8, OUT_F32, F16, TAIL, VCAT, T16, WRES, NIT): the template arguments of k_conv_igemm (conv.hip).  One line per tile shape
// (KS, MF, NF) with the forms that shape has, for storage type F; every shape is built for F16 = true and false.  The forms, the fused ones first and the plain kernel last: WRES
// (weights resident; these rows run above the default LDS cap) with the fp32 head tail / plain, T16 (fused 16-bit tail: the cv1 of a
// C3k2 block behind a stride-2 conv), TAIL (fused fp32 head tail), IN_U8 (uint8 network input), OUT_F32 (head rows), NIT (multi-image
// tiles), VCAT (1x1 over a virtual [upsample | skip] concat).  The order of the rows is the order of the kernels in the code object.
#define OBB_C16_K3_M1_N1(X, F) X(3, 1, 1, 1, 0, F, 0, 0, 0, 0, 0) X(3, 1, 1, 0, 1, F, 0, 0, 0, 0, 0) X(3, 1, 1, 0, 0, F, 0, 0, 0, 0, 0)
#define OBB_C16_K3_M1_N2(X, F) X(3, 1, 2, 1, 0, F, 0, 0, 0, 0, 0) X(3, 1, 2, 0, 1, F, 0, 0, 0, 0, 0) X(3, 1, 2, 0, 0, F, 0, 0, 0, 0, 0)
#define OBB_C16_K3_M1_N4(X, F) X(3, 1, 4, 1, 0, F, 0, 0, 0, 0, 0) X(3, 1, 4, 0, 1, F, 0, 0, 0, 0, 0) X(3, 1, 4, 0, 0, F, 0, 0, 0, 0, 1) X(3, 1, 4, 0, 0, F, 0, 0, 0, 0, 0)
#define OBB_C16_K3_M2_N1(X, F) X(3, 2, 1, 1, 0, F, 0, 0, 0, 0, 0) X(3, 2, 1, 0, 1, F, 0, 0, 0, 0, 0) X(3, 2, 1, 0, 0, F, 0, 0, 0, 0, 0)
#define OBB_C16_K3_M2_N2(X, F) X(3, 2, 2, 1, 0, F, 0, 0, 0, 0, 0) X(3, 2, 2, 0, 1, F, 0, 0, 0, 0, 0) X(3, 2, 2, 0, 0, F, 0, 0, 0, 0, 0)
#define OBB_C16_K3_M2_N4(X, F) X(3, 2, 4, 1, 0, F, 0, 0, 0, 0, 0) X(3, 2, 4, 0, 1, F, 0, 0, 0, 0, 0) X(3, 2, 4, 0, 0, F, 0, 0, 0, 0, 0)
#define OBB_C16_K3_M3_N1(X, F) X(3, 3, 1, 0, 0, F, 1, 0, 0, 1, 0) X(3, 3, 1, 0, 0, F, 0, 0, 0, 1, 0) X(3, 3, 1, 0, 0, F, 1, 0, 0, 0, 0) X(3, 3, 1, 1, 0, F, 0, 0, 0, 0, 0) X(3, 3, 1, 0, 1, F, 0, 0, 0, 0, 0) X(3, 3, 1, 0, 0, F, 0, 0, 0, 0, 0)
#define OBB_C16_K3_M3_N2(X, F) X(3, 3, 2, 0, 0, F, 0, 0, 0, 1, 0) X(3, 3, 2, 0, 0, F, 2, 0, 1, 0, 0) X(3, 3, 2, 1, 0, F, 0, 0, 0, 0, 0) X(3, 3, 2, 0, 1, F, 0, 0, 0, 0, 0) X(3, 3, 2, 0, 0, F, 0, 0, 0, 0, 0)
#define OBB_C16_K3_M3_N4(X, F) X(3, 3, 4, 0, 0, F, 4, 0, 0, 1, 0) X(3, 3, 4, 0, 0, F, 0, 0, 0, 1, 0) X(3, 3, 4, 0, 0, F, 4, 0, 1, 0, 0) X(3, 3, 4, 0, 0, F, 4, 0, 0, 0, 0) X(3, 3, 4, 1, 0, F, 0, 0, 0, 0, 0) X(3, 3, 4, 0, 1, F, 0, 0, 0, 0, 0) X(3, 3, 4, 0, 0, F, 0, 0, 0, 0, 0)
#define OBB_C16_K1_M1_N1(X, F) X(1, 1, 1, 0, 1, F, 0, 0, 0, 0, 0) X(1, 1, 1, 0, 0, F, 0, 0, 0, 0, 0)
#define OBB_C16_K1_M1_N2(X, F) X(1, 1, 2, 0, 1, F, 0, 0, 0, 0, 0) X(1, 1, 2, 0, 0, F, 0, 0, 0, 0, 0)
#define OBB_C16_K1_M1_N4(X, F) X(1, 1, 4, 0, 1, F, 0, 0, 0, 0, 0) X(1, 1, 4, 0, 0, F, 0, 0, 0, 0, 0)
#define OBB_C16_K1_M2_N1(X, F) X(1, 2, 1, 0, 1, F, 0, 0, 0, 0, 0) X(1, 2, 1, 0, 0, F, 0, 0, 0, 0, 0)
#define OBB_C16_K1_M2_N2(X, F) X(1, 2, 2, 0, 1, F, 0, 0, 0, 0, 0) X(1, 2, 2, 0, 0, F, 0, 0, 0, 0, 0)
#define OBB_C16_K1_M2_N4(X, F) X(1, 2, 4, 0, 0, F, 1, 0, 0, 0, 0) X(1, 2, 4, 0, 0, F, 0, 1, 0, 0, 0) X(1, 2, 4, 0, 1, F, 0, 0, 0, 0, 0) X(1, 2, 4, 0, 0, F, 0, 0, 0, 0, 0)
#define OBB_C16_K1_M3_N1(X, F) X(1, 3, 1, 0, 1, F, 0, 0, 0, 0, 0) X(1, 3, 1, 0, 0, F, 0, 0, 0, 0, 0)
#define OBB_C16_K1_M3_N2(X, F) X(1, 3, 2, 0, 1, F, 0, 0, 0, 0, 0) X(1, 3, 2, 0, 0, F, 0, 0, 0, 0, 0)
#define OBB_C16_K1_M3_N4(X, F) X(1, 3, 4, 0, 1, F, 0, 0, 0, 0, 0) X(1, 3, 4, 0, 0, F, 0, 0, 0, 0, 0)
#define OBB_CONV_IGEMM_VARIANTS(X) \
    OBB_C16_K3_M1_N1(X, true) OBB_C16_K3_M1_N1(X, false) \
    OBB_C16_K3_M1_N2(X, true) OBB_C16_K3_M1_N2(X, false) \
    OBB_C16_K3_M1_N4(X, true) OBB_C16_K3_M1_N4(X, false) \
    OBB_C16_K3_M2_N1(X, true) OBB_C16_K3_M2_N1(X, false) \
    OBB_C16_K3_M2_N2(X, true) OBB_C16_K3_M2_N2(X, false) \
    OBB_C16_K3_M2_N4(X, true) OBB_C16_K3_M2_N4(X, false) \
    OBB_C16_K3_M3_N1(X, true) OBB_C16_K3_M3_N1(X, false) \
    OBB_C16_K3_M3_N2(X, true) OBB_C16_K3_M3_N2(X, false) \
    OBB_C16_K3_M3_N4(X, true) OBB_C16_K3_M3_N4(X, false) \
    OBB_C16_K1_M1_N1(X, true) OBB_C16_K1_M1_N1(X, false) \
    OBB_C16_K1_M1_N2(X, true) OBB_C16_K1_M1_N2(X, false) \
    OBB_C16_K1_M1_N4(X, true) OBB_C16_K1_M1_N4(X, false) \
    OBB_C16_K1_M2_N1(X, true) OBB_C16_K1_M2_N1(X, false) \
    OBB_C16_K1_M2_N2(X, true) OBB_C16_K1_M2_N2(X, false) \
    OBB_C16_K1_M2_N4(X, true) OBB_C16_K1_M2_N4(X, false) \
    OBB_C16_K1_M3_N1(X, true) OBB_C16_K1_M3_N1(X, false) \
    OBB_C16_K1_M3_N2(X, true) OBB_C16_K1_M3_N2(X, false) \
    OBB_C16_K1_M3_N4(X, true) OBB_C16_K1_M3_N4(X, false)

// X(F16, TAIL, S, NF): the template arguments of k_conv3_pair
#define OBB_C16_BOTH(X, ...) X(true, __VA_ARGS__) X(false, __VA_ARGS__)
#define OBB_CONV_PAIR_VARIANTS(X) OBB_C16_BOTH(X, 16, 2, 4) OBB_C16_BOTH(X, 0, 2, 4) OBB_C16_BOTH(X, 0, 1, 5) OBB_C16_BOTH(X, 4, 1, 4) OBB_C16_BOTH(X, 0, 1, 4)

namespace obb {

// one integer per variant (the case labels of the two lookups; 0 is no variant); a duplicate row is a duplicate case label
constexpr uint32_t conv_igemm_key(int KS, int MF, int NF, bool IN_U8, bool OUT_F32, bool F16, int TAIL, bool VCAT, bool T16, bool WRES, bool NIT) {
    return (uint32_t)KS | (uint32_t)MF << 4 | (uint32_t)NF << 8 | (uint32_t)TAIL << 12 | (uint32_t)IN_U8 << 20 | (uint32_t)OUT_F32 << 21 | (uint32_t)F16 << 22 |
           (uint32_t)VCAT << 23 | (uint32_t)T16 << 24 | (uint32_t)WRES << 25 | (uint32_t)NIT << 26;
}
constexpr uint32_t conv_pair_key(bool F16, int TAIL, int S, int NF) { return 1u << 31 | (uint32_t)F16 | (uint32_t)TAIL << 4 | (uint32_t)S << 12 | (uint32_t)NF << 16; }
inline uint32_t conv_variant_key(const ConvVariant &V) {
    if ((unsigned)V.KS > 15 || (unsigned)V.MF > 15 || (unsigned)V.NF > 15 || (unsigned)V.TAIL > 255 || (unsigned)V.S > 15) return 0;
    return V.pair ? conv_pair_key(V.F16, V.TAIL, V.S, V.NF) : conv_igemm_key(V.KS, V.MF, V.NF, V.IN_U8, V.OUT_F32, V.F16, V.TAIL, V.VCAT, V.T16, V.WRES, V.NIT);
}

// dynamic-LDS cap of the variant's row (above c16::kLdsDefault the launch raises the kernel's limit first), or 0: no such kernel
inline int conv_variant_lds_cap(const ConvVariant &V) {
    switch (conv_variant_key(V)) {
#define X(KS, MF, NF, IN_U8, OUT_F32, F16, TAIL, VCAT, T16, WRES, NIT) \
    case conv_igemm_key(KS, MF, NF, IN_U8, OUT_F32, F16, TAIL, VCAT, T16, WRES, NIT): return WRES ? c16::kLdsWres : c16::kLdsDefault;
        OBB_CONV_IGEMM_VARIANTS(X)
#undef X
#define X(F16, TAIL, S, NF) \
    case conv_pair_key(F16, TAIL, S, NF): return c16::kLdsPair;
        OBB_CONV_PAIR_VARIANTS(X)
#undef X
    }
    return 0;
}

}  // namespace obb
