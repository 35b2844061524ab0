// Holds the integer fp16 conversions of csrc/halfx.h (what a host compiler without _Float16 packs weights with: tests/host/convplan_main.cpp
// under g++) to the _Float16 conversions the library itself is built with.  Needs a compiler that has _Float16 (the ROCm clang).
//   clang++ -std=c++17 -O2 -D__HIP_PLATFORM_AMD__ -I<rocm>/include -I<repo>/oriented-object-detection_amd/csrc halfx_main.cpp
// float -> half: every float of magnitude 2^-26 .. 2^-12 (where the rounding position moves through the subnormals), and outside that every
// sign / exponent / upper 10 mantissa bits with the lower 13 at and around the rounding ties; half -> float: all 65536.  NaNs must
// stay NaNs (with the sign); their payloads are not compared.
#include "halfx.h"

#include <cstdio>
#include <cstring>

#ifndef __FLT16_MANT_DIG__
#error "this program compares against _Float16 and needs a compiler that has it"
#endif

using namespace obb;

static long n_bad = 0, n_checked = 0;

static void check_to(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    const half_bits_t a = host_to_f16_int(f), r = host_to_f16(f);
    ++n_checked;
    const bool nan = (u & 0x7fffffffu) > 0x7f800000u;
    const bool ok = nan ? ((a & 0x7fffu) > 0x7c00u && (r & 0x7fffu) > 0x7c00u && ((a ^ r) & 0x8000u) == 0) : a == r;
    if (!ok && n_bad++ < 8) fprintf(stderr, "float %08x -> half %04x, _Float16 gives %04x\n", u, a, r);
}

int main() {
    static const uint32_t lows[] = {0x0000, 0x0001, 0x0800, 0x0fff, 0x1000, 0x1001, 0x1800, 0x1ffe, 0x1fff};
    for (uint32_t sign = 0; sign < 2; ++sign) {
        for (uint32_t u = 0x32800000u; u < 0x39800000u; u += 1) check_to(sign << 31 | u);  // 2^-26 .. 2^-12, one by one
        for (uint32_t hi = 0; hi < (0x80000000u >> 13); ++hi)
            if (hi < (0x32800000u >> 13) || hi >= (0x39800000u >> 13))
                for (uint32_t lo : lows) check_to(sign << 31 | hi << 13 | lo);
    }
    for (uint32_t b = 0; b < 65536; ++b) {
        const float a = host_from_f16_int((half_bits_t)b), r = host_from_f16((half_bits_t)b);
        uint32_t ua, ur;
        memcpy(&ua, &a, 4);
        memcpy(&ur, &r, 4);
        ++n_checked;
        const bool nan = (b & 0x7fffu) > 0x7c00u;
        const bool ok = nan ? (a != a && r != r && ((ua ^ ur) & 0x80000000u) == 0) : ua == ur;
        if (!ok && n_bad++ < 16) fprintf(stderr, "half %04x -> float %08x, _Float16 gives %08x\n", b, ua, ur);
    }
    if (n_bad) { fprintf(stderr, "halfx: %ld of %ld conversions differ\n", n_bad, n_checked); return 1; }
    printf("halfx ok: %ld conversions\n", n_checked);
    return 0;
}
