// A tensor slice as every launch descriptor names it (16-bit and fp32 paths alike).  Plain C++: no device code, so that host-only
// translation units (f32plan.hip) can take launch descriptors without the 16-bit path's device helpers.
#pragma once
#include <cstdint>

namespace obb {

// Tensors are NHWC slices: element (b, y, x, c) of X lives at X.p + b*X.bs + (y*W + x)*X.cs + X.co + c.
// Channel-blocked variant (cpb > 0): the buffer is [C / blk][image][pixel][blk] with blk = 8 * cpb channels per block, so that a
// consumer which walks the channels in stages (or reads a channel slice) touches dense memory instead of 16..32-byte pieces of wide
// pixel rows: element (b, y, x, c) lives at X.p + (c / blk) * X.ps + b * X.bs + (y*W + x) * blk + c % blk   (co must be a multiple of blk).
struct TensorRef {
    void *p = nullptr;
    int64_t bs = 0;  // batch stride (elements)
    int cs = 0;      // pixel stride = channels of the underlying buffer (elements); blk for a blocked buffer
    int co = 0;      // channel offset of the slice
    int cpb = 0;     // 16-byte chunks (8 channels) per block; 0 = plain NHWC
    int64_t ps = 0;  // block stride (elements), blocked buffers only
};

}  // namespace obb
