// The numerical contracts the training kernels share (bntrain / convgrad / dwgrad / narrowgrad / routegrad / criterion .hip), each defined ONCE:
// the bf16 rounding rule, the order of the fp32 additions of the two reductions, and the work split that feeds them.  A training result is
// reproducible bit for bit because every kernel rounds and adds by these definitions; a new kernel of the family includes this file.
// Nothing here is for the inference path: halfx.h rounds with the hardware convert and its silu_f uses v_rcp_f32 / __expf -- other arithmetic,
// tested as such.  The names differ from halfx.h's (unpack8<F16>, pack8<F16>, silu_f), so both headers can be included together.
//
//   bf16       round to nearest even by bit arithmetic (host_to_bf16's), a NaN keeps its sign and top payload bits with the quiet bit set;
//              widening is exact.
//   reductions deterministic, no float atomics.  Pass 1: a workgroup is CW columns x RP pixel rows of lanes (row_split); the RP partial sums
//              of a column meet in LDS in a fixed pairwise tree, row r takes in row r + st, st = top / 2 .. 1, top = the power of two >= RP
//              (lds_row_tree); workgroup bx writes its result to row bx of an fp32 slab [nbx][n].  Pass 2: slab_combine adds the nbx rows of
//              element q: 64 strided walkers (walker w: rows w, w + 64, .. ascending, from 0.f), then walker w takes in walker w + st,
//              st = 32 .. 1.  slab_chain(nbx) is the longest fp32 addition chain of pass 2; the tests' error bounds are built from it.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

namespace obb {

// ---------------------------------------------------------------------------------------------- bf16
__device__ __forceinline__ float bf16_widen(unsigned short h) { return __uint_as_float((unsigned)h << 16); }
__device__ __forceinline__ float bf16_lo(unsigned u) { return __uint_as_float(u << 16); }          // the two values of a dword
__device__ __forceinline__ float bf16_hi(unsigned u) { return __uint_as_float(u & 0xffff0000u); }
__device__ __forceinline__ unsigned short bf16_rne(float f) {
    unsigned u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40);
    return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
__device__ __forceinline__ float bf16_round(float f) { return bf16_widen(bf16_rne(f)); }  // the nearest bf16 value, as fp32
__device__ __forceinline__ unsigned bf16_pack2(float a, float b) { return (unsigned)bf16_rne(a) | ((unsigned)bf16_rne(b) << 16); }

__device__ __forceinline__ void unpack8_bf16(const uint4 v, float f[8]) {
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) { f[2 * j] = bf16_lo(w[j]); f[2 * j + 1] = bf16_hi(w[j]); }
}
__device__ __forceinline__ uint4 pack8_bf16(const float f[8]) {
    return make_uint4(bf16_pack2(f[0], f[1]), bf16_pack2(f[2], f[3]), bf16_pack2(f[4], f[5]), bf16_pack2(f[6], f[7]));
}
__device__ __forceinline__ uint4 pack8_bf16_exact(const float f[8]) {  // f holds bf16 values: the high halves are the bits
    unsigned w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) w[j] = (__float_as_uint(f[2 * j]) >> 16) | (__float_as_uint(f[2 * j + 1]) & 0xffff0000u);
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// SiLU and its derivative with the library exp and a true division (halfx.h's silu_f is the inference form)
__device__ __forceinline__ float silu_exact(float y) { return y / (1.0f + expf(-y)); }
__device__ __forceinline__ float silu_grad_exact(float y) {  // s (1 + y (1 - s)), s = sigmoid(y): what autograd computes for y * sigmoid(y)
    const float sg = 1.0f / (1.0f + expf(-y));
    return sg * (1.0f + y * (1.0f - sg));
}

// ---------------------------------------------------------------------------------------------- pass 1: the work split and the LDS row tree
constexpr int kGroupChunks = 32;  // 16-byte channel chunks per workgroup column group (256 channels)

inline int tree_depth(int rows) {  // ceil(log2 rows): the additions a value passes in lds_row_tree
    int d = 0;
    while ((1 << d) < rows) ++d;
    return d;
}

// C channels as 8-channel chunks over 256 lanes: CW chunk columns x RP pixel rows per workgroup, ny column groups
struct RowSplit { int C8, CW, RP, ny, depth; };
inline RowSplit row_split(int C) {
    RowSplit g;
    g.C8 = C / 8;
    g.CW = std::min(g.C8, kGroupChunks);
    g.RP = 256 / g.CW;
    g.ny = (g.C8 + kGroupChunks - 1) / kGroupChunks;
    g.depth = tree_depth(g.RP);
    return g;
}

// `red` holds NP planes (PS floats apart) of [row][col][V] floats, 16-byte aligned; afterwards row 0 of every plane holds the sums over the RP
// rows, added pairwise: row r takes in row r + st, st = top / 2 .. 1 (RP need not be a power of two).  One barrier per step for all the planes.
// Every thread of the workgroup calls (`on`: this lane owns a column); the caller's stores to `red` need no barrier before, and the call ends
// with every thread past a barrier.
template <int V, int NP = 1>
__device__ __forceinline__ void lds_row_tree(float *red, int PS, int row, int col, int CW, int RP, bool on = true) {
    static_assert(V % 4 == 0, "a lane's V floats move as float4");
    for (int st = RP > 1 ? 1 << (31 - __clz(RP - 1)) : 0; st >= 1; st >>= 1) {  // from top / 2: the largest power of two below RP
        __syncthreads();
        if (on && row < st && row + st < RP) {
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                float4 *a = reinterpret_cast<float4 *>(red + p * PS + (row * CW + col) * V);
                const float4 *b = reinterpret_cast<const float4 *>(red + p * PS + ((row + st) * CW + col) * V);
#pragma unroll
                for (int v = 0; v < V / 4; ++v) {
                    const float4 x = a[v], y = b[v];
                    a[v] = make_float4(x.x + y.x, x.y + y.y, x.z + y.z, x.w + y.w);
                }
            }
        }
    }
    __syncthreads();
}

// ---------------------------------------------------------------------------------------------- pass 2: the slab combine
constexpr int kSlabWalkers = 64;                   // strided walkers per element
constexpr int kSlabWalkEl = 256 / kSlabWalkers;    // elements per 256-thread workgroup: grid = ceil(n / kSlabWalkEl)
constexpr int kSlabTreeDepth = 6;
static_assert(1 << kSlabTreeDepth == kSlabWalkers, "the walkers' tree");

// longest fp32 addition chain of slab_combine over nbx slabs: a walker's run, then the tree
inline int64_t slab_chain(int nbx) { return (nbx + kSlabWalkers - 1) / kSlabWalkers + kSlabTreeDepth; }

// the element of this thread: thread t is walker t / kSlabWalkEl of element blockIdx.x * kSlabWalkEl + t % kSlabWalkEl
__device__ __forceinline__ int slab_elem() { return blockIdx.x * kSlabWalkEl + threadIdx.x % kSlabWalkEl; }

// a[s] = sum over k < nbx of slab[s][k * n + q] for NS slabs of one shape, each in the order above; q = slab_elem().  Every thread of the
// 256-thread workgroup calls, once per kernel.  True on walker 0 of an element q < n: that thread holds the sums.
template <int NS>
__device__ __forceinline__ bool slab_combine(const float *const (&slab)[NS], int nbx, int n, int q, float (&a)[NS]) {
    __shared__ float sm[NS][kSlabWalkers][kSlabWalkEl];
    const int el = threadIdx.x % kSlabWalkEl, w = threadIdx.x / kSlabWalkEl;
#pragma unroll
    for (int s = 0; s < NS; ++s) a[s] = 0.f;
    if (q < n)
        for (int k = w; k < nbx; k += kSlabWalkers)
#pragma unroll
            for (int s = 0; s < NS; ++s) a[s] += slab[s][(size_t)k * n + q];
#pragma unroll
    for (int s = 0; s < NS; ++s) sm[s][w][el] = a[s];
    for (int st = kSlabWalkers / 2; st >= 1; st >>= 1) {
        __syncthreads();
        if (w < st)
#pragma unroll
            for (int s = 0; s < NS; ++s) { a[s] += sm[s][w + st][el]; sm[s][w][el] = a[s]; }
    }
    return w == 0 && q < n;
}

}  // namespace obb
