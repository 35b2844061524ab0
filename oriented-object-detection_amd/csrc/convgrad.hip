// Third slice of the training step (`model.train(...)`, Train_OBB.py:796-841: bf16 autocast, fp32 master
// weights): the backward of a stride-1 convolution (the 3x3 64 -> 64 and 1x1 shapes of YOLO11's C3k2 / head blocks), bf16 tensors in,
// fp32 accumulation.
//
//   dgrad  dX[b, y, x, ci] = sum_{ky, kx, co} dY[b, y + p - ky, x + p - kx, co] * W[co][ci][ky][kx]          (p = k / 2)
//          = the forward convolution of dY with the spatially flipped, channel-transposed weights: it runs on the forward's bf16
//          MFMA implicit-GEMM kernel (conv.hip, v_mfma_f32_16x16x32_bf16) with weights repacked per call; output rounded to bf16 once.
//   wgrad  dW[co][ci][ky][kx] = sum_{b, y, x} dY[b, y, x, co] * X[b, y + ky - p, x + kx - p, ci]
//          a GEMM whose reduction runs over PIXELS, which are the strided dimension of both NHWC operands.  First form (this file):
//          bf16 values widened to fp32 in registers (exact) and multiplied on the exact-f32 matrix instruction
//          v_mfma_f32_16x16x4_f32, whose operands are ONE k value per lane -- no transposition of the tiles is needed; fp32
//          accumulation in registers over all the tiles a persistent workgroup walks, one fp32 slab per workgroup, summed by a second
//          kernel in a fixed order (deterministic; no float atomics).  The 16x-faster bf16 form (v_mfma_f32_16x16x32_bf16 fed by
//          ds_read_b64_tr_b16 transposed LDS reads) is the next step: it needs the same tiles and the same walk.
//
// Stride 2 (3x3, pad 1, Hout = (H + 1) / 2: the downsampling convs of the backbone and the PAN, models 3 / 5 / 7 / 17 / 20 of yolo11s):
//   forward  the same conv kernel with stride 2, pair = false (obb_conv_fwd_s2_bf16 on obb_conv_s2_pack_bf16 weights).
//   dgrad    dX[m] = sum_k dY_up[m + 1 - k] W[k] with dY_up[2i] = dY[i] and zeros at odd positions: the stride-1 `same` forward of the
//            zero-inserted dY on the dgrad-form weights.  dY_up only needs the H x W extent (positions H and -1 are zeros / padding either
//            way), so the conv writes dX directly, no crop.  It spends 4x the useful MACs (three taps of four see an inserted zero).
//   wgrad    k_conv_wgrad<3, 2, ..>: R output rows stage 2R + 1 input rows of width 2 Wp + 1 (one 208-pixel row of model.3 at 416 px: R = 1).
//
// Channel counts: multiples of 8, at least 8, through ONE kernel (k_conv_wgrad) on blocks of ceil(live / 16) fragments per side -- the LDS tile
// at the live width, only the block's cout fragments issued, and the waves that have no cin fragment of their own taking every nshare-th k step
// of another wave's fragment.  The 64 x 64 blocks run the instance whose widths are compile-time constants.  obb_conv_wgrad_bf16 /
// obb_conv_wgrad_s2_bf16 (multiples of 64 only) and obb_conv_wgrad_c8_bf16 are checks in front of the same launcher: at multiples of 64 they
// give the same bits.  The split is described at the kernel.
#include <algorithm>
#include <vector>

#include "conv.h"
#include "ctx.h"
#include "launchcfg.h"
#include "traindev.h"

namespace obb {

typedef __attribute__((ext_vector_type(4))) float f32x4g;

// One workgroup = 4 waves = one (cout block, cin block) pair of dW for all KS*KS taps.  Channel blocks are ceil(c / 64) per side; the last block
// of a side holds c % 64 live channels (8 .. 56).  A tile of the input = R rows x W pixels of one image: dY rows padded with zeros to a multiple
// of 4 pixels (the k step), X rows with the zero halo of the convolution's padding.  S = 2: X is H x W, dY is Ho x Wo; R dY rows need
// (R - 1) S + KS X rows of (Wp - 1) S + KS pixels.  The launcher issues one launch per CLASS of blocks -- (full | partial cout block) x
// (full | partial cin block), at most four -- so that within a launch every workgroup has the same shape:
//   NCF   cout fragments of the block = ceil(live cout / 16): acc[NCF][TAPS] tiles of 16 x 16; a 16 -> 8 layer issues 1 x TAPS MFMAs per k step
//   CIF   4: the (full cout block) x (full cin block) class -- 64 live channels per side, so the pixel strides, the staging index arithmetic and
//         the wave split are compile-time constants and no liveness test is left; 0: cin fragments = the argument ncif = ceil(live cin / 16)
// LDS tile at the LIVE width: X pixels are ncif * 16 channels apart, dY pixels NCF * 16, staged in 16-byte chunks; a chunk whose first channel
// is >= the live count (the upper half of a fragment with 8 live channels) is zero-filled and never read from memory.
// Wave split: a wave owns ONE cin fragment and all NCF cout fragments.  With ncif < 4 the other waves take a share of the reduction of the same
// fragment: nshare = 4 / ncif (4, 2, 1, 1) waves per fragment, wave w -> fragment w % ncif, share w / ncif; the k steps of a tile (4 pixels of
// a row each) are numbered row-major and share s takes steps s, s + nshare, ...  (ncif = 3 leaves wave 3 without work: 3 does not divide 4.)
// After the walk the shares' accumulators are added into share 0's in share order 1, 2, 3, tap by tap through LDS (the tile is dead by then),
// and share 0 writes the workgroup's slab.  Slab of a walker = fp32 [tap][cout][cin], exactly dW's elements: nothing outside is written.
template <int KS, int S, int NCF, int CIF>
__global__ __launch_bounds__(256) void k_conv_wgrad(const unsigned short *__restrict__ x, const unsigned short *__restrict__ dy, int B, int H, int W, int Ho, int Wo,
                                                   int cin, int cout, int R, int cob0, int cib0, int ncif_arg, float *__restrict__ slabs) {
    static_assert(CIF == 0 || (CIF == 4 && NCF == 4), "CIF = 4 is the full x full class; every other class reads ncif from the argument");
    extern __shared__ __attribute__((aligned(16))) unsigned short swg[];
    constexpr int TAPS = KS * KS, PAD = KS / 2, COW = NCF * 16, ych = COW >> 3;
    constexpr bool FULL = CIF == 4;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, r16 = lane & 15;
    const int cob = cob0 + blockIdx.y, cib = cib0 + blockIdx.z;
    const int ncif = FULL ? 4 : ncif_arg;
    const int co_live = FULL ? 64 : min(64, cout - cob * 64), ci_live = FULL ? 64 : min(64, cin - cib * 64);  // multiples of 8; ceil(live / 16) == NCF, ncif
    const int CIW = ncif * 16, xch = CIW >> 3;  // channels per staged pixel; 16-byte chunks per pixel
    const int nshare = 4 / ncif, frag = FULL ? wave : wave % ncif, share = FULL ? 0 : wave / ncif;
    const bool active = share < nshare;
    const int Wp = (Wo + 3) & ~3, Wx = (Wp - 1) * S + KS, Rx = (R - 1) * S + KS;  // padded widths of the dY / X tiles, X rows
    unsigned short *sx = swg, *sdy = swg + (size_t)Rx * Wx * CIW;
    const int tiles_y = (Ho + R - 1) / R, ntiles = B * tiles_y;
    const int spr = Wp >> 2;  // k steps per row
    f32x4g acc[NCF][TAPS];
#pragma unroll
    for (int c = 0; c < NCF; ++c)
#pragma unroll
        for (int t = 0; t < TAPS; ++t) acc[c][t] = f32x4g{0.f, 0.f, 0.f, 0.f};
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int b = tile / tiles_y, y0 = (tile % tiles_y) * R;
        __syncthreads();
        // stage X rows y0 S - PAD .. (y0 + R - 1) S + PAD, pixels -PAD .. (Wp - 1) S + PAD of block cib (16-byte chunks, zeros outside)
        for (int i = tid; i < Rx * Wx * xch; i += 256) {
            const int c8 = i % xch, px = (i / xch) % Wx, ry = (i / xch) / Wx;
            const int yy = y0 * S + ry - PAD, xx = px - PAD;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (c8 * 8 < ci_live && yy >= 0 && yy < H && xx >= 0 && xx < W)
                v = *reinterpret_cast<const uint4 *>(x + (((int64_t)b * H + yy) * W + xx) * cin + cib * 64 + c8 * 8);
            *reinterpret_cast<uint4 *>(sx + ((size_t)ry * Wx + px) * CIW + c8 * 8) = v;
        }
        for (int i = tid; i < R * Wp * ych; i += 256) {
            const int c8 = i % ych, px = (i / ych) % Wp, ry = (i / ych) / Wp;
            const int yy = y0 + ry;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (c8 * 8 < co_live && yy < Ho && px < Wo) v = *reinterpret_cast<const uint4 *>(dy + (((int64_t)b * Ho + yy) * Wo + px) * cout + cob * 64 + c8 * 8);
            *reinterpret_cast<uint4 *>(sdy + ((size_t)ry * Wp + px) * COW + c8 * 8) = v;
        }
        __syncthreads();
        // One k step = 4 consecutive pixels of row ry, from pixel 4 xs: lane group g takes one.  The step body stands twice, once per walk: as a
        // lambda shared by both, four narrow shapes measured 2 - 3 % slower than the former kernel (profiles/wgrad_unified.md).
        if constexpr (FULL) {  // every step of the tile, row by row: no division in the walk
            for (int ry = 0; ry < R; ++ry)
                for (int xs = 0; xs < spr; ++xs) {
                    const int xg = xs * 4 + g;
                    float a[NCF];
#pragma unroll
                    for (int c = 0; c < NCF; ++c) a[c] = bf16_widen(sdy[((size_t)ry * Wp + xg) * COW + c * 16 + r16]);
#pragma unroll
                    for (int t = 0; t < TAPS; ++t) {
                        const int ky = t / KS, kx = t % KS;
                        const float bv = bf16_widen(sx[((size_t)(ry * S + ky) * Wx + xg * S + kx) * CIW + frag * 16 + r16]);
#pragma unroll
                        for (int c = 0; c < NCF; ++c) acc[c][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[c], bv, acc[c][t], 0, 0, 0);
                    }
                }
        } else if (active) {  // the steps of a tile are numbered row-major; this wave takes steps share, share + nshare, ...
            const int nsteps = R * spr;
            for (int q = share; q < nsteps; q += nshare) {
                const int ry = q / spr, xs = q % spr;
                const int xg = xs * 4 + g;
                float a[NCF];
#pragma unroll
                for (int c = 0; c < NCF; ++c) a[c] = bf16_widen(sdy[((size_t)ry * Wp + xg) * COW + c * 16 + r16]);
#pragma unroll
                for (int t = 0; t < TAPS; ++t) {
                    const int ky = t / KS, kx = t % KS;
                    const float bv = bf16_widen(sx[((size_t)(ry * S + ky) * Wx + xg * S + kx) * CIW + frag * 16 + r16]);
#pragma unroll
                    for (int c = 0; c < NCF; ++c) acc[c][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[c], bv, acc[c][t], 0, 0, 0);
                }
            }
        }
    }
    if (nshare > 1) {  // (workgroup-uniform) shares 1 .. nshare - 1 -> share 0, in share order; red[share - 1][frag][c][q][lane]
        float *red = reinterpret_cast<float *>(swg);
#pragma unroll
        for (int t = 0; t < TAPS; ++t) {
            __syncthreads();  // (t = 0: every wave is done with the tile; t > 0: share 0 has read tap t - 1)
            if (active && share > 0)
#pragma unroll
                for (int c = 0; c < NCF; ++c)
#pragma unroll
                    for (int q = 0; q < 4; ++q) red[((((share - 1) * ncif + frag) * NCF + c) * 4 + q) * 64 + lane] = acc[c][t][q];
            __syncthreads();
            if (share == 0)
                for (int s = 1; s < nshare; ++s)
#pragma unroll
                    for (int c = 0; c < NCF; ++c)
#pragma unroll
                        for (int q = 0; q < 4; ++q) acc[c][t][q] += red[((((s - 1) * ncif + frag) * NCF + c) * 4 + q) * 64 + lane];
        }
    }
    if (!active || share != 0) return;
    // D layout: lane holds ci = frag * 16 + r16 (column), couts c * 16 + 4 g .. + 3 (rows) of each tile; only dW's own elements are stored.
    // Address = a workgroup-uniform row pointer + one per-lane byte offset that is the same for every store.
    const int ci_l = frag * 16 + r16;
    if (ci_l >= ci_live) return;
    const size_t tap_stride = (size_t)cout * cin;
    const float *slab = slabs + (size_t)blockIdx.x * TAPS * tap_stride + (size_t)cob * 64 * cin + cib * 64;
    const unsigned lane_bytes = ((unsigned)(4 * g) * cin + ci_l) * 4u;
#pragma unroll
    for (int t = 0; t < TAPS; ++t, slab += tap_stride)
#pragma unroll
        for (int c = 0; c < NCF; ++c)
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (c * 16 + 4 * g + q < co_live)
                    *reinterpret_cast<float *>((char *)(slab + (unsigned)(c * 16 + q) * (unsigned)cin) + lane_bytes) = acc[c][t][q];
}

// dW[co][ci][tap] (OIHW, fp32) = sum over the walkers' [tap][cout][cin] slabs, in walker order
__global__ __launch_bounds__(256) void k_wgrad_reduce(const float *__restrict__ slabs, int nwalk, int taps, int cin, int cout, float *__restrict__ dw) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t per = (int64_t)taps * cout * cin;
    if (i >= per) return;
    float s = 0.f;
    for (int w = 0; w < nwalk; ++w) s += slabs[(size_t)w * per + i];
    const int ci = (int)(i % cin), co = (int)((i / cin) % cout), t = (int)(i / ((int64_t)cin * cout));
    dw[((size_t)co * cin + ci) * taps + t] = s;
}

// ---- assembled-chain pieces (round 4): device-side weight packing (no per-call host repack / synchronisation), the training forward that keeps
//      the pre-activation, SiLU forward / backward, bias gradient (bf16 rounding and the exact SiLU: traindev.h)

// fp32 OIHW master weights (device) -> the forward kernel's bf16 A-operand fragment order [cout block][stage][k step][fragment][lane][8]
// (pack_conv_weights' index arithmetic, element for element).  tflip = 1: the dgrad form -- the logical conv has the channel roles swapped and
// the taps flipped: W'[ci][co][t] = W[co][ci][taps - 1 - t].  pack_conv_elem = element o of one layer's blob: what k_pack_conv_bf16 and
// k_pack_conv_multi_bf16 both store.
__device__ __forceinline__ unsigned short pack_conv_elem(const float *__restrict__ w, int coutL, int cinL, int ks, int CK, int NF, int tflip, int64_t o) {
    const int cpk = CK / 8, taps = ks * ks, kst = ((ks == 3 ? 9 : 1) * cpk + 3) / 4, nstage = (cinL + CK - 1) / CK;
    const int j = (int)(o & 7), lane = (int)((o >> 3) & 63);
    int64_t rest = o >> 9;
    const int f = (int)(rest % NF); rest /= NF;
    const int k = (int)(rest % kst); rest /= kst;
    const int st = (int)(rest % nstage);
    const int cb = (int)(rest / nstage);
    const int r = lane & 15, gq = lane >> 4;
    const int co = cb * 16 * NF + (r >> 2) * 4 * NF + f * 4 + (r & 3);
    const int q = k * 4 + gq;
    const int tap = ks == 3 ? q / cpk : 0, c0 = ks == 3 ? (q % cpk) * 8 : q * 8;
    const int c = st * CK + c0 + j;
    float v = 0.f;
    if (co < coutL && c < cinL && tap < taps && (ks == 3 || c0 < CK))
        v = tflip ? w[((size_t)c * coutL + co) * taps + (taps - 1 - tap)] : w[((size_t)co * cinL + c) * taps + tap];
    return bf16_rne(v);
}

__global__ __launch_bounds__(256) void k_pack_conv_bf16(const float *__restrict__ w, int coutL, int cinL, int ks, int CK, int NF, int tflip, unsigned short *__restrict__ out,
                                                       int64_t total) {
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= total) return;
    out[o] = pack_conv_elem(w, coutL, cinL, ks, CK, NF, tflip, o);
}

// Every dense conv of a network, both forms, in ONE launch: the weights are windows of one flat fp32 buffer (train.ParamGroups' group 0) and the
// packed blobs segments of one bf16 buffer, described by a device-resident table of int64 words (built once per (layer list, input size) by
// obb_conv_pack_plan):
//     head   [0] kPackMagic  [1] records  [2] elements of the packed buffer  [3] elements of the flat buffer the records read up to
//     record [0] source offset  [1] destination offset  [2] elements  [3] first workgroup  [4] coutL | cinL << 32  [5] ks | tflip << 32
//            [6] CK | NF << 32  [7] 0
// A segment starts at a multiple of 256 elements and owns ceil(elements / 256) workgroups, so a workgroup lies in one segment: it finds its
// record by bisection over the records' first workgroups (uniform loads), then every lane stores pack_conv_elem of its element.  The padding
// behind a segment is never written.  The head is compared with the launch's own arguments: a table of another plan, or a flat buffer too short
// for it, makes every workgroup return before its first store.
constexpr int64_t kPackMagic = 0x4f42425041434b31ll;  // "OBBPACK1"
constexpr int kPackHead = OBB_PACK_TABLE_HEAD, kPackRec = OBB_PACK_TABLE_REC;

__global__ __launch_bounds__(256) void k_pack_conv_multi_bf16(const float *__restrict__ w, int64_t w_elems, const int64_t *__restrict__ tab, int nrec,
                                                             unsigned short *__restrict__ out, int64_t total) {
    if (tab[0] != kPackMagic || tab[1] != nrec || tab[2] != total || tab[3] > w_elems) return;
    int lo = 0, hi = nrec - 1;
    while (lo < hi) {  // the last record whose first workgroup is <= blockIdx.x
        const int mid = (lo + hi + 1) >> 1;
        if (tab[kPackHead + (int64_t)mid * kPackRec + 3] <= (int64_t)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const int64_t *__restrict__ r = tab + kPackHead + (int64_t)lo * kPackRec;
    const int64_t src = r[0], dst = r[1], n = r[2];
    const int64_t o = ((int64_t)blockIdx.x - r[3]) * 256 + threadIdx.x;
    const int coutL = (int)(r[4] & 0xffffffff), cinL = (int)(r[4] >> 32), ks = (int)(r[5] & 0xffffffff), tflip = (int)(r[5] >> 32);
    const int CK = (int)(r[6] & 0xffffffff), NF = (int)(r[6] >> 32);
    if (o < 0 || o >= n || dst < 0 || dst + o >= total || src < 0 || src + (int64_t)coutL * cinL * ks * ks > w_elems) return;
    out[dst + o] = pack_conv_elem(w + src, coutL, cinL, ks, CK, NF, tflip, o);
}

__global__ __launch_bounds__(256) void k_silu_bf16(const unsigned short *__restrict__ z, unsigned short *__restrict__ a, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    a[i] = bf16_rne(silu_exact(bf16_widen(z[i])));
}

// dz = da * silu'(z), silu'(z) = s (1 + z (1 - s)), s = sigmoid(z): what autograd computes for x * sigmoid(x); bf16 in / out, fp32 inside
__global__ __launch_bounds__(256) void k_silu_bwd_bf16(const unsigned short *__restrict__ z, const unsigned short *__restrict__ da, unsigned short *__restrict__ dz, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    dz[i] = bf16_rne(bf16_widen(da[i]) * silu_grad_exact(bf16_widen(z[i])));
}

// db[c] = sum over the pixels of dy[pixel][c], deterministic in a fixed order (traindev.h's slab pattern): pass 1 = one workgroup per (pixel
// block of PB pixels, 64-channel column block), 4 thread rows each summing every 4th pixel of the block in fp32, the rows added in a fixed tree,
// one partial per (block, channel) into the slab [nbx][cout]; pass 2 = slab_combine.  Partial sums stay small (PB / 4 terms per thread), so no
// bf16 value is lost against a large running sum -- the old form (4 threads per channel walking all npix / 4 pixels serially) reached 6e-6 of
// sum |dy| at 64 x 104 x 104 pixels.

__global__ __launch_bounds__(256) void k_bias_grad_part(const unsigned short *__restrict__ dy, int64_t npix, int cout, int64_t PB, float *__restrict__ slab) {
    __shared__ float part[4][64];
    const int c = blockIdx.y * 64 + (threadIdx.x & 63), rowg = threadIdx.x >> 6;
    const int64_t p0 = (int64_t)blockIdx.x * PB, p1 = min(p0 + PB, npix);
    float s = 0.f;
    if (c < cout)
        for (int64_t p = p0 + rowg; p < p1; p += 4) s += bf16_widen(dy[p * cout + c]);
    part[rowg][threadIdx.x & 63] = s;
    __syncthreads();
    if (rowg == 0 && c < cout) slab[(size_t)blockIdx.x * cout + c] = (part[0][threadIdx.x] + part[1][threadIdx.x]) + (part[2][threadIdx.x] + part[3][threadIdx.x]);
}

__global__ __launch_bounds__(256) void k_bias_grad_final(const float *__restrict__ slab, int nbx, int cout, float *__restrict__ db) {
    const int c = slab_elem();
    float a[1];
    if (slab_combine<1>({slab}, nbx, cout, c, a)) db[c] = a[0];
}

// dY bf16 [B][Ho][Wo][C] -> dY_up [B][H][W][C]: dY[i][j] at (2i, 2j), zeros elsewhere; one 16-byte chunk per thread and step
__global__ __launch_bounds__(256) void k_zero_insert_s2(const unsigned short *__restrict__ dy, int H, int W, int Ho, int Wo, int C8, int64_t nchunk,
                                                        unsigned short *__restrict__ up) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nchunk; i += (int64_t)gridDim.x * 256) {
        const int c8 = (int)(i % C8);
        const int64_t pix = i / C8;
        const int xx = (int)(pix % W), yy = (int)((pix / W) % H);
        const int64_t b = pix / ((int64_t)W * H);
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (((xx | yy) & 1) == 0) v = reinterpret_cast<const uint4 *>(dy)[((b * Ho + yy / 2) * Wo + xx / 2) * C8 + c8];
        reinterpret_cast<uint4 *>(up)[i] = v;
    }
}

namespace {

// the layer shapes of the training entry points: (stride 1) H x W -> H x W, (stride 2, 3x3) H x W -> (H + 1) / 2 x (W + 1) / 2
int out_dim(int n, int stride) { return stride == 2 ? (n + 1) / 2 : n; }

// ---- k_conv_wgrad's launch plan
using WgradFn = void (*)(const unsigned short *, const unsigned short *, int, int, int, int, int, int, int, int, int, int, int, float *);

template <int KS, int S>
WgradFn wgrad_kernel(int ncof, bool full) {
    if (full) return k_conv_wgrad<KS, S, 4, 4>;
    switch (ncof) {
        case 1: return k_conv_wgrad<KS, S, 1, 0>;
        case 2: return k_conv_wgrad<KS, S, 2, 0>;
        case 3: return k_conv_wgrad<KS, S, 3, 0>;
        default: return k_conv_wgrad<KS, S, 4, 0>;
    }
}

constexpr size_t kWgradLdsDefault = 64 * 1024, kWgradLdsMax = 160 * 1024;  // without / with allow_dyn_lds (the CU's whole LDS)

// LDS of one workgroup whose block has ncif cin and ncof cout fragments: the tile at the live width, or the cross-wave reduction's 4 ncof
// floats per lane of every wave with a share > 0, whichever is larger
size_t wgrad_lds(int R, int ks, int stride, int Wp, int Wx, int ncif, int ncof) {
    const size_t tile = ((size_t)((R - 1) * stride + ks) * Wx * ncif + (size_t)R * Wp * ncof) * 32;
    const int nshare = 4 / ncif;
    return std::max(tile, (size_t)(nshare - 1) * ncif * ncof * 1024);
}

// Blocks of 64 channels per side, the last one partial; one launch per class of blocks (see k_conv_wgrad).  R rows per tile: as many as the
// default 64 KiB hold at the widest class; a single row beyond that raises the kernel's cap (allow_dyn_lds) up to the CU's 160 KiB; a row
// that does not fit then is refused.  Walkers: at most 512 / (blocks of dW) per block; slabs in WS_TRAIN_C.
int wgrad_launch(obb_ctx *ctx, const char *fn, const uint16_t *x, const uint16_t *dy, int B, int H, int W, int cin, int cout, int ks, int stride, float *dw,
                 hipStream_t st) {
    const int taps = ks * ks, Ho = out_dim(H, stride), Wo = out_dim(W, stride);
    const int Wp = (Wo + 3) & ~3, Wx = (Wp - 1) * stride + ks;
    const int ncob = (cout + 63) / 64, ncib = (cin + 63) / 64;
    const int fco = cout / 64, fci = cin / 64;                             // full blocks per side
    const int pcof = (cout % 64 + 15) / 16, pcif = (cin % 64 + 15) / 16;  // fragments of the partial block (0: none)
    const int wcof = fco ? 4 : pcof, wcif = fci ? 4 : pcif;               // the widest class
    int R = 1;
    while (R < Ho && wgrad_lds(R + 1, ks, stride, Wp, Wx, wcif, wcof) <= kWgradLdsDefault) ++R;
    OBB_REQUIRE(ctx, wgrad_lds(R, ks, stride, Wp, Wx, wcif, wcof) <= kWgradLdsMax,
                "%s: a row of %d pixels at %d x %d channels per block does not fit the LDS tile (%zu bytes of %zu)", fn, W, wcif * 16, wcof * 16,
                wgrad_lds(R, ks, stride, Wp, Wx, wcif, wcof), kWgradLdsMax);
    const int ntiles = B * ((Ho + R - 1) / R);
    const int nwalk = std::max(1, std::min(ntiles, 512 / (ncob * ncib)));
    const size_t per = (size_t)taps * cout * cin;
    float *slabs = (float *)ctx->workspace(WS_TRAIN_C, (size_t)nwalk * per * 4);
    if (!slabs) return set_error(ctx, OBB_ERR_HIP, "%s: workspace allocation failed", fn);
    // classes: {first block, block count, fragments} per side; class 0 of a side = its full blocks
    const int co_cls[2][3] = {{0, fco, 4}, {fco, pcof ? 1 : 0, pcof}}, ci_cls[2][3] = {{0, fci, 4}, {fci, pcif ? 1 : 0, pcif}};
    for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 2; ++b) {
            const int *co = co_cls[a], *ci = ci_cls[b];
            if (!co[1] || !ci[1]) continue;
            const bool full = a == 0 && b == 0;
            const WgradFn k = stride == 2 ? wgrad_kernel<3, 2>(co[2], full) : ks == 3 ? wgrad_kernel<3, 1>(co[2], full) : wgrad_kernel<1, 1>(co[2], full);
            const size_t lds = wgrad_lds(R, ks, stride, Wp, Wx, ci[2], co[2]);
            if (lds > kWgradLdsDefault) {
                hipError_t e = allow_dyn_lds(reinterpret_cast<const void *>(k), kWgradLdsMax);
                if (e != hipSuccess) return set_error(ctx, OBB_ERR_HIP, "%s: raising the LDS cap failed: %s", fn, hipGetErrorString(e));
            }
            hipLaunchKernelGGL(k, dim3((unsigned)nwalk, (unsigned)co[1], (unsigned)ci[1]), dim3(256), lds, st, x, dy, B, H, W, Ho, Wo, cin, cout, R, co[0], ci[0], ci[2],
                               slabs);
        }
    hipLaunchKernelGGL(k_wgrad_reduce, dim3((unsigned)cdiv((int64_t)per, 256)), dim3(256), 0, st, slabs, nwalk, taps, cin, cout, dw);
    OBB_LAUNCH_CHECK(ctx);
    return OBB_OK;
}

// packed size / device packing of the forward-kernel weights of a layer whose INPUT is H x W
int packed_elems(obb_ctx *ctx, const char *fn, int cout, int cin, int ks, int stride, int H, int W, int dgrad_form, int64_t *n_elems) {
    OBB_REQUIRE(ctx, ctx && n_elems && cout > 0 && cin > 0 && (ks == 1 || ks == 3) && H > 0 && W > 0, "%s: bad arguments", fn);
    const int coutL = dgrad_form ? cin : cout, cinL = dgrad_form ? cout : cin;
    const ConvTiling t = plan_conv(ks, stride, cinL, coutL, out_dim(H, stride), out_dim(W, stride), false);
    *n_elems = conv_packed_elems(coutL, cinL, ks, t, 0);
    return OBB_OK;
}

int pack_launch(obb_ctx *ctx, const char *fn, const float *w_oihw, int cout, int cin, int ks, int stride, int H, int W, int dgrad_form, uint16_t *packed, hipStream_t st) {
    OBB_REQUIRE(ctx, ctx && w_oihw && packed, "%s: NULL buffer", fn);
    int64_t n = 0;
    int rc = packed_elems(ctx, fn, cout, cin, ks, stride, H, W, dgrad_form, &n);
    if (rc) return rc;
    const int coutL = dgrad_form ? cin : cout, cinL = dgrad_form ? cout : cin;
    const ConvTiling t = plan_conv(ks, stride, cinL, coutL, out_dim(H, stride), out_dim(W, stride), false);
    hipLaunchKernelGGL(k_pack_conv_bf16, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, st, w_oihw, coutL, cinL, ks, t.CK, t.NF, dgrad_form ? 1 : 0, packed, n);
    OBB_LAUNCH_CHECK(ctx);
    return OBB_OK;
}

// y = conv(x) + bias, no activation, input H x W, output out_dim(H, stride) x out_dim(W, stride)
int fwd_launch(obb_ctx *ctx, const char *fn, const uint16_t *x, const uint16_t *packed_w, const float *bias, int B, int H, int W, int cin, int cout, int ks, int stride,
               uint16_t *y, hipStream_t st) {
    const int Ho = out_dim(H, stride), Wo = out_dim(W, stride);
    const ConvTiling t = plan_conv(ks, stride, cin, cout, Ho, Wo, false);
    // [bias padded to the kernel's 64-float granule (zeros without one)][2 KiB: the `lut` argument = the sink of the kernel's unconditional stores]
    const size_t bbytes = (((size_t)cout + 63) / 64 * 64 * 4 + 256 + 255) & ~(size_t)255;
    char *ws = (char *)ctx->workspace(WS_TRAIN_A, bbytes + 2048);
    if (!ws) return set_error(ctx, OBB_ERR_HIP, "%s: workspace allocation failed", fn);
    OBB_HIP(ctx, hipMemsetAsync(ws, 0, bbytes, st));
    if (bias) OBB_HIP(ctx, hipMemcpyAsync(ws, bias, (size_t)cout * 4, hipMemcpyDeviceToDevice, st));
    ConvLaunch L;
    L.in.p = (void *)x; L.in.bs = (int64_t)H * W * cin; L.in.cs = cin; L.in.co = 0;
    L.out.p = (void *)y; L.out.bs = (int64_t)Ho * Wo * cout; L.out.cs = cout; L.out.co = 0;
    L.wpk = (const bf16_t *)packed_w; L.bias = (const float *)ws; L.lut = (const bf16_t *)(ws + bbytes);
    L.B = B; L.Hin = H; L.Hout = Ho; L.Win = W; L.Wout = Wo; L.cin = cin; L.cout = cout; L.ks = ks; L.stride = stride; L.act = 0; L.f16 = 0;
    L.TH = t.TH; L.TW = t.TW; L.MF = t.MF; L.NF = t.NF; L.CK = t.CK;
    L.tiles_y = (Ho + t.TH - 1) / t.TH; L.tiles_x = (Wo + t.TW - 1) / t.TW;
    if (ks == 1) {
        const int64_t npx = (int64_t)B * H * W;
        OBB_REQUIRE(ctx, npx < (1ll << 31) / 4, "%s: too many pixels for one launch", fn);
        L.B = 1; L.Hin = L.Hout = 1; L.Win = L.Wout = (int)npx;
        L.tiles_y = 1; L.tiles_x = (int)((npx + L.TW - 1) / L.TW);
    }
    hipError_t e = launch_conv(L, st);
    if (e != hipSuccess) return set_error(ctx, OBB_ERR_HIP, "%s: launch failed: %s", fn, hipGetErrorString(e));
    return OBB_OK;
}

}  // namespace
}  // namespace obb

using namespace obb;

extern "C" {

int obb_conv_dgrad_bf16(obb_ctx *ctx, const uint16_t *dy, const float *w_oihw_host, int32_t B, int32_t H, int32_t W, int32_t cin, int32_t cout, int32_t ks,
                        uint16_t *dx, obb_stream_t s) {
    OBB_REQUIRE(ctx, ctx && B >= 0 && H > 0 && W > 0 && (ks == 1 || ks == 3), "obb_conv_dgrad_bf16: bad arguments");
    OBB_REQUIRE(ctx, cin % 8 == 0 && cout % 8 == 0 && cin >= 8 && cout >= 8, "obb_conv_dgrad_bf16: channel counts must be multiples of 8");
    if (B == 0) return OBB_OK;
    OBB_REQUIRE(ctx, dy && w_oihw_host && dx, "obb_conv_dgrad_bf16: NULL buffer");
    hipStream_t st = (hipStream_t)s;
    const int taps = ks * ks;
    // W'[ci][co][ky][kx] = W[co][ci][k - 1 - ky][k - 1 - kx]: the forward conv of dY with W' is dX
    std::vector<float> wt((size_t)cin * cout * taps);
    for (int co = 0; co < cout; ++co)
        for (int ci = 0; ci < cin; ++ci)
            for (int t = 0; t < taps; ++t) wt[((size_t)ci * cout + co) * taps + (taps - 1 - t)] = w_oihw_host[((size_t)co * cin + ci) * taps + t];
    const ConvTiling t = plan_conv(ks, 1, cout, cin, H, W, false);
    const std::vector<bf16_t> pk = pack_conv_weights(wt.data(), cin, cout, ks, t, nullptr, 0, false);
    const size_t wbytes = pk.size() * sizeof(bf16_t);
    bf16_t *wpk = (bf16_t *)ctx->workspace(WS_TRAIN_B, wbytes);
    if (!wpk) return set_error(ctx, OBB_ERR_HIP, "obb_conv_dgrad_bf16: workspace allocation failed");
    OBB_HIP(ctx, hipMemcpyAsync(wpk, pk.data(), wbytes, hipMemcpyHostToDevice, st));
    OBB_HIP(ctx, hipStreamSynchronize(st));  // (the packed weights live in host memory that goes out of scope)
    return fwd_launch(ctx, "obb_conv_dgrad_bf16", dy, (const uint16_t *)wpk, nullptr, B, H, W, cout, cin, ks, 1, dx, st);
}

int obb_conv_wgrad_bf16(obb_ctx *ctx, const uint16_t *x, const uint16_t *dy, int32_t B, int32_t H, int32_t W, int32_t cin, int32_t cout, int32_t ks, float *dw,
                        obb_stream_t s) {
    OBB_REQUIRE(ctx, ctx && B >= 1 && H > 0 && W > 0 && (ks == 1 || ks == 3), "obb_conv_wgrad_bf16: bad arguments");
    OBB_REQUIRE(ctx, cin % 64 == 0 && cout % 64 == 0, "obb_conv_wgrad_bf16: channel counts must be multiples of 64 (one workgroup = a 64 x 64 block of dW)");
    OBB_REQUIRE(ctx, x && dy && dw, "obb_conv_wgrad_bf16: NULL buffer");
    OBB_REQUIRE(ctx, cin >= 64 && cout >= 64, "obb_conv_wgrad_bf16: cin = %d, cout = %d: at least 64 channels each", (int)cin, (int)cout);  // (0 % 64 == 0)
    return wgrad_launch(ctx, "obb_conv_wgrad_bf16", x, dy, B, H, W, cin, cout, ks, 1, dw, (hipStream_t)s);
}

int obb_conv_packed_elems(obb_ctx *ctx, int32_t cout, int32_t cin, int32_t ks, int32_t H, int32_t W, int32_t dgrad_form, int64_t *n_elems) {
    return packed_elems(ctx, "obb_conv_packed_elems", cout, cin, ks, 1, H, W, dgrad_form, n_elems);
}

int obb_conv_pack_bf16(obb_ctx *ctx, const float *w_oihw, int32_t cout, int32_t cin, int32_t ks, int32_t H, int32_t W, int32_t dgrad_form, uint16_t *packed,
                       obb_stream_t s) {
    return pack_launch(ctx, "obb_conv_pack_bf16", w_oihw, cout, cin, ks, 1, H, W, dgrad_form, packed, (hipStream_t)s);
}

int obb_conv_fwd_bf16(obb_ctx *ctx, const uint16_t *x, const uint16_t *packed_w, const float *bias, int32_t B, int32_t H, int32_t W, int32_t cin, int32_t cout,
                      int32_t ks, uint16_t *y, obb_stream_t s) {
    OBB_REQUIRE(ctx, ctx && B >= 0 && H > 0 && W > 0 && (ks == 1 || ks == 3), "obb_conv_fwd_bf16: bad arguments");
    OBB_REQUIRE(ctx, cin % 8 == 0 && cout % 8 == 0 && cin >= 8 && cout >= 8, "obb_conv_fwd_bf16: channel counts must be multiples of 8");
    if (B == 0) return OBB_OK;
    OBB_REQUIRE(ctx, x && packed_w && y, "obb_conv_fwd_bf16: NULL buffer");
    return fwd_launch(ctx, "obb_conv_fwd_bf16", x, packed_w, bias, B, H, W, cin, cout, ks, 1, y, (hipStream_t)s);
}

// ---- stride 2 (3x3, pad 1): H x W -> (H + 1) / 2 x (W + 1) / 2
int obb_conv_s2_packed_elems(obb_ctx *ctx, int32_t cout, int32_t cin, int32_t H, int32_t W, int64_t *n_elems) {
    return packed_elems(ctx, "obb_conv_s2_packed_elems", cout, cin, 3, 2, H, W, 0, n_elems);
}

int obb_conv_s2_pack_bf16(obb_ctx *ctx, const float *w_oihw, int32_t cout, int32_t cin, int32_t H, int32_t W, uint16_t *packed, obb_stream_t s) {
    return pack_launch(ctx, "obb_conv_s2_pack_bf16", w_oihw, cout, cin, 3, 2, H, W, 0, packed, (hipStream_t)s);
}

// ---- every dense conv in one launch (k_pack_conv_multi_bf16): the plan, once per (layer list, input size), and the per-step launch
int obb_conv_pack_plan(obb_ctx *ctx, int32_t nrec, const int32_t *cout, const int32_t *cin, const int32_t *ks, const int32_t *stride, const int32_t *H,
                       const int32_t *W, const int32_t *dgrad_form, const int64_t *src_off, int64_t src_elems, int64_t *dst_off, int64_t *n_elems,
                       int64_t *total, int64_t *table, int64_t table_words, obb_stream_t s) {
    const char *fn = "obb_conv_pack_plan";
    OBB_REQUIRE(ctx, ctx && nrec >= 1 && cout && cin && ks && stride && H && W && dgrad_form && src_off && dst_off && n_elems && total && src_elems > 0,
                "%s: bad arguments", fn);
    OBB_REQUIRE(ctx, !table || table_words == kPackHead + (int64_t)nrec * kPackRec, "%s: the table holds %lld words, %lld needed for %d records", fn,
                (long long)table_words, (long long)(kPackHead + (int64_t)nrec * kPackRec), (int)nrec);
    std::vector<int64_t> tab((size_t)(kPackHead + (int64_t)nrec * kPackRec), 0), dst((size_t)nrec), cnt((size_t)nrec);
    int64_t blk = 0, need = 0;
    for (int i = 0; i < nrec; ++i) {
        OBB_REQUIRE(ctx, (stride[i] == 1 && (ks[i] == 1 || ks[i] == 3)) || (stride[i] == 2 && ks[i] == 3), "%s: record %d: k = %d at stride %d", fn, i, (int)ks[i],
                    (int)stride[i]);
        // (the dgrad form is a stride-1 conv on the layer's H x W input, whatever the layer's stride: obb_conv_dgrad_s2_bf16)
        const int st = dgrad_form[i] ? 1 : stride[i];
        int64_t n = 0;
        if (int rc = packed_elems(ctx, fn, cout[i], cin[i], ks[i], st, H[i], W[i], dgrad_form[i], &n)) return rc;
        const int64_t wn = (int64_t)cout[i] * cin[i] * ks[i] * ks[i];
        OBB_REQUIRE(ctx, src_off[i] >= 0 && src_off[i] + wn <= src_elems, "%s: record %d reads [%lld, %lld) of a flat buffer of %lld elements", fn, i,
                    (long long)src_off[i], (long long)(src_off[i] + wn), (long long)src_elems);
        const int coutL = dgrad_form[i] ? cin[i] : cout[i], cinL = dgrad_form[i] ? cout[i] : cin[i];
        const ConvTiling t = plan_conv(ks[i], st, cinL, coutL, out_dim(H[i], st), out_dim(W[i], st), false);
        int64_t *r = tab.data() + kPackHead + (int64_t)i * kPackRec;
        r[0] = src_off[i]; r[1] = blk * 256; r[2] = n; r[3] = blk;
        r[4] = (int64_t)coutL | ((int64_t)cinL << 32); r[5] = (int64_t)ks[i] | ((int64_t)(dgrad_form[i] ? 1 : 0) << 32); r[6] = (int64_t)t.CK | ((int64_t)t.NF << 32);
        dst[(size_t)i] = r[1]; cnt[(size_t)i] = n;
        blk += cdiv(n, 256);
        need = std::max(need, src_off[i] + wn);
    }
    OBB_REQUIRE(ctx, blk < (1ll << 31), "%s: %lld workgroups: too many for one launch", fn, (long long)blk);
    tab[0] = kPackMagic; tab[1] = nrec; tab[2] = blk * 256; tab[3] = need;
    if (table) {
        hipStream_t st = (hipStream_t)s;
        OBB_HIP(ctx, hipMemcpyAsync(table, tab.data(), tab.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
        OBB_HIP(ctx, hipStreamSynchronize(st));  // (the host copy of the table goes out of scope)
    }
    std::copy(dst.begin(), dst.end(), dst_off);
    std::copy(cnt.begin(), cnt.end(), n_elems);
    *total = blk * 256;
    return OBB_OK;
}

int obb_conv_pack_multi_bf16(obb_ctx *ctx, const float *w_flat, int64_t w_elems, const int64_t *table, int64_t table_words, int32_t nrec, uint16_t *packed,
                             int64_t packed_elems_, obb_stream_t s) {
    const char *fn = "obb_conv_pack_multi_bf16";
    OBB_REQUIRE(ctx, ctx && w_flat && table && packed, "%s: NULL buffer", fn);
    OBB_REQUIRE(ctx, nrec >= 1 && w_elems > 0 && table_words == kPackHead + (int64_t)nrec * kPackRec, "%s: the table holds %lld words, %lld needed for %d records", fn,
                (long long)table_words, (long long)(kPackHead + (int64_t)nrec * kPackRec), (int)nrec);
    OBB_REQUIRE(ctx, packed_elems_ > 0 && packed_elems_ % 256 == 0 && packed_elems_ / 256 < (1ll << 31),
                "%s: the packed buffer holds %lld elements: a plan's total is a positive multiple of 256", fn, (long long)packed_elems_);
    hipLaunchKernelGGL(k_pack_conv_multi_bf16, dim3((unsigned)(packed_elems_ / 256)), dim3(256), 0, (hipStream_t)s, w_flat, w_elems, table, (int)nrec, packed,
                       packed_elems_);
    OBB_LAUNCH_CHECK(ctx);
    return OBB_OK;
}

int obb_conv_fwd_s2_bf16(obb_ctx *ctx, const uint16_t *x, const uint16_t *packed_w, const float *bias, int32_t B, int32_t H, int32_t W, int32_t cin, int32_t cout,
                         uint16_t *y, obb_stream_t s) {
    OBB_REQUIRE(ctx, ctx && B >= 0 && H > 0 && W > 0, "obb_conv_fwd_s2_bf16: bad arguments");
    OBB_REQUIRE(ctx, cin % 8 == 0 && cout % 8 == 0 && cin >= 8 && cout >= 8, "obb_conv_fwd_s2_bf16: channel counts must be multiples of 8");
    if (B == 0) return OBB_OK;
    OBB_REQUIRE(ctx, x && packed_w && y, "obb_conv_fwd_s2_bf16: NULL buffer");
    return fwd_launch(ctx, "obb_conv_fwd_s2_bf16", x, packed_w, bias, B, H, W, cin, cout, 3, 2, y, (hipStream_t)s);
}

int obb_conv_dgrad_s2_bf16(obb_ctx *ctx, const uint16_t *dy, const uint16_t *packed_dgrad, int32_t B, int32_t H, int32_t W, int32_t cin, int32_t cout, uint16_t *dx,
                           obb_stream_t s) {
    OBB_REQUIRE(ctx, ctx && B >= 0 && H > 0 && W > 0, "obb_conv_dgrad_s2_bf16: bad arguments");
    OBB_REQUIRE(ctx, cin % 8 == 0 && cout % 8 == 0 && cin >= 8 && cout >= 8, "obb_conv_dgrad_s2_bf16: channel counts must be multiples of 8");
    if (B == 0) return OBB_OK;
    OBB_REQUIRE(ctx, dy && packed_dgrad && dx, "obb_conv_dgrad_s2_bf16: NULL buffer");
    hipStream_t st = (hipStream_t)s;
    const int64_t nchunk = (int64_t)B * H * W * (cout / 8);
    uint16_t *up = (uint16_t *)ctx->workspace(WS_TRAIN_D, (size_t)nchunk * 16);
    if (!up) return set_error(ctx, OBB_ERR_HIP, "obb_conv_dgrad_s2_bf16: workspace allocation failed");
    hipLaunchKernelGGL(k_zero_insert_s2, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv(nchunk, 256), 2048))), dim3(256), 0, st, dy, (int)H, (int)W,
                       out_dim(H, 2), out_dim(W, 2), (int)(cout / 8), nchunk, up);
    OBB_LAUNCH_CHECK(ctx);
    return fwd_launch(ctx, "obb_conv_dgrad_s2_bf16", up, packed_dgrad, nullptr, B, H, W, cout, cin, 3, 1, dx, st);
}

int obb_conv_wgrad_s2_bf16(obb_ctx *ctx, const uint16_t *x, const uint16_t *dy, int32_t B, int32_t H, int32_t W, int32_t cin, int32_t cout, float *dw, obb_stream_t s) {
    OBB_REQUIRE(ctx, ctx && B >= 1 && H > 0 && W > 0, "obb_conv_wgrad_s2_bf16: bad arguments");
    OBB_REQUIRE(ctx, cin % 64 == 0 && cout % 64 == 0,
                "obb_conv_wgrad_s2_bf16: cin = %d, cout = %d: channel counts must be multiples of 64 (one workgroup = a 64 x 64 block of dW); "
                "models 0 and 1 of the backbone (3 -> 32, 32 -> 64) have no stride-2 wgrad", (int)cin, (int)cout);
    OBB_REQUIRE(ctx, x && dy && dw, "obb_conv_wgrad_s2_bf16: NULL buffer");
    OBB_REQUIRE(ctx, cin >= 64 && cout >= 64, "obb_conv_wgrad_s2_bf16: cin = %d, cout = %d: at least 64 channels each", (int)cin, (int)cout);  // (0 % 64 == 0)
    return wgrad_launch(ctx, "obb_conv_wgrad_s2_bf16", x, dy, B, H, W, cin, cout, 3, 2, dw, (hipStream_t)s);
}

int obb_conv_wgrad_c8_bf16(obb_ctx *ctx, const uint16_t *x, const uint16_t *dy, int32_t B, int32_t H, int32_t W, int32_t cin, int32_t cout, int32_t ks, int32_t stride,
                           float *dw, obb_stream_t s) {
    OBB_REQUIRE(ctx, ctx && B >= 1 && H > 0 && W > 0, "obb_conv_wgrad_c8_bf16: bad arguments (B = %d, H = %d, W = %d)", (int)B, (int)H, (int)W);
    OBB_REQUIRE(ctx, (stride == 1 && (ks == 1 || ks == 3)) || (stride == 2 && ks == 3),
                "obb_conv_wgrad_c8_bf16: k = %d at stride %d: 1x1 and 3x3 at stride 1 and 3x3 at stride 2 are built", (int)ks, (int)stride);
    OBB_REQUIRE(ctx, cin >= 8 && cout >= 8 && cin % 8 == 0 && cout % 8 == 0,
                "obb_conv_wgrad_c8_bf16: cin = %d, cout = %d: channel counts must be multiples of 8, at least 8 (16-byte staging chunks)", (int)cin, (int)cout);
    OBB_REQUIRE(ctx, x && dy && dw, "obb_conv_wgrad_c8_bf16: NULL buffer");
    return wgrad_launch(ctx, "obb_conv_wgrad_c8_bf16", x, dy, B, H, W, cin, cout, ks, stride, dw, (hipStream_t)s);
}

int obb_silu_bf16(obb_ctx *ctx, const uint16_t *z, uint16_t *a, int64_t n, obb_stream_t s) {
    OBB_REQUIRE(ctx, ctx && n >= 0, "obb_silu_bf16: bad arguments");
    if (n == 0) return OBB_OK;
    OBB_REQUIRE(ctx, z && a, "obb_silu_bf16: NULL buffer");
    hipLaunchKernelGGL(k_silu_bf16, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)s, z, a, n);
    OBB_LAUNCH_CHECK(ctx);
    return OBB_OK;
}

int obb_silu_bwd_bf16(obb_ctx *ctx, const uint16_t *z, const uint16_t *da, uint16_t *dz, int64_t n, obb_stream_t s) {
    OBB_REQUIRE(ctx, ctx && n >= 0, "obb_silu_bwd_bf16: bad arguments");
    if (n == 0) return OBB_OK;
    OBB_REQUIRE(ctx, z && da && dz, "obb_silu_bwd_bf16: NULL buffer");
    hipLaunchKernelGGL(k_silu_bwd_bf16, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)s, z, da, dz, n);
    OBB_LAUNCH_CHECK(ctx);
    return OBB_OK;
}

int obb_bias_grad_bf16(obb_ctx *ctx, const uint16_t *dy, int64_t npix, int32_t cout, float *db, obb_stream_t s) {
    OBB_REQUIRE(ctx, ctx && npix >= 1 && cout >= 1, "obb_bias_grad_bf16: bad arguments");
    OBB_REQUIRE(ctx, dy && db, "obb_bias_grad_bf16: NULL buffer");
    hipStream_t st = (hipStream_t)s;
    const int ncb = (cout + 63) / 64;
    const int64_t nbx0 = std::min<int64_t>(cdiv(npix, 4), std::max(1, 1024 / ncb));  // ~1024 workgroups: four per CU
    const int64_t PB = cdiv(npix, nbx0);
    const int nbx = (int)cdiv(npix, PB);
    float *slab = (float *)ctx->workspace(WS_TRAIN_F, (size_t)nbx * cout * 4);
    if (!slab) return set_error(ctx, OBB_ERR_HIP, "obb_bias_grad_bf16: workspace allocation failed");
    hipLaunchKernelGGL(k_bias_grad_part, dim3((unsigned)nbx, (unsigned)ncb), dim3(256), 0, st, dy, npix, (int)cout, PB, slab);
    hipLaunchKernelGGL(k_bias_grad_final, dim3((unsigned)cdiv(cout, kSlabWalkEl)), dim3(256), 0, st, slab, nbx, (int)cout, db);
    OBB_LAUNCH_CHECK(ctx);
    return OBB_OK;
}

}  // extern "C"
