/*
 * obbhip.h -- C-ABI of libobbhip.so: the MI355X (gfx950) drop-in for the Detect_OBB.py sliding-window
 * oriented-box inference path of Abolfazlmsl/Oriented-Object-Detection.
 *
 * The reference has no FFI: its seams are plain Python callables.  Each entry point below
 * names the reference interface it replaces (file:line in /root/reference).  Rules of the boundary:
 *   - plain pointers and sizes only; every DATA pointer is a DEVICE pointer unless the name ends in _host;
 *   - the caller allocates every buffer; the library owns only the context (weights, workspaces, hipGraphs);
 *   - every launch goes to the caller's stream (hipStream_t passed as void*); no hidden synchronisation except
 *     where a function is documented "(synchronises)";
 *   - int status return (0 = ok, <0 = error) + obb_last_error(); nothing throws across the boundary;
 *   - invalid / degenerate polygons yield IoU 0.0, not an error (Detect_OBB.py:150-151).
 *
 * Record layout shared by the detection-level calls ("det arrays"), all SoA:
 *   boxes  double[n*8]   x1,y1,...,x4,y4  global pixel coordinates   (Detect_OBB.py:256-260)
 *   cls    int32[n]                                                   (Detect_OBB.py:261)
 *   conf   double[n]     float32 confidences widened to double        (Detect_OBB.py:231)
 */
#ifndef OBBHIP_H
#define OBBHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OBB_OK 0
#define OBB_ERR_INVALID (-1) /* bad argument                          */
#define OBB_ERR_HIP (-2)     /* a HIP runtime call failed             */
#define OBB_ERR_STATE (-3)   /* e.g. forward before weights are loaded */
#define OBB_ERR_FORMAT (-4)  /* malformed weight blob                 */

typedef struct obb_ctx obb_ctx;
typedef void *obb_stream_t; /* hipStream_t */

int obb_version(void);
/* One context per device / rank.  (synchronises) */
int obb_ctx_create(int device, obb_ctx **out);
int obb_ctx_destroy(obb_ctx *ctx);
/* Last error text of this context (or of the calling thread when ctx == NULL). */
const char *obb_last_error(const obb_ctx *ctx);

/* Engine knobs (no reference counterpart).
 *   "precision"   16 = fp16 activation/weight storage (default; what Ultralytics' half=True inference uses), 1016 = bf16 storage; fp32
 *                 accumulation either way.  32 = fp32 arithmetic end to end (what the reference computes: Detect_OBB.py:79-83 calls the
 *                 model with half=False): fp32 weights and activations, convolutions on the exact-f32 matrix instruction (a k-ordered
 *                 fmaf chain), one kernel per layer, no fusion; error vs a double-precision evaluation of the same weights ~1e-5 on a
 *                 head logit, the same as torch's own fp32 forward (tests/test_gpu_fp32.py).  Applies to the next obb_model_load.
 *   "model_slot"  index (0..63) of the model that obb_model_load / obb_forward / obb_decode* address (several models may live in one
 *                 context, e.g. the 128 px and 416 px checkpoints of the dual-scale config).
 *   fused forms, 1 = on (default), 0 = the separate launches they replace; each applies to the next obb_model_load and exists so that
 *   parity tests can compare both forms on identical inputs:
 *     "tail"      last 1x1 conv of each head branch behind its producer; 0 also turns every other intermediate-swallowing fusion off
 *                 (bneck, hmerge, c3kimg, dwpw, tail16): every layer's output is then observable through obb_debug_activation
 *     "tail16"    cv1 of the C3k2 blocks 2 / 4 inside the preceding stride-2 conv      "bneck"     Bottleneck row stripes (104 / 52 levels)
 *     "bneck_cv2" closing 1x1 of those C3k2 blocks behind the Bottleneck               "c3kimg"    inner C3k of the stride-32 level per image
 *     "dwpw"      depthwise 3x3 -> 1x1 stripes of the class branch                     "upfold"    Upsample + Concat read in place by the 1x1
 *     "stem"      model.0 as row stripes on the uint8 tile                             "hmerge"    sibling convs on one input as one launch
 *     "sppf_fuse" the three SPPF pools in one launch                                   "attn_mfma" C2PSA attention on the matrix cores
 *     "front"     model.0 + model.1 + model.2.cv1 as one launch (tile sides % 52 == 0)  "pair"      64 -> 64-cout 3x3 convs on k_conv3_pair
 *     "nitile"    (16-bit modes) several whole images per tile on the 4 x 4 / 2 x 2 maps of small tiles (3x3 convs with 64-cout groups)
 *     "nc2"       (fp32) two cout fragments per wave (32 couts x <= 64 pixels) in the conv kernel where the plan allows: a third fewer LDS reads
 *     "xtile"     (fp32) conv workgroups stay resident and walk several tiles, the next tile's first stage fetched under this tile's last k loop
 *     "blk32"     (fp32) the tensors read by 3x3 convs in 8- / 16-channel stages stored as 8-channel blocks per image
 *     "c3k2f"     (fp32) Bottleneck + closing 1x1 of the 104 x 104 C3k2 block in one launch (k_c3k2_f32)
 *     "pw32"      (fp32) 1x1 layers with >= 64 input channels on k_pw_f32: weights resident in LDS, activations straight from global memory
 *     "upacc"     (fp32, with "upfold") the 1x1 behind [Upsample x2 | skip] as two launches: the upsampled half's product once per COARSE pixel
 *                 (raw accumulators), then the skip half at full resolution with its accumulators starting from it -- the same fma chain, bit
 *                 for bit, without 3/4 of the upsampled half's multiply-adds
 *   issue of a forward (take effect at the next obb_forward): "graph" 1 = capture / replay hipGraphs (default), "fwd_split" 0..4
 *   concurrent sub-batch chains (default 0 = 2), "microbatch" 416 x 416 tiles per round (default and maximum 1024; smaller tiles
 *   get proportionally more per round, at most 16 384: 128 px -> 11 264). */
int obb_set_option(obb_ctx *ctx, const char *key, int64_t value);

/* ------------------------------------------------------------------ S2: compute_polygon_iou  (Detect_OBB.py:144-154) */
/* out[i] = IoU(a[i], b[i]); a, b: double[m*8].  Replaces Shapely Polygon/is_valid/intersection/area per pair. */
int obb_poly_iou_pairs(obb_ctx *ctx, const double *a, const double *b, int64_t m, double *out, obb_stream_t s);
/* out[i*nb+j] = IoU(a[i], b[j]) if cls_a[i]==cls_b[j] (or either cls pointer is NULL), else 0.
 * The O(N1*N2) loops of Detect_OBB.py:387-403 and :541-547. */
int obb_poly_iou_matrix(obb_ctx *ctx, const double *a, const int32_t *cls_a, int64_t na, const double *b,
                        const int32_t *cls_b, int64_t nb, double *out, obb_stream_t s);

/* Center-Hit metric (Detect_OBB.py:609-648): out[i*nq + j] = 1 iff point i (a detection centre, :159-165) lies strictly inside the
 * valid quad j  (`poly.is_valid and poly.contains(Point(cx, cy))`, :631-634) and cls_p[i] == cls_q[j] (when both are given). */
int obb_points_in_quads(obb_ctx *ctx, const double *pts, const int32_t *cls_p, int64_t np, const double *quads, const int32_t *cls_q,
                        int64_t nq, uint8_t *out, obb_stream_t s);

/* 4-channel network input (RGB + distance-transform edge channel) for every crop of a batch: `build_multich(crop_bgr, out_channels=4)`,
 * Detect_OBB.py:87-133 (called per tile at :77).  bgr: uint8[B,h,w,3], out4: uint8[B,h,w,4] = [R, G, B, dt_edge].  The OpenCV steps
 * are restated from their documented algorithms (cv2 is absent offline: parity with cv2 itself is unpinned). */
int obb_build_multich(obb_ctx *ctx, const uint8_t *bgr, int32_t B, int32_t h, int32_t w, uint8_t *out4, obb_stream_t s);
/* The same launches with a read-out of the intermediates (for tests): every non-NULL pointer receives, densely, acc float[B,h,w]
 * (max Scharr magnitude over the scales), edges uint8[B,h,w] (0 / 255, after the opening), dist float[B,h,w] (the chamfer distance)
 * and stats double[B,5] = the 90th percentile of acc, the 1st and 99th of dist, min and max of acc.  All NULL == obb_build_multich. */
int obb_build_multich_stages(obb_ctx *ctx, const uint8_t *bgr, int32_t B, int32_t h, int32_t w, uint8_t *out4, float *acc, uint8_t *edges,
                             float *dist, double *stats, obb_stream_t s);

/* ------------------------------------------------------------------ S3: merge_detections  (Detect_OBB.py:176-200) */
/* order[n] = stable descending argsort of key (Python list.sort(key=conf, reverse=True), Detect_OBB.py:183). */
int obb_sort_desc_stable(obb_ctx *ctx, const double *key, int64_t n, int32_t *order, obb_stream_t s);
/* Pair-suppression bit matrix over boxes already in sorted order, column-block-major: bit (j % 64) of word
 * mask[(j / 64) * n + i] is set iff j > i, cls equal and IoU(i,j) >= thr  (Detect_OBB.py:193).
 * mask: uint64[ceil(n/64) * n]. */
int obb_nms_mask(obb_ctx *ctx, const double *boxes_sorted, const int32_t *cls_sorted, int64_t n, double thr,
                 uint64_t *mask, obb_stream_t s);
/* Greedy scan of that matrix (Detect_OBB.py:186-198): keep[i] in sorted order, *n_keep = number kept. */
int obb_nms_reduce(obb_ctx *ctx, const uint64_t *mask, int64_t n, uint8_t *keep, int32_t *n_keep, obb_stream_t s);
/* The whole function: sort + suppression pairs + greedy scan.  order[n] (sorted position -> input index), keep[n] (sorted order).
 * No host read and no synchronisation at any n: the choice between the sparse pair list and the matrix-free dense scan (pair-list
 * overflow, thr <= 0) is taken on the device, so the call can be captured into a hipGraph once its workspaces exist (call it once
 * eagerly at the largest n first).  n <= 1.2 M rows. */
int obb_merge_detections(obb_ctx *ctx, const double *boxes, const int32_t *cls, const double *conf, int64_t n,
                         double thr, int32_t *order, uint8_t *keep, int32_t *n_keep, obb_stream_t s);
/* Batched form for the per-tile call at Detect_OBB.py:264: nseg independent segments, segment k owning rows
 * [seg_off[k], seg_off[k+1]) (device int32[nseg+1]); order holds GLOBAL row indices per sorted position.  Segments of up to 512 rows run
 * in one launch; longer ones are detected on the host and taken through the dense path of obb_merge_detections (synchronises then). */
int obb_merge_segments(obb_ctx *ctx, const double *boxes, const int32_t *cls, const double *conf,
                       const int32_t *seg_off, int32_t nseg, int64_t n, double thr, int32_t *order, uint8_t *keep,
                       obb_stream_t s);

/* ------------------------------------------------------------------ S4: cross_scale_consensus_filter  (Detect_OBB.py:347-423) */
/* Rows of all scales concatenated in ascending-scale order; scale k owns [off_host[k], off_host[k+1]).
 * out_idx[<= n] receives kept row indices in the reference's output order, *n_out their count.
 * Constants: CONS_IOU_PARTNER / CONS_LOW / CONS_HIGH (Detect_OBB.py:349-351). */
int obb_consensus(obb_ctx *ctx, const double *boxes, const int32_t *cls, const double *conf, const int64_t *off_host,
                  int32_t nscales, double iou_partner, double cons_low, double cons_high, int32_t *out_idx,
                  int32_t *n_out, obb_stream_t s);

/* ------------------------------------------------------------------ S5: detect_symbols  (Detect_OBB.py:202-266) */
/* Tile rectangles (x, y, x2, y2) in the reference's visiting order (Detect_OBB.py:211-223).  Host-only helper:
 * rects_host int32[max_tiles*4]; *n_tiles receives the full count even when it exceeds max_tiles. */
int obb_tile_grid(int32_t H, int32_t W, int32_t tile, int32_t overlap, int32_t *rects_host, int64_t max_tiles,
                  int64_t *n_tiles);
/* Per-detection work of the tile loop (Detect_OBB.py:229-262): local float32 corners + integer tile offset in
 * float64 (exact), inclusive border filter with `margin`, strike angle for class `strike_cls` (else 0.0).
 * local_pts float[n*8], det_tile int32[n] (index into rects), rects int32[ntiles*4] (device). */
int obb_tile_postprocess(obb_ctx *ctx, const float *local_pts, const int32_t *cls, const int32_t *det_tile, int64_t n,
                         const int32_t *rects, int32_t ntiles, int32_t margin, int32_t strike_cls, double *gboxes,
                         double *angle, uint8_t *inside, obb_stream_t s);
/* The whole stretch between the NMS output and the exchange records of a batch of tiles, on the device with no host-visible count in
 * between (Detect_OBB.py:228-264 per tile): Results.obb construction of each NMS row (regularize_rboxes, scale_boxes with the tile's
 * letterbox lb[t] = (gain, pad_x, pad_y) or NULL, xywhr2xyxyxyxy), the per-detection body (:229-262: global corners, border filter with
 * `margin`), the per-tile merge_detections (:264, threshold iou_thr) and the compaction of the survivors into 48-byte records
 * {tile id, class, conf (float32 bits), 0, 8 x local corner (float32 bits)} in tile order, merge (confidence) order inside a tile.
 * det float[B*max_det*7] + count int32[B]: the outputs of obb_decode_nms; tile_ids int32[B]: index of each tile into rects int32[*][4];
 * records int32[B*max_det*12] (capacity), tile_off int32[B+1] (first record of every tile), *n_records (device) = tile_off[B].
 * max_det <= 512.  Bit-identical to obb_results -> obb_tile_postprocess -> obb_merge_segments on the same rows (shared device code). */
int obb_tile_survivors(obb_ctx *ctx, const float *det, const int32_t *count, int32_t B, int32_t max_det, const float *lb,
                       const int32_t *tile_ids, const int32_t *rects, int32_t margin, int32_t strike_cls, double iou_thr,
                       int32_t *records, int32_t *tile_off, int32_t *n_records, obb_stream_t s);
/* Ordered compaction of a merge result (the list comprehension that closes merge_detections, Detect_OBB.py:198-200): out row r =
 * input row order[i] of the r-th sorted position i with keep[i] != 0; *n_out (device) = number of rows written.  angle / out_angle
 * may be NULL.  Output buffers hold n rows. */
int obb_select_kept(obb_ctx *ctx, const int32_t *order, const uint8_t *keep, int64_t n, const double *boxes, const int32_t *cls,
                    const double *conf, const double *angle, double *out_boxes, int32_t *out_cls, double *out_conf, double *out_angle,
                    int32_t *n_out, obb_stream_t s);
/* Consumer side of the 48-byte records: global float64 corners (float32 local corner + integer tile offset: exact), class, confidence
 * widened to float64 and the strike angle (Detect_OBB.py:229-234, 251-254), straight from the packed rows records int32[n][12]. */
int obb_records_to_dets(obb_ctx *ctx, const int32_t *records, int64_t n, const int32_t *rects, int32_t strike_cls, double *gboxes,
                        int32_t *cls, double *conf, double *angle, obb_stream_t s);
/* Multi-GPU exchange: the valid rows of a fixed-capacity all-gather buffer recv int32[world][capacity+1][12]
 * (row 0 of every rank's block carries its record count in column 0) -> dense out int32[<= world*capacity][12] in rank order;
 * counts int32[world+1] (device): every rank's count as sent (a count above `capacity` tells the caller to repeat the exchange with a
 * larger one) and, last, the number of rows written. */
int obb_gather_compact(obb_ctx *ctx, const int32_t *recv, int32_t world, int32_t capacity, int32_t *out, int32_t *counts, obb_stream_t s);
/* Gather all full-size tiles of one image into an NHWC uint8 batch (Detect_OBB.py:218-220 crop, vectorised).
 * image uint8[H*W*C]; rects device int32[ntiles*4] must all be tile x tile. */
int obb_gather_tiles(obb_ctx *ctx, const uint8_t *image, int32_t H, int32_t W, int32_t C, const int32_t *rects,
                     int32_t ntiles, int32_t tile, uint8_t *tiles_out, obb_stream_t s);
/* Letterbox one partial crop to (out_h, out_w) the way the Ultralytics predictor does for a single image
 * (LetterBox auto=True stride 32, pad value 114, bilinear resize only when the gain != 1; SURVEY.md Appendix A2;
 * call site Detect_OBB.py:81-83).  Returns gain and left/top pad through *_host pointers. */
int obb_letterbox(obb_ctx *ctx, const uint8_t *image, int32_t H, int32_t W, int32_t C, int32_t x, int32_t y, int32_t x2,
                  int32_t y2, int32_t imgsz, uint8_t *out, int32_t out_h, int32_t out_w, obb_stream_t s);

/* ------------------------------------------------------------------ training step, slice 2 */
/* RotatedTaskAlignedAssigner.forward of ultralytics==8.3.196 (utils/tal.py; reached from `model.train(...)`, Train_OBB.py:796-841, through
 * v8OBBLoss with topk = 10, alpha = 0.5, beta = 6.0): pd_scores float[bs][na][nc] (sigmoid scores), pd_bboxes float[bs][na][5] (x, y, w,
 * h, theta in pixels), anc_points float[na][2], gt_labels int32[bs][n_max], gt_bboxes float[bs][n_max][5], mask_gt uint8[bs][n_max] ->
 * target_labels int32[bs][na], target_bboxes float[bs][na][5], target_scores float[bs][na][nc], fg_mask uint8[bs][na],
 * target_gt_idx int32[bs][na].  na <= 10240.  All device pointers. */
int obb_rotated_tal_assign(obb_ctx *ctx, const float *pd_scores, const float *pd_bboxes, const float *anc_points, const int32_t *gt_labels,
                           const float *gt_bboxes, const uint8_t *mask_gt, int32_t bs, int32_t na, int32_t nc, int32_t n_max, int32_t topk,
                           float alpha, float beta, int32_t *target_labels, float *target_bboxes, float *target_scores, uint8_t *fg_mask,
                           int32_t *target_gt_idx, obb_stream_t s);

/* ------------------------------------------------------------------ training step, slice 3 */
/* Backward of a stride-1 convolution with `same` padding (k = 1 or 3), bf16 NHWC tensors, fp32 accumulation (Train_OBB.py:796-841: bf16
 * autocast over fp32 master weights).  dgrad: dy bf16[B][H][W][cout] (device), w fp32[cout][cin][k][k] (HOST: repacked per call into
 * the MFMA fragment order of the forward kernel; (synchronises)) -> dx bf16[B][H][W][cin].  wgrad: x bf16[B][H][W][cin], dy -> dw fp32[cout][cin][k][k]
 * (device), cin and cout multiples of 64; deterministic (fixed summation order). */
int obb_conv_dgrad_bf16(obb_ctx *ctx, const uint16_t *dy, const float *w_oihw_host, int32_t B, int32_t H, int32_t W, int32_t cin,
                        int32_t cout, int32_t ks, uint16_t *dx, obb_stream_t s);
int obb_conv_wgrad_bf16(obb_ctx *ctx, const uint16_t *x, const uint16_t *dy, int32_t B, int32_t H, int32_t W, int32_t cin, int32_t cout,
                        int32_t ks, float *dw, obb_stream_t s);
/* Assembled-chain pieces (round 4; Train_OBB.py:796-841 -> loss.backward() under bf16 autocast over fp32 master weights):
 * obb_conv_pack_bf16: fp32 OIHW master weights ON THE DEVICE -> the bf16 MFMA fragment order of the forward kernel (n_elems from
 *   obb_conv_packed_elems for the same shape); dgrad_form 1 packs the flipped / channel-transposed weights, so that
 *   obb_conv_fwd_bf16(dy, packed_dgrad, NULL, ..., cin = cout, cout = cin) IS the input gradient -- no host repack, no synchronisation.
 * obb_conv_fwd_bf16: y = conv(x) + bias, stride 1, `same` padding, NO activation (the pre-activation is kept for the backward), bf16
 *   NHWC in / out, fp32 accumulation, one bf16 rounding.
 * obb_silu_bf16 / obb_silu_bwd_bf16: a = z sigmoid(z);  dz = da * s (1 + z (1 - s)).   obb_bias_grad_bf16: db[c] = sum_pixels dy[pixel][c] (fp32). */
int obb_conv_packed_elems(obb_ctx *ctx, int32_t cout, int32_t cin, int32_t ks, int32_t H, int32_t W, int32_t dgrad_form, int64_t *n_elems);
int obb_conv_pack_bf16(obb_ctx *ctx, const float *w_oihw, int32_t cout, int32_t cin, int32_t ks, int32_t H, int32_t W, int32_t dgrad_form,
                       uint16_t *packed, obb_stream_t s);
int obb_conv_fwd_bf16(obb_ctx *ctx, const uint16_t *x, const uint16_t *packed_w, const float *bias, int32_t B, int32_t H, int32_t W, int32_t cin,
                      int32_t cout, int32_t ks, uint16_t *y, obb_stream_t s);
int obb_silu_bf16(obb_ctx *ctx, const uint16_t *z, uint16_t *a, int64_t n, obb_stream_t s);
int obb_silu_bwd_bf16(obb_ctx *ctx, const uint16_t *z, const uint16_t *da, uint16_t *dz, int64_t n, obb_stream_t s);
int obb_bias_grad_bf16(obb_ctx *ctx, const uint16_t *dy, int64_t npix, int32_t cout, float *db, obb_stream_t s);
/* Stride-2 3x3 convolution (pad 1; input H x W, output Ho = (H + 1) / 2 x Wo = (W + 1) / 2): the downsampling Convs of the backbone and the
 * PAN (yolo11 models 3 / 5 / 7 / 17 / 20) in `model.train(...)` (Train_OBB.py:796-841), bf16 NHWC tensors, fp32 accumulation.
 * obb_conv_s2_pack_bf16: fp32 OIHW master weights (device) -> the forward kernel's bf16 fragment order for an H x W input (n_elems from
 *   obb_conv_s2_packed_elems).   obb_conv_fwd_s2_bf16: y[B][Ho][Wo][cout] = conv_s2(x[B][H][W][cin]) + bias (NULL: none), no activation.
 * obb_conv_dgrad_s2_bf16: dx[B][H][W][cin] = sum_k dY_up[m + 1 - k] W[k] with dY_up = dy[B][Ho][Wo][cout] zero-inserted (dY_up[2i] = dy[i]):
 *   the stride-1 forward on obb_conv_pack_bf16(w, cout, cin, 3, H, W, dgrad_form = 1) weights (4x the useful MACs).
 * obb_conv_wgrad_s2_bf16: dw[cout][cin][3][3] fp32 = sum_{b,i,j} dy[b,i,j,co] x[b, 2i + ky - 1, 2j + kx - 1, ci]; cin and cout multiples of 64
 *   (models 0 and 1, 3 -> 32 -> 64, are rejected); deterministic. */
int obb_conv_s2_packed_elems(obb_ctx *ctx, int32_t cout, int32_t cin, int32_t H, int32_t W, int64_t *n_elems);
int obb_conv_s2_pack_bf16(obb_ctx *ctx, const float *w_oihw, int32_t cout, int32_t cin, int32_t H, int32_t W, uint16_t *packed, obb_stream_t s);
int obb_conv_fwd_s2_bf16(obb_ctx *ctx, const uint16_t *x, const uint16_t *packed_w, const float *bias, int32_t B, int32_t H, int32_t W, int32_t cin,
                         int32_t cout, uint16_t *y, obb_stream_t s);
int obb_conv_dgrad_s2_bf16(obb_ctx *ctx, const uint16_t *dy, const uint16_t *packed_dgrad, int32_t B, int32_t H, int32_t W, int32_t cin, int32_t cout,
                           uint16_t *dx, obb_stream_t s);
int obb_conv_wgrad_s2_bf16(obb_ctx *ctx, const uint16_t *x, const uint16_t *dy, int32_t B, int32_t H, int32_t W, int32_t cin, int32_t cout, float *dw,
                           obb_stream_t s);
/* The bf16 weights of EVERY dense Conv of `model.train(...)` for one iteration in one launch (Train_OBB.py:796-841: autocast casts each fp32
 * master weight once per forward; here that cast is the pack of obb_conv_pack_bf16 / obb_conv_s2_pack_bf16, per layer in its forward form and
 * its dgrad form).  The layers' weights are windows of ONE flat fp32 device buffer and the blobs segments of ONE bf16 device buffer, each
 * segment starting at a multiple of 256 elements and bit-identical to what the per-layer entry writes.
 * obb_conv_pack_plan (once per layer list and input size; it copies the table to the device and synchronises): record i = a layer cout[i] x
 *   cin[i] x ks[i] x ks[i] of stride[i] whose INPUT map is H[i] x W[i], in the form dgrad_form[i] (1: the stride plays no part, as in
 *   obb_conv_dgrad_s2_bf16), its weights at element src_off[i] of a flat buffer of src_elems elements -> dst_off[i], n_elems[i] (the segment of
 *   record i in the packed buffer), *total (elements of the packed buffer, a multiple of 256) and, unless `table` is NULL, the device table of
 *   table_words = OBB_PACK_TABLE_HEAD + nrec * OBB_PACK_TABLE_REC int64 words.
 * obb_conv_pack_multi_bf16 (every step): ONE kernel launch, no host read, copy, allocation or synchronisation (capturable in a graph).  w_flat /
 *   w_elems: the flat buffer; table / table_words / nrec and packed / packed_elems as the plan gave them.  A table size that does not match nrec,
 *   a packed_elems that is no positive multiple of 256 or a NULL pointer is refused with OBB_ERR_INVALID before any launch; a table whose own
 *   head disagrees with nrec, packed_elems or w_elems (a plan made for other layers or another input size) makes the kernel store nothing. */
#define OBB_PACK_TABLE_HEAD 4
#define OBB_PACK_TABLE_REC 8
int obb_conv_pack_plan(obb_ctx *ctx, int32_t nrec, const int32_t *cout, const int32_t *cin, const int32_t *ks, const int32_t *stride, const int32_t *H,
                       const int32_t *W, const int32_t *dgrad_form, const int64_t *src_off, int64_t src_elems, int64_t *dst_off, int64_t *n_elems,
                       int64_t *total, int64_t *table, int64_t table_words, obb_stream_t s);
int obb_conv_pack_multi_bf16(obb_ctx *ctx, const float *w_flat, int64_t w_elems, const int64_t *table, int64_t table_words, int32_t nrec,
                             uint16_t *packed, int64_t packed_elems, obb_stream_t s);
/* Weight gradient of every dense Conv of `model.train(...)` (Train_OBB.py:796-841 -> loss.backward() through Conv2d under bf16 autocast) whose
 * channel counts are multiples of 8, both >= 8 -- what obb_conv_wgrad_bf16 / obb_conv_wgrad_s2_bf16 refuse below multiples of 64: model.1, the
 * C3k2 Bottlenecks down to 16 -> 8, the 1x1s behind a 48- / 96-channel concat, the head's angle branch.  (ks, stride) = (1, 1), (3, 1) or
 * (3, 2); x bf16[B][H][W][cin], dy bf16[B][Ho][Wo][cout] (Ho = H at stride 1, (H + 1) / 2 at stride 2) -> dw fp32[cout][cin][ks][ks], all on
 * the device; fp32 accumulation of exact products, deterministic (fixed summation order).  Multiples of 64 are accepted too: one kernel and
 * one launch plan serve all three entry points, so there the results are bit-identical to the two above.  B >= 1. */
int obb_conv_wgrad_c8_bf16(obb_ctx *ctx, const uint16_t *x, const uint16_t *dy, int32_t B, int32_t H, int32_t W, int32_t cin, int32_t cout, int32_t ks,
                           int32_t stride, float *dw, obb_stream_t s);
/* Training-mode BatchNorm2d + SiLU of the Ultralytics Conv block (Conv2d(bias=False) -> BatchNorm2d -> SiLU, `model.train(...)`), z / a / da / dz
 * bf16 [npix][C] (NHWC rows), C % 8 == 0, npix >= 2; per-channel vectors fp32 [C], all on the device.
 * obb_bn_silu_fwd_bf16: mean, invstd = 1 / sqrt(var + eps) of the batch (biased var); running_mean / running_var updated in place,
 *   r = (1 - momentum) r + momentum * batch (running var: the unbiased var N / (N - 1)); a = silu(gamma (z - mean) invstd + beta).
 * obb_bn_silu_bwd_bf16: xhat and y = gamma xhat + beta recomputed from z, g = da silu'(y): dbeta = sum g, dgamma = sum g xhat,
 *   dz = gamma invstd (g - dbeta / N - xhat dgamma / N).  Reductions: per-block fp32 partials combined in a fixed order (deterministic). */
int obb_bn_silu_fwd_bf16(obb_ctx *ctx, const uint16_t *z, int64_t npix, int32_t C, const float *gamma, const float *beta, float eps, float momentum,
                         float *running_mean, float *running_var, float *mean, float *invstd, uint16_t *a, obb_stream_t s);
int obb_bn_silu_bwd_bf16(obb_ctx *ctx, const uint16_t *z, const uint16_t *da, int64_t npix, int32_t C, const float *gamma, const float *beta,
                         const float *mean, const float *invstd, float *dgamma, float *dbeta, uint16_t *dz, obb_stream_t s);
/* Gradient routing through what is not a convolution (`model.train(...)`, Train_OBB.py:796-841 -> ultralytics SPPF / nn.Upsample / Concat:
 * yolo11 models 9, 11/12, 14/15, 18, 21), bf16 NHWC device tensors, channel counts multiples of 8 (>= 8), B, H, W >= 1.  No atomics, fixed
 * summation order (bit-reproducible), no workspace.
 * obb_sppf_pools_fwd_bf16: cat[B][H][W][4C] = [x, y1, y2, y3], y_k = maxpool5x5(y_{k-1}), y0 = x[B][H][W][C] (stride 1, pad 2, padding never
 *   wins); one launch, the map of a workgroup's channels resident in LDS: H <= 32 and W <= 32, larger maps are OBB_ERR_INVALID.  Values are
 *   copied, not re-rounded: bit-equal to F.max_pool2d on the same bf16 values.
 * obb_sppf_pools_bwd_bf16: dx[B][H][W][C] from cat and dcat[B][H][W][4C] alone.  The argmax of level k is recomputed from member k - 1 of cat
 *   as the first maximum of a row-major scan of the window (strict >, torch's rule); gather form, level 3 -> 1, fp32 sums in LDS, the dcat
 *   member of each level added there, one bf16 rounding at the store.
 *   Both pool kernels require FINITE inputs (SiLU outputs are): on those the selection is torch's.  A NaN is not propagated (torch's scan has
 *   an isnan clause) and a window that is all -inf passes no gradient (torch sends it to the window's first element).
 * obb_upcat_fwd_bf16: out[B][up H][up W][Ca + Cb] = cat(nearest_upsample_up(a[B][H][W][Ca]), b[B][up H][up W][Cb]) along C, a first
 *   (Ultralytics' Concat([-1, skip])), up in {1, 2}; up = 1 is the plain concat.  Bit-exact copies.
 * obb_upcat_bwd_bf16: da[p] = the sum of the up^2 elements of dout[..., :Ca] that p was copied to (fp32, dy then dx, one bf16 rounding),
 *   db = dout[..., Ca:].  accum_a / accum_b = 1: the existing bf16 value of da / db is read and added in fp32 before the one rounding (the
 *   gradient sum of a tensor with two consumers).  da or db NULL: that half is skipped. */
int obb_sppf_pools_fwd_bf16(obb_ctx *ctx, const uint16_t *x, int32_t B, int32_t H, int32_t W, int32_t C, uint16_t *cat, obb_stream_t s);
int obb_sppf_pools_bwd_bf16(obb_ctx *ctx, const uint16_t *cat, const uint16_t *dcat, int32_t B, int32_t H, int32_t W, int32_t C, uint16_t *dx,
                            obb_stream_t s);
int obb_upcat_fwd_bf16(obb_ctx *ctx, const uint16_t *a, const uint16_t *b, int32_t B, int32_t H, int32_t W, int32_t Ca, int32_t Cb, int32_t up,
                       uint16_t *out, obb_stream_t s);
int obb_upcat_bwd_bf16(obb_ctx *ctx, const uint16_t *dout, int32_t B, int32_t H, int32_t W, int32_t Ca, int32_t Cb, int32_t up, uint16_t *da,
                       uint16_t *db, int32_t accum_a, int32_t accum_b, obb_stream_t s);
/* Depthwise 3x3 Conv blocks in training mode (`model.train(...)`, Train_OBB.py:796-841 -> ultralytics DWConv / Conv(g = c): the head's class
 * branch model.23.cv3.i.{0,1}.0 and C2PSA's attn.pe): stride 1, pad 1 (zeros), groups = C, no bias, no activation.  x, z, dz, dx bf16 NHWC
 * [B][H][W][C] on the device, C % 8 == 0 (>= 8), B, H, W >= 1, no map-size limit.  w: the fp32 MASTER weights [C][1][3][3] on the device; every
 * kernel rounds them to bf16 (nearest even) as it loads them (w~ below: what bf16 autocast hands F.conv2d) -- there is no pack step.  Products and
 * sums are fp32, taps are added in (ky, kx) ascending order starting from 0, one bf16 rounding at each bf16 store; dw is fp32 [C][1][3][3].
 * obb_dwconv3_fwd_bf16: z[b,i,j,c] = sum_{ky,kx} w~[c,ky,kx] x[b, i+ky-1, j+kx-1, c].
 * obb_dwconv3_bwd_bf16: BOTH gradients from one pass over x and dz:
 *   dx[b,i,j,c] = sum_{ky,kx} w~[c,ky,kx] dz[b, i-ky+1, j-kx+1, c];   dw[c,ky,kx] = sum_{b,i,j} dz[b,i,j,c] x[b, i+ky-1, j+kx-1, c].
 *   dx or dw NULL: that half is skipped and nothing of it is written (x may then be NULL for dx alone, w for dw alone); the half that is
 *   computed is bit-equal to the fused call's.  Both NULL: OBB_ERR_INVALID.  dw: per-lane fp32 sums, a fixed LDS tree over the lanes of a channel
 *   chunk, one fp32 slab per workgroup in a ctx workspace slot, a second launch that adds the slabs in index order.  No atomics: results are
 *   bit-reproducible, also after the workspace slot has grown.
 * obb_dwconv3_bwd_geometry: host only, no context.  out = {rows per stripe, pixels per lane run, number of slabs, L} -- the split the launcher
 *   itself uses for that shape (it calls the same function); L = the longest chain of fp32 additions a dw element passes through (lane run +
 *   LDS tree depth + slab combine).  OBB_ERR_INVALID on a bad shape.
 * obb_bn_fwd_bf16 / obb_bn_bwd_bf16: obb_bn_silu_fwd_bf16 / obb_bn_silu_bwd_bf16 with `act`: 1 = SiLU (bit-identical to those), 0 = identity
 *   (a = gamma xhat + beta; g = da) for Conv(act=False). */
int obb_dwconv3_fwd_bf16(obb_ctx *ctx, const uint16_t *x, const float *w, int32_t B, int32_t H, int32_t W, int32_t C, uint16_t *z, obb_stream_t s);
int obb_dwconv3_bwd_bf16(obb_ctx *ctx, const uint16_t *x, const uint16_t *dz, const float *w, int32_t B, int32_t H, int32_t W, int32_t C, uint16_t *dx,
                         float *dw, obb_stream_t s);
int obb_dwconv3_bwd_geometry(int32_t B, int32_t H, int32_t W, int32_t C, int32_t out[4]);
int obb_bn_fwd_bf16(obb_ctx *ctx, const uint16_t *z, int64_t npix, int32_t C, const float *gamma, const float *beta, float eps, float momentum,
                    float *running_mean, float *running_var, float *mean, float *invstd, uint16_t *a, int32_t act, obb_stream_t s);
int obb_bn_bwd_bf16(obb_ctx *ctx, const uint16_t *z, const uint16_t *da, int64_t npix, int32_t C, const float *gamma, const float *beta,
                    const float *mean, const float *invstd, float *dgamma, float *dbeta, uint16_t *dz, int32_t act, obb_stream_t s);
/* The conv layers whose channel counts are no multiples of 8, in training mode (`model.train(...)`, Train_OBB.py:796-841): the head's plain
 * Conv2d 1x1 + bias outputs (model.23.cv3.i.2: c -> nc class logits, model.23.cv4.i.2: c -> 1 angle logit) and the stem (model.0: Conv 3x3,
 * stride 2, pad 1 on the 3- or 4-channel uint8 tile).  All buffers on the device.  w: the fp32 MASTER weights, rounded to bf16 (nearest even) by
 * every kernel as it loads them (w~; no pack step); products and sums fp32; no padded channel is ever read from or written to global memory.
 * HEAD, pixels flattened (N = B H W >= 1): x, dx bf16 [N][cin], cin % 8 == 0, 8 <= cin <= 512; w, dw fp32 [cout][cin], bias, db fp32 [cout],
 *   1 <= cout <= 64; y, dy fp32 [N][cout], DENSE rows of cout floats (4-byte accesses: no row alignment is assumed); x 16-byte aligned.
 * obb_headconv_fwd_bf16: y[n,o] = (sum_c w~[o,c] x[n,c]) + bias[o], c ascending from 0, the bias last (bias NULL: none).  fp32 out: no rounding.
 * obb_headconv_bwd_bf16: ALL gradients from one pass over x and dy; dy is rounded to bf16 as it is loaded (dy~):
 *   dx[n,c] = sum_o w~[o,c] dy~[n,o] (o ascending, one bf16 rounding);  dw[o,c] = sum_n dy~[n,o] x[n,c];  db[o] = sum_n dy~[n,o].
 *   dx NULL, or dw and db both NULL: that half is skipped and nothing of it is written (x may then be NULL for dx alone, w for dw / db alone);
 *   the half that is computed is bit-equal to the fused call's.  One of dw / db NULL: only the other is stored.  All three NULL:
 *   OBB_ERR_INVALID.  dw / db: per-lane fp32 sums, a fixed LDS tree over the lanes of a channel, one fp32 slab per workgroup in a ctx workspace
 *   slot, a second launch that adds the slabs in index order.  No atomics: bit-reproducible, also after the workspace slot has grown.
 * STEM: x uint8 [B][H][W][cin], cin 3 or 4, B, H, W >= 1, channel order as stored; the operand is x~ = bf16(v / 255) (fp32 division, nearest
 *   even: the inference stem's bf16-mode value); w, dw fp32 [cout][cin][3][3], cout % 8 == 0, 8 <= cout <= 64; z, dz bf16 [B][Ho][Wo][cout],
 *   Ho = (H + 1) / 2, Wo = (W + 1) / 2, 16-byte aligned; x 4-byte aligned at cin = 4 (byte loads at cin = 3: any address).
 * obb_stemconv_fwd_u8: z[b,i,j,o] = sum_{ky,kx,c} w~[o,c,ky,kx] x~[b, 2i+ky-1, 2j+kx-1, c], (ky, kx, c) ascending from 0, taps outside the map
 *   skipped, one bf16 rounding.  No bias (BatchNorm follows).
 * obb_stemconv_wgrad_u8: dw[o,c,ky,kx] = sum_{b,i,j} dz[b,i,j,o] x~[b, 2i+ky-1, 2j+kx-1, c]; slabs and a second launch as above.  There is no
 *   input gradient: the input is the image.
 * obb_headconv_bwd_geometry / obb_stemconv_wgrad_geometry: host only, no context.  out = {pixels per lane run, lane rows per workgroup RP,
 *   number of slabs nbx, L} -- the split the launcher itself uses for that shape (it calls the same function): lane row r of workgroup bx walks
 *   (output) pixels bx RP + r + t nbx RP, t = 0 .. run - 1; L = the longest chain of fp32 additions a dw / db element passes through
 *   (run + ceil(log2 RP) + ceil(nbx / 64) + 6).  OBB_ERR_INVALID on a bad shape. */
int obb_headconv_fwd_bf16(obb_ctx *ctx, const uint16_t *x, const float *w, const float *bias, int64_t N, int32_t cin, int32_t cout, float *y,
                          obb_stream_t s);
int obb_headconv_bwd_bf16(obb_ctx *ctx, const uint16_t *x, const float *dy, const float *w, int64_t N, int32_t cin, int32_t cout, uint16_t *dx,
                          float *dw, float *db, obb_stream_t s);
int obb_headconv_bwd_geometry(int64_t N, int32_t cin, int32_t cout, int32_t out[4]);
int obb_stemconv_fwd_u8(obb_ctx *ctx, const uint8_t *x, const float *w, int32_t B, int32_t H, int32_t W, int32_t cin, int32_t cout, uint16_t *z,
                        obb_stream_t s);
int obb_stemconv_wgrad_u8(obb_ctx *ctx, const uint8_t *x, const uint16_t *dz, int32_t B, int32_t H, int32_t W, int32_t cin, int32_t cout,
                          float *dw, obb_stream_t s);
int obb_stemconv_wgrad_geometry(int32_t B, int32_t H, int32_t W, int32_t cin, int32_t cout, int32_t out[4]);
/* Softmax attention core of C2PSA in training mode (`model.train(...)`, Train_OBB.py:796-841 -> ultralytics Attention(dim, num_heads,
 * attn_ratio = 0.5), model.10.m.*.attn), key_dim 32, head_dim 64, all tensors on the device.  Layout, the inference core's: qkv and dqkv bf16
 * [B][N][nh * 128], per token [q: nh * 32 | k: nh * 32 | v: nh * 64] (the qkv conv's output channels in DEVICE order, heads grouped); out, dout
 * and dv_add bf16 [B][N][nh * 64]; lse fp32 [B][nh][N].  scale = (float)(1 / sqrt(32.0)).  Limits: 1 <= N <= 192 (the keys of a head are
 * resident in LDS; a longer sequence is OBB_ERR_INVALID, not a slower path), nh >= 1, B >= 1; a NULL buffer other than dv_add is
 * OBB_ERR_INVALID; the bf16 buffers are 16-byte aligned.
 * obb_attn_fwd_bf16: S = scale q k^T, P = softmax over the keys of S, out = P v; lse[q] = max_k S[q][k] + log(sum_k exp(S[q][k] - max)) is the
 *   only thing kept for the backward.
 * obb_attn_bwd_bf16: P = exp(S - lse) recomputed from qkv and lse; dV = P^T dO (+ dv_add), dP = dO V^T, D[q] = sum_d dO[q][d] out[q][d],
 *   dS = P o (dP - D), dQ = scale dS K, dK = scale dS^T Q; EVERY element of dqkv is written.  dv_add may be NULL; given, it is added to dV in
 *   fp32 before dV's single bf16 rounding (the gradient of v's second consumer, attn.pe: the accumulate form of obb_upcat_bwd_bf16).
 * Rounding points: bf16 x bf16 products are exact in fp32; sums are fp32 (matrix-core accumulators; D: 16 products in index order per quarter,
 *   then (p0 + p1) + (p2 + p3)); exp / log are the hardware's base-2 instructions on arguments scaled by fp32 log2(e) / ln(2); P and dS enter
 *   their matrix products SPLIT into hi + lo bf16 parts (2^-16 relative is lost, they are not rounded to bf16); one bf16 rounding at each
 *   bf16 store, scale applied to the fp32 sum of dQ / dK just before it.
 * Determinism: every output row has one owner wave (a dQ row: the wave of its 16-query block, walking all keys; a dK / dV row: the wave of
 *   its 16-key block, walking all queries); no atomics, no cross-wave sum, no workspace: results are bit-reproducible.
 * obb_add_bf16: out[i] = bf16(fp32(a[i]) + fp32(b[i])), i < n, n % 8 == 0 (>= 8), 16-byte aligned; out may alias a.  The residual adds of a
 *   PSA block and the gradient sums at their fan-outs. */
int obb_attn_fwd_bf16(obb_ctx *ctx, const uint16_t *qkv, int32_t B, int32_t N, int32_t nh, uint16_t *out, float *lse, obb_stream_t s);
int obb_attn_bwd_bf16(obb_ctx *ctx, const uint16_t *qkv, const uint16_t *out, const float *lse, const uint16_t *dout, const uint16_t *dv_add,
                      int32_t B, int32_t N, int32_t nh, uint16_t *dqkv, obb_stream_t s);
int obb_add_bf16(obb_ctx *ctx, const uint16_t *a, const uint16_t *b, int64_t n, uint16_t *out, obb_stream_t s);
/* Channel-window routing of the composite blocks in training mode (`model.train(...)`, Train_OBB.py:796-841 -> `Tensor.chunk` / `split` /
 * `torch.cat` inside Ultralytics C3k2 (models 2, 4, 6, 8, 13, 16, 19, 22) and C2PSA (model 10), forward and backward).  src [npix][Cs], add
 * [npix][Ca], dst [npix][Cd]: bf16 NHWC tensors on the device with their leading dims flattened to npix pixels.
 * obb_chanwin_bf16: dst[p][d0 + j] = src[p][s0 + j] for p < npix, j < n; with add (may be NULL):
 *   dst[p][d0 + j] = bf16(fp32(src[p][s0 + j]) + fp32(add[p][a0 + j])), one rounding, obb_add_bf16's.  Every other channel of dst is left as it
 *   is.  Without add the 16-byte chunks are copied as bits (NaN payloads and -0 survive).  No LDS, no atomics, no workspace.
 *   Refused (nothing launched): n, Cs, Cd (Ca with add) not positive multiples of 8; s0, d0 (a0) not non-negative multiples of 8; a window
 *   past its tensor; npix < 1; a NULL src or dst; a pointer that is not 16-byte aligned; dst's bytes [dst, dst + npix Cd) overlapping src's or
 *   add's. */
int obb_chanwin_bf16(obb_ctx *ctx, const uint16_t *src, int32_t Cs, int32_t s0, const uint16_t *add, int32_t Ca, int32_t a0, int64_t npix, int32_t n,
                     uint16_t *dst, int32_t Cd, int32_t d0, obb_stream_t s);

/* ------------------------------------------------------------------ S1: model(...) -> results[0].obb  (Detect_OBB.py:26,81-83,228-231) */
/* Weight blob ("OBBW" format, produced by the Python side from BN-folded conv weights) for a
 * YOLO11-OBB graph (ultralytics==8.3.196 yolo11-obb.yaml).  Host pointer.  (synchronises) */
int obb_model_load(obb_ctx *ctx, const void *blob_host, size_t bytes);
/* Frees the model of `slot` (weights, activation slabs, captured graphs); the slot can be loaded again.  (synchronises) */
int obb_model_unload(obb_ctx *ctx, int32_t slot);
/* nc, input channels, number of anchors A for an (h, w) input, number of weight records. */
int obb_model_info(const obb_ctx *ctx, int32_t h, int32_t w, int32_t *nc, int32_t *ch, int32_t *anchors, int32_t *nconv);
/* OBBModel forward on B letterboxed inputs: tiles uint8[B*h*w*ch] (NHWC; BGR for ch==3 exactly as the reference
 * passes crops, Detect_OBB.py:93) -> raw head float[B*A*NO] with NO = 64+nc+1 rounded up to a multiple of 4 (per anchor:
 * 4x16 DFL logits, nc class logits, 1 angle logit, zero padding).  Preprocess (BGR->RGB, /255; Appendix A2) is fused
 * into the first convolution. */
int obb_forward(obb_ctx *ctx, const uint8_t *tiles, int32_t B, int32_t h, int32_t w, float *head, obb_stream_t s);
/* The same forward, which also leaves cmax float[B][A] = the largest class logit of every anchor (a dense tensor: the confidence gate of
 * obb_decode_nms_gate then reads 4 bytes per anchor instead of a 48-byte piece of every 320-byte head row).  Written by the fused class
 * tails of the head where the plan has them, by one extra pass over the head rows otherwise.  cmax NULL = obb_forward. */
int obb_forward_gate(obb_ctx *ctx, const uint8_t *tiles, int32_t B, int32_t h, int32_t w, float *head, float *cmax, obb_stream_t s);
/* Debug: text dump of the lowered forward for an (h, w) input -- one line per kernel launch (layer name, tiling,
 * grid, LDS bytes, MACs).  buf_host may be NULL to query *needed. */
int obb_debug_plan(obb_ctx *ctx, int32_t h, int32_t w, char *buf_host, int64_t buf_bytes, int64_t *needed);
/* Debug, host only (no context, no device): the packed fp32 weights of columns [c0, c0 + nc) of the 1x1 matrix w[cout][cin] exactly as the plan
 * builder packs them.  form 0: k_pw_f32 order (the coarse launch of "upacc"), 1: the two-fragment k_conv_f32 order (its fine launch), 2: the
 * order of the one-launch form over the whole virtual concat.  tiling_host (optional, forms 1 / 2): {channels per stage, waves along cout,
 * cout fragments per wave}.  out may be NULL to query *needed (floats). */
int obb_debug_pack_1x1(int32_t form, const float *w, int32_t cout, int32_t cin, int32_t c0, int32_t nc, float *out, int64_t max_floats,
                       int64_t *needed, int32_t *tiling_host);
/* Debug/parity tap: copy the activation called `name` (a conv's state-dict path such as "model.2.cv1", or a
 * layer output "x0".."x22") of the last forward to out as dense float[B*H*W*C] (bf16 widened).  out may be NULL to
 * query *n_elems / shape only. */
int obb_debug_activation(obb_ctx *ctx, int32_t h, int32_t w, int32_t B, const char *name, float *out, int64_t max_elems,
                         int64_t *n_elems, int32_t *shape_hwc_host, obb_stream_t s);
/* Decode (DFL, dist2rbox, angle, sigmoid; Appendix A4) + conf filter + class-offset ProbIoU Fast-NMS + max_det.
 * out float[B*max_det*7] rows (x, y, w, h, conf, cls, theta) in score order; count int32[B]. */
int obb_decode_nms(obb_ctx *ctx, const float *head, int32_t B, int32_t h, int32_t w, float conf_thres, float iou_thres,
                   int32_t max_det, float *out, int32_t *count, obb_stream_t s);
/* obb_decode_nms with the candidate gate read from cmax (obb_forward_gate's output for the SAME head tensor; NULL = obb_decode_nms): the
 * exact class scores are still taken from the head rows of the anchors that pass, so the result is identical. */
int obb_decode_nms_gate(obb_ctx *ctx, const float *head, const float *cmax, int32_t B, int32_t h, int32_t w, float conf_thres, float iou_thres,
                        int32_t max_det, float *det, int32_t *count, obb_stream_t s);
/* The same function in its full form (decode every anchor, then NMS sized for all of them): an independent implementation kept for the
 * parity tests, which require obb_decode_nms (candidate-first: conf filter on the class logits, decode + NMS of the survivors only) to
 * return the same rows bit for bit. */
int obb_decode_nms_full(obb_ctx *ctx, const float *head, int32_t B, int32_t h, int32_t w, float conf_thres, float iou_thres,
                        int32_t max_det, float *out, int32_t *count, obb_stream_t s);
/* Pieces of the above for parity tests: decoded predictions float[B*A*(4+nc+1)] (x,y,w,h, cls scores, theta). */
int obb_decode(obb_ctx *ctx, const float *head, int32_t B, int32_t h, int32_t w, float *pred, obb_stream_t s);
/* ProbIoU Fast-NMS on one candidate list: boxes float[n*5] (x,y,w,h,theta; class offset applied), scores float[n]. */
int obb_probiou_nms(obb_ctx *ctx, const float *boxes, const float *scores, int64_t n, float iou_thres, int32_t *order,
                    uint8_t *keep, obb_stream_t s);
/* Result construction (regularize_rboxes, scale_boxes(xywh=True), xywhr2xyxyxyxy; Appendix A6; consumed at
 * Detect_OBB.py:229-231).  det float[n*7] rows as written by obb_decode_nms; per-row letterbox params
 * lb float[n*3] = (gain, pad_x, pad_y) or NULL for identity.  xywhr float[n*5], pts float[n*8]. */
int obb_results(obb_ctx *ctx, const float *det, const float *lb, int64_t n, float *xywhr, float *pts, obb_stream_t s);

/* ------------------------------------------------------------------ f1 (first slice): the ProbIoU rotated-box loss of the training step */
/* `model.train(...)` (Train_OBB.py:796-841) -> ultralytics v8OBBLoss -> RotatedBboxLoss: loss_iou = sum((1 - probiou(pred, target)) * weight)
 * / target_scores_sum over the n matched (prediction, target) pairs, forward and backward in one pass.  pred, target float[n*5] rows
 * (x, y, w, h, theta); weight float[n] (NULL = 1); *loss (device float) receives the scalar, grad_pred float[n*5] = d loss / d pred. */
int obb_probiou_loss(obb_ctx *ctx, const float *pred, const float *target, const float *weight, int64_t n, float target_scores_sum,
                     float *loss, float *grad_pred, obb_stream_t s);

/* ------------------------------------------------------------------ f4: the training-set tiler's label assignment (Train_OBB.py:87-112) */
/* For every (tile, label) pair: mask uint8[ntiles*n] = 1 when the label goes into the tile's label file (midpoint of corners 1 and 4
 * inside the half-open tile AND >= min_fraction (object_boundary_threshold, :33) of its axis-aligned box inside), and then out
 * double[(t*n + l)*8] = its corners shifted to the tile, clipped to [0, tile] and divided by the tile size.  labels double[n*8] pixel
 * corners of one image; rects device int32[ntiles*4] (x, y, x2, y2) square tiles (the tiler only keeps full tiles, :83-84). */
int obb_tile_labels(obb_ctx *ctx, const double *labels, int64_t n, const int32_t *rects, int32_t ntiles, double min_fraction, uint8_t *mask,
                    double *out, obb_stream_t s);

/* f1 (second slice): the other two terms of v8OBBLoss, forward and backward in one pass each.
 * DFL (ultralytics DFLoss inside RotatedBboxLoss): pred_dist float[n*4*reg_max] logits of the n matched anchors' four sides, target_ltrb
 * float[n*4] = bbox2dist(anchor, xyxy(target), reg_max - 1) (clamped to [0, reg_max - 1.01] here as the reference does), weight float[n]
 * (NULL = 1); *loss = sum_i mean_side(CE(l) wl + CE(r) wr) weight_i / target_scores_sum; grad_pred float[n*4*reg_max].  reg_max must be 16. */
int obb_dfl_loss(obb_ctx *ctx, const float *pred_dist, const float *target_ltrb, const float *weight, int64_t n, int32_t reg_max,
                 float target_scores_sum, float *loss, float *grad_pred, obb_stream_t s);
/* classification term: BCEWithLogitsLoss(reduction="none")(logits, targets).sum() / target_scores_sum over n = batch * anchors * classes
 * elements; grad_logits float[n] = (sigmoid(logit) - target) / target_scores_sum. */
int obb_bce_loss(obb_ctx *ctx, const float *logits, const float *targets, int64_t n, float target_scores_sum, float *loss, float *grad_logits,
                 obb_stream_t s);

/* f1 (criterion chain): ultralytics v8OBBLoss.__call__ (restated from recall, parity unpinned) around the assigner, on the head's own outputs.
 * Three levels (strides 8, 16, 32; maps H[i] x W[i]; anchors row-major, levels concatenated, A = sum H[i] W[i]).  box, cls, angle, H, W (and
 * d_box, d_cls, d_angle, gains below) are HOST arrays of three; their elements are device pointers: box[i] [B][H][W][64] DFL logits, bf16
 * (box_bf16 != 0) or float, 16-byte aligned; cls[i] float [B][H][W][nc]; angle[i] float [B][H][W][1].  1 <= nc <= 64, B A nc <= 2^24.
 * obb_crit_decode: the assigner's inputs -- pd_scores float[B][A][nc] = sigmoid(cls), pd_bboxes float[B][A][5] = the decoded (x, y, w, h) in
 * pixels and theta (DFL expectation, dist2rbox, theta = (sigmoid(angle) - 0.25) pi), anc_points float[A][2] in pixels, stride float[A]. */
int obb_crit_decode(obb_ctx *ctx, const void *const *box, int32_t box_bf16, const float *const *cls, const float *const *angle, const int32_t *H,
                    const int32_t *W, int32_t B, int32_t nc, float *pd_scores, float *pd_bboxes, float *anc_points, float *stride, obb_stream_t s);
/* obb_crit_loss: given the assigner's target_bboxes float[B][A][5] (pixels), target_scores float[B][A][nc] and fg_mask uint8[B][A]:
 * tss[0] = max(sum target_scores, 1) (device); items[3] (device) = (g_box L_box, g_cls L_cls, g_dfl L_dfl), gains = (g_box, g_cls, g_dfl), with
 * L_box the ProbIoU term and L_dfl the DFL term over the foreground anchors (weight = sum_c target_scores, targets over the stride, ltrb clamped
 * to [0, 14.99]) and L_cls the BCE term over every anchor, each over tss; and the gradient of B * sum(items) with respect to every logit, in the
 * logits' layouts: d_box[i] bf16 (16-byte aligned), d_cls[i], d_angle[i] float.  Every element is written (background anchors: zeros in d_box and
 * d_angle); the decode is recomputed from the logits.  No host read: stream-ordered and capturable. */
int obb_crit_loss(obb_ctx *ctx, const void *const *box, int32_t box_bf16, const float *const *cls, const float *const *angle, const int32_t *H,
                  const int32_t *W, int32_t B, int32_t nc, const float *target_bboxes, const float *target_scores, const uint8_t *fg_mask,
                  const float *gains, void *const *d_box, float *const *d_cls, float *const *d_angle, float *items, float *tss, obb_stream_t s);

/* f1 (optimiser step): the update behind `model.train(...)` (Train_OBB.py:796-841; ultralytics `build_optimizer`: torch.optim.SGD with
 * nesterov momentum or torch.optim.AdamW, three parameter groups).  A group = flat fp32 device buffers of n elements, 16-byte aligned.
 * obb_sgd_step: d = grad + weight_decay * param; buf = first_step ? d : momentum * buf + d; d = nesterov ? d + momentum * buf : buf;
 * param -= lr * d (momentum 0: no buffer touched).  obb_adamw_step: torch.optim.AdamW's single-tensor order with step counted from 1;
 * the betas are double, as torch's Python floats: the bias corrections and 1 - beta come from them (1 - 0.999f is 1.3e-5 off 0.001). */
int obb_sgd_step(obb_ctx *ctx, float *param, const float *grad, float *momentum_buf, int64_t n, float lr, float momentum, float weight_decay,
                 int32_t nesterov, int32_t first_step, obb_stream_t s);
int obb_adamw_step(obb_ctx *ctx, float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n, int64_t step, float lr, double beta1,
                   double beta2, float eps, float weight_decay, obb_stream_t s);

/* f1 (trainer update): what ultralytics `BaseTrainer.optimizer_step` and `ModelEMA.update` do around that step inside `model.train(...)`
 * (Train_OBB.py:796-841), over SEGMENTS: a segment is one flat fp32 device buffer (a parameter group, or the buffer of BatchNorm running
 * statistics) of n[k] elements, 16-byte aligned; 0 <= nseg <= 8; the pointer and length arrays are HOST arrays of nseg entries.  n[k] = 0 is legal
 * (the segment is skipped, its pointers are not looked at).  Each call is one launch over all segments (none when every segment is empty); none
 * reads back to the host, and none uses atomics, so every result is reproducible bit for bit.
 * obb_grad_sumsq: replaces the per-tensor norms of `torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=10.0)`.  partials[j] = the sum of
 * squares (each square and each sum in double) of slab j: the 4096-element slabs of segment 0, then those of segment 1, ...;
 * obb_grad_sumsq_partials (host only) gives their count, sum_k ceil(n[k] / 4096); partials_cap = the workspace's capacity in doubles.
 * obb_clip_coef: the rest of clip_grad_norm_ without its host read.  total = sqrt(partials summed in index order, in double); clip[0] = total_norm =
 * (float)total; clip[1] = coef = (float)min(1, max_norm / (total + 1e-6)) (NaN for a NaN total, 0 for an infinite one: error_if_nonfinite=False);
 * clip[2] = 1.0f when total is finite, else 0.0f.  clip: device float[3]. */
int obb_grad_sumsq_partials(const int64_t *n, int32_t nseg, int64_t *count);
int obb_grad_sumsq(obb_ctx *ctx, const float *const *grad, const int64_t *n, int32_t nseg, double *partials, int64_t partials_cap, obb_stream_t s);
int obb_clip_coef(obb_ctx *ctx, const double *partials, int64_t npartials, double max_norm, float *clip, obb_stream_t s);
/* obb_sgd_step_multi / obb_adamw_step_multi: replace the in-place gradient scaling of clip_grad_norm_ and `optimizer.step()` over all parameter
 * groups: obb_sgd_step / obb_adamw_step of every segment with its own lr[k] and weight_decay[k] (host float[nseg]) on the gradient g * clip[1] (one
 * fp32 multiply; clip == NULL: the gradient as it is).  With clip[1] == 1.0f or clip == NULL the results are bit-identical to the single-group
 * entry points.  The gradient buffers are only read.  clip: the device float[3] of obb_clip_coef. */
int obb_sgd_step_multi(obb_ctx *ctx, float *const *param, const float *const *grad, float *const *momentum_buf, const int64_t *n, const float *lr,
                       const float *weight_decay, int32_t nseg, float momentum, int32_t nesterov, int32_t first_step, const float *clip, obb_stream_t s);
int obb_adamw_step_multi(obb_ctx *ctx, float *const *param, const float *const *grad, float *const *exp_avg, float *const *exp_avg_sq, const int64_t *n,
                         const float *lr, const float *weight_decay, int32_t nseg, int64_t step, double beta1, double beta2, float eps, const float *clip,
                         obb_stream_t s);
/* obb_grad_accumulate: replaces autograd's accumulation into `.grad` over the `accumulate` iterations between two optimiser steps (the kernels
 * here write gradients, they do not add to them): acc = first ? grad : acc + grad (first: acc is not read).
 * obb_ema_update: replaces the per-entry loop of `ModelEMA.update` over the state dict (weights AND BatchNorm running statistics):
 * ema = ema * d + (1 - d) * src in torch's order (v.mul_(d); v.add_((1 - d) * src): three fp32 roundings), d = (float)decay and 1 - d =
 * (float)(1 - decay) each rounded from double (1.0f - (float)0.9999 is 6e-4 off 1e-4 in relative terms). */
int obb_grad_accumulate(obb_ctx *ctx, float *const *acc, const float *const *grad, const int64_t *n, int32_t nseg, int32_t first, obb_stream_t s);
int obb_ema_update(obb_ctx *ctx, float *const *ema, const float *const *src, const int64_t *n, int32_t nseg, double decay, obb_stream_t s);

/* ------------------------------------------------------------------ f1 (training batches): the dataloader's augmentation, on the device */
/* What the Ultralytics dataloader does to a tile between the disk and `model.train(...)` (Train_OBB.py:796-841 leaves every augmentation argument at
 * its default: 4-image Mosaic with probability 1, RandomPerspective with translate 0.1 / scale 0.5 / degrees 0, RandomHSV 0.015 / 0.7 / 0.4, fliplr
 * 0.5), restated from recall: Ultralytics 8.3.x and cv2 are not installed, so parity with them is UNPINNED, like the criterion chain above; pinned
 * is the device against this repository's numpy / fp64 restatement (tests/aug_ref.py).
 *
 * Both entries read one device TABLE of B records of OBB_AUG_REC_BYTES bytes, 8-byte aligned, one per output tile:
 *   offset   0  double inv[6]    the map output pixel -> canvas, rows (m00 m01 m02) (m10 m11 m12); the host inverts M in double
 *   offset  48  double fwd[6]    M, canvas -> output: M = T R C of RandomPerspective.affine_transform with shear and perspective at 0
 *   offset  96  double scale     the scale factor inside R (box_candidates multiplies the boxes before the warp by it)
 *   offset 104  int32  xc, yc    the mosaic centre on the canvas, 0 <= xc, yc <= 2 s
 *   offset 112  int32  src[4]    pool tiles of the quadrants top-left, top-right, bottom-left, bottom-right; src[0] alone without mosaic
 *   offset 128  uint32 flags     OBB_AUG_MOSAIC | OBB_AUG_FLIPLR | OBB_AUG_FLIPUD | OBB_AUG_HSV
 *   offset 132  int32  reserved
 *   offset 136  uint8  lut[768]  lut_h = (i r0) mod 180 | lut_s = clip(i r1, 0, 255) | lut_v = clip(i r2, 0, 255), float64 -> uint8 on the host
 * The canvas is virtual: side S = 2 s with mosaic (pixel (u, v) belongs to the quadrant given by u < xc, v < yc and is pixel (u - padw, v - padh)
 * of that quadrant's tile, pads (xc - s, yc - s), (xc, yc - s), (xc - s, yc), (xc, yc): `_mosaic4` for equal-sized images), S = s and canvas = tile
 * src[0] without.  114 wherever that pixel is outside its tile, and outside the canvas.  The table is on the device, so the entries cannot look at
 * it: a record with a source index outside [0, N) or a centre outside [0, 2 s] makes ITS tile a no-op (nothing of that tile is written).
 *
 * obb_aug_tiles: pool uint8 [N][s][s][C] (C = 3 or 4, 4-byte aligned at C = 4) -> out uint8 [B][s][s][C].  Per output pixel (x, y), mirrored first
 * (x -> s - 1 - x, y -> s - 1 - y) under the flip bits: X = (rint(m00 x 1024) + rint((m01 y + m02) 1024) + 16) >> 5 and Y likewise (warpAffine's
 * INTER_LINEAR fixed point), integer part X >> 5, fraction fx = X & 31, four canvas taps under the weights 32 (32 - fx)(32 - fy), 32 fx (32 - fy),
 * 32 (32 - fx) fy, 32 fx fy, result (sum + 16384) >> 15.  With the HSV bit, channels 0..2 (channel 0 is B when bgr != 0, else R; channel 3 is
 * warped only) go through cv2's 8-bit BGR -> HSV (H in 0..179), the three LUTs and the float HSV -> BGR with saturate(rint(255 x)); without it the
 * warped bytes pass.  swap_rb != 0 swaps channels 0 and 2 on store.  2 <= s <= 16384, B <= 65535; a refused call writes nothing.
 *
 * obb_aug_labels: pool_labels double [N][Lmax][9] = class + 8 corner coordinates normalised to the tile (the tiler's rows), pool_counts int32 [N]
 * -> what OBBCriterion reads: gt_labels int32 [B][n_cap], gt_bboxes float [B][n_cap][5] = (x, y, w, h, theta) in pixels, mask_gt uint8 [B][n_cap],
 * count int32 [B].  Per candidate (quadrant q, label l), in fp64: corners to pixels, plus the quadrant's pad, clipped to [0, S]; M; the flips
 * (x -> s - x, y -> s - y); box_candidates on the axis-aligned box before (times scale) and after (clipped to [0, s]): w, h > wh_thr, aspect <
 * ar_thr, area after / before > area_thr; convex hull, clipped to [0, s]^2 (Sutherland-Hodgman, an empty result drops the label); the minimum-area
 * enclosing rectangle over the hull's edge directions (what xyxyxyxy2xywhr gets from cv2.minAreaRect), theta in [0, pi/2), w the extent along
 * (cos theta, sin theta), the first edge in hull order winning a tie; dropped when w < 2 or h < 2.  Survivors are compacted in (q, l) order; rows
 * behind them are zero and masked out; count is the true number of survivors even past n_cap (rows past n_cap are dropped).
 * Both entries only enqueue on the stream: no host read, no allocation, capturable. */
#define OBB_AUG_REC_BYTES 904
#define OBB_AUG_MOSAIC 1u
#define OBB_AUG_FLIPLR 2u
#define OBB_AUG_FLIPUD 4u
#define OBB_AUG_HSV 8u
int obb_aug_tiles(obb_ctx *ctx, const uint8_t *pool, int32_t N, int32_t s, int32_t C, const void *table, int32_t B, int32_t bgr, int32_t swap_rb,
                  uint8_t *out, obb_stream_t st);
int obb_aug_labels(obb_ctx *ctx, const double *pool_labels, const int32_t *pool_counts, int32_t N, int32_t Lmax, const void *table, int32_t B, int32_t s,
                   double wh_thr, double ar_thr, double area_thr, int32_t n_cap, int32_t *gt_labels, float *gt_bboxes, uint8_t *mask_gt, int32_t *count,
                   obb_stream_t st);

/* ------------------------------------------------------------------ validation of the net being trained */
/* The `val` pass `model.train(...)` runs on the EMA model after every epoch (Train_OBB.py:792-841), Ultralytics 8.3.x restated from recall (the
 * package is not installed: UNPINNED, like the schedule and the criterion above; pinned is the device against tests/val_ref.py in fp64).
 *
 * obb_fold_blob_f32: replaces `model.fuse()` (per layer: BatchNorm folded into its conv) + the host loop that lays the folded tensors out as a
 * weight blob.  ONE launch turns the four flat fp32 buffers of the trainer's state -- w_flat (conv weights, parameter group 0), g_flat (BatchNorm
 * gamma, group 1), b_flat (beta and the plain convs' biases, group 2), buffers (the running statistics); the live ones or the EMA's copies -- into
 * the fp32 DATA SECTION of an "OBBW" blob: per record the OIHW weights, then the bias, records in table order, no padding.  `table` (device int64,
 * table_words = OBB_FOLD_TABLE_HEAD + nrec * OBB_FOLD_TABLE_REC, written once by the host):
 *     head   [0] magic "OBBFOLD1" (0x4f4242464f4c4431)  [1] nrec  [2] out_elems  [3..6] elements the records read up to in w_flat, g_flat, b_flat,
 *            buffers (the caller holds buffers at least that long)  [7] 0
 *     record [0] weight offset in w_flat  [1] gamma offset in g_flat  [2] beta / bias offset in b_flat  [3] running-mean offset and [4] running-
 *            variance offset in buffers  [5] destination offset in out  [6] cout | (elements per output channel) << 32
 *            [7] first workgroup | kind << 32; record i owns ceil(cout (per + 1) / 256) workgroups, first workgroups ascending from 0
 * OBB_FOLD_BN: f = gamma / sqrt(var + eps), w' = w f, b' = beta - mean f, each operation rounded to fp32 on its own (correctly rounded IEEE division and square
 * root, nothing contracted).  OBB_FOLD_PLAIN: weight and bias copied.  OBB_FOLD_QKV: OBB_FOLD_BN for the attention's qkv conv, whose rows the trainer
 * holds as [q of all heads | k of all heads | v of all heads] (32, 32, 64 rows per head): output row c is read from that device row, so the
 * blob is in checkpoint order ([q | k | v] per head).  The kernel compares the head with nrec and out_elems and every record with the head; on a
 * mismatch nothing is stored.  No host read, no allocation, no synchronisation: capturable. */
#define OBB_FOLD_TABLE_HEAD 8
#define OBB_FOLD_TABLE_REC 8
#define OBB_FOLD_BN 0
#define OBB_FOLD_PLAIN 1
#define OBB_FOLD_QKV 2
int obb_fold_blob_f32(obb_ctx *ctx, const float *w_flat, const float *g_flat, const float *b_flat, const float *buffers, const int64_t *table,
                      int64_t table_words, int32_t nrec, float eps, float *out, int64_t out_elems, obb_stream_t s);
/* obb_val_match: replaces `OBBValidator._process_batch` = batch_probiou(gt, pred) + match_predictions.  det float [B][max_det][7] = (x, y, w, h,
 * conf, cls, theta) and count int32 [B] as obb_decode_nms writes them (score order; rows at or past count[b] are ignored whatever they hold);
 * gt_labels int32 [B][n_cap], gt_bboxes float [B][n_cap][5] = (x, y, w, h, theta), mask_gt uint8 [B][n_cap] (masked rows are ignored whatever
 * they hold); thr DEVICE float [n_thr], ascending (the trainer's: float32(linspace(0.5, 0.95, 10))).  Per detection d: g(d) = the class-equal,
 * unmasked ground truth with the largest ProbIoU (covariance form, eps 1e-7, fp32), ties to the lower index; d claims g(d) at threshold i iff
 * that IoU >= thr[i]; of the detections claiming one ground truth at one threshold the lowest index is the true positive, the others are false
 * positives (no fall-back to a second-best ground truth: the trainer's rule).  -> tp uint16 [B][max_det] (bit i = threshold i), best_iou float
 * [B][max_det], best_gt int32 [B][max_det] (-1: none; rows at or past count[b]: 0, 0, -1).  A class outside [0, nc) or a non-finite box, in a
 * detection or a ground truth, matches nothing and never forms an address.  One 256-lane workgroup per image.  Refused with nothing written:
 * n_cap outside [1, OBB_VAL_MAX_GT], max_det < 1, n_thr outside [1, OBB_VAL_MAX_THR], nc < 1, a NULL buffer.  Enqueues only: capturable. */
#define OBB_VAL_MAX_GT 512
#define OBB_VAL_MAX_THR 16
int obb_val_match(obb_ctx *ctx, const float *det, const int32_t *count, const int32_t *gt_labels, const float *gt_bboxes, const uint8_t *mask_gt,
                  int32_t B, int32_t max_det, int32_t n_cap, int32_t nc, const float *thr, int32_t n_thr, uint16_t *tp, float *best_iou,
                  int32_t *best_gt, obb_stream_t s);
/* The validation report (csrc/valreport.hip; Ultralytics 8.3.x restated from recall, parity UNPINNED).
 * obb_val_crit_decode / obb_val_crit_items: forward-only twins of obb_crit_decode / obb_crit_loss that read obb_forward's head float [B][A][NO] of
 * an h x w input in place (NO = 64 + nc + 1 rounded up to a multiple of 4; levels = strides 8, 16, 32; anchors in the head's own order; the
 * padding is never read; head 16-byte aligned).  obb_val_crit_decode: the same outputs and the same arithmetic as obb_crit_decode (bit-equal on
 * equal logits).  obb_val_crit_items: tss[0] = max(sum target_scores, 1); items[3] = (g_box L_box, g_cls L_cls, g_dfl L_dfl) as obb_crit_loss
 * defines them, gains a HOST array of three; no gradient is written; accumulate != 0 ADDS the three items to what items holds (a whole validation
 * pass needs no host read per batch; tss is always overwritten).  The sums run in a fixed order without floating-point atomics: two runs give the
 * same bits.  Refused with nothing written: B < 1, nc outside [1, 64], h or w no positive multiple of 32, B A nc > 2^24, a NULL or misaligned
 * buffer.  Enqueue only (the first call may grow the context's workspace). */
int obb_val_crit_decode(obb_ctx *ctx, const float *head, int32_t B, int32_t h, int32_t w, int32_t nc, float *pd_scores, float *pd_bboxes,
                        float *anc_points, float *stride, obb_stream_t s);
int obb_val_crit_items(obb_ctx *ctx, const float *head, int32_t B, int32_t h, int32_t w, int32_t nc, const float *target_bboxes,
                       const float *target_scores, const uint8_t *fg_mask, const float *gains, float *items, float *tss, int32_t accumulate,
                       obb_stream_t s);
/* obb_val_confusion: `ConfusionMatrix.process_batch` for OBB.  det, count, gt_labels, gt_bboxes, mask_gt as obb_val_match reads them.  Candidates =
 * the detections below min(count, max_det) with conf > conf_thr; IoU = obb_val_match's ProbIoU, CLASS-AGNOSTIC.  Each candidate picks the unmasked
 * ground truth with the largest IoU > iou_thr (ties: the lower index); of the candidates that picked one ground truth the one with the largest IoU
 * keeps it (ties: the lower index).  matrix int32 [nc + 1][nc + 1] is ADDED to (the caller zeroes it once per pass): [pred_cls][gt_cls] per kept
 * pair, [pred_cls][nc] per candidate left without a ground truth, [nc][gt_cls] per unmasked ground truth left without a detection.  A class outside
 * [0, nc) or a non-finite box, in a detection or a ground truth, matches nothing, counts nowhere and forms no address.  Integer adds only: the
 * result does not depend on scheduling.  One 256-lane workgroup per image.  Refused with nothing written: n_cap outside [1, OBB_VAL_MAX_GT],
 * max_det < 1, nc outside [1, 32766], a NaN threshold, a NULL buffer.  Enqueues only: capturable. */
int obb_val_confusion(obb_ctx *ctx, const float *det, const int32_t *count, const int32_t *gt_labels, const float *gt_bboxes, const uint8_t *mask_gt,
                      int32_t B, int32_t max_det, int32_t n_cap, int32_t nc, float conf_thr, float iou_thr, int32_t *matrix, obb_stream_t s);
/* obb_get_option: reads back what obb_set_option set ("model_slot": the active slot), so that a component that loads a model of its own -- the
 * validator's, next to whatever the application runs -- can put the context's slot and switches back as it found them.  Replaces nothing of the
 * reference: Ultralytics' validator owns a deep copy of the model instead. */
int obb_get_option(const obb_ctx *ctx, const char *key, int64_t *value);

#ifdef __cplusplus
}
#endif
#endif /* OBBHIP_H */
