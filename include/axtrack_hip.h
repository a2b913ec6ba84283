/*
 * axtrack_hip.h -- C ABI of libaxtrack_hip.so: AxTrack's detect + associate hot path on MI355X (gfx950).
 *
 * The reference (LoaloaF/axtrack) is pure Python; it has no FFI of its own. The seams this
 * library replaces are the Python call sites listed per function below (paths relative to the
 * reference repo). INTEGRATION.md shows the ctypes binding a maintainer of the reference adds.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes. Pointers prefixed d_ are DEVICE pointers (HIP),
 *     h_ are HOST pointers. `stream` is a hipStream_t passed as void* (NULL = default stream).
 *   - Every function returns 0 on success, a negative AXT_E* code on error and never throws;
 *     axt_last_error() returns a human-readable message for the calling thread.
 *   - No hidden global state: all device state lives in an axt_detector handle or in
 *     caller-provided buffers; calls are asynchronous on `stream` unless stated otherwise.
 *   - Detections of a frame are three parallel arrays (conf f32, x i32, y i32) of capacity
 *     `cap` per frame, sorted by descending confidence, plus a per-frame count.
 *   - Arguments outside the bounds stated per function: AXT_EINVAL before any device call, with the function's name or
 *     the offending value in axt_last_error(); output buffers and host outputs (*n_arcs, *n_cells, ...) stay as they
 *     were. Shared bounds: a frame or grid of H x W cells has H, W >= 1 and H * W <= 2^31 - 1 (cells are numbered
 *     y*W + x in i32); a floating-point argument must be finite unless its function says otherwise, and a NaN is
 *     always refused. Flag arguments (conn8, bg, big_endian, label_quirk, log_correct, flip_y, flip_x, rotate, and `on` of
 *     axt_conv_trainer_set_batch_stats) are read as zero / non-zero: any int is accepted. group (axt_link_paths,
 *     axt_target_paths) is any int: a value that no frame carries selects nothing. tests/contract_cases.py holds every
 *     bound as a table; the two are kept in step by the tests.
 */
#ifndef AXTRACK_HIP_H
#define AXTRACK_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AXT_OK 0
#define AXT_EINVAL (-22)   /* bad argument (shape, null pointer, capacity)          */
#define AXT_ENOMEM (-12)   /* device or host allocation failed                       */
#define AXT_EHIP (-5)      /* a HIP runtime call failed, see axt_last_error()        */
#define AXT_ERUNTIME (-71)  /* an internal consistency check failed (a bug: please report) */
#define AXT_INFEASIBLE 1   /* axt_mcf_solve: fewer than min_flow unit flows exist    */

#define AXT_TILE 512       /* TILESIZE (deployed_model/params.txt:33)                */
#define AXT_S 12           /* SX = SY  (deployed_model/params.txt:34-35)             */
#define AXT_CELLS (AXT_S * AXT_S)
#define AXT_YOLO_FLOATS (AXT_CELLS * 3)
#define AXT_IN_CH 5        /* 1 * (2*TEMPORAL_CONTEXT+1), core_functionality.py:66   */
#define AXT_N_WEIGHT_TENSORS 54   /* 8 conv blocks x 6 + 3 linear x 2                */

const char *axt_last_error(void);
int axt_abi_version(void);

/* ------------------------------------------------------------------------------------------
 * Detector: replaces YOLO_AXTrack (axtrack/machinelearning/model.py:20-125) in eval mode.
 * ------------------------------------------------------------------------------------------ */
typedef struct axt_detector axt_detector;

/* Builds the device-resident detector from the tensors of the reference's state_dict
 * (checkpoint layout: utils.py:258-272; key set: model.py:85-117).
 * h_tensors[54], host f32, in this order:
 *   for blk in ConvBlock_{0,1,2,4,5,7,8,10}:
 *     conv.weight[Co,Ci,3,3], conv.bias[Co], batchnorm.weight[Co], batchnorm.bias[Co],
 *     batchnorm.running_mean[Co], batchnorm.running_var[Co]
 *   then fcs.1.weight[1024,40960], fcs.1.bias, fcs.3.weight[1024,1024], fcs.3.bias,
 *        fcs.5.weight[432,1024], fcs.5.bias
 * BatchNorm (eps 1e-5) is folded into the convolution in f64 and rounded once to f32.
 * max_batch = largest number of tile-forwards one call will be asked for (sizes the workspace), 1 <= max_batch <= 65535.
 * Synchronous (returns after the upload has completed). */
int axt_detector_create(const float *const *h_tensors, int n_tensors, int max_batch,
                        axt_detector **out);
void axt_detector_destroy(axt_detector *det);

/* Arithmetic of the stride-1 conv blocks (blocks 2, 4, 5, 7, 8, 10 of model.py:85-103; 73 % of the forward pass's FLOPs;
 * mode 1 leaves block 10 on the direct kernel); parameters['CNN_ARITH'].
 * mode 2 (default after axt_detector_create, "f32" / "f32_winograd"): Winograd F(2x2,3x3) on the f32 matrix pipe -- every
 *   operation f32 (transforms are additions, G g G^T formed in f64 and rounded once), 16/36 of the direct multiplications;
 *   as close to an f64 convolution as the direct kernel, like the algorithms cuDNN / oneDNN choose for
 *   the reference's own Conv2d.
 * mode 0 ("f32_direct"): direct convolution, f32-in / f32-accumulate MFMA, a k-ordered chain of f32 FMAs per output.
 * mode 1 ("bf16x3", opt-in): every f32 operand split exactly into three bf16 terms, six partial products per multiply on
 *   the bf16 matrix pipe, f32 accumulation -- per-product error of the size of an f32 rounding.
 * The modes agree to ~1e-6 on the grids and are not bit-identical to each other. Packed weights of modes 1 and 2 are built
 * on the first switch to them. Synchronous. */
int axt_detector_set_arith(axt_detector *det, int mode);
/* The two stride-2 conv blocks (0 and 1) of the detector: fused = 1 (the default at create) runs them as ONE kernel that
 * keeps block 0's output in LDS (conv_s2_fused, cnn_front.hip) -- used whenever the frame width is a multiple of 4;
 * fused = 0 runs the two separate kernels (conv3x3_s2_k1), which other widths take in either setting. The fused kernel
 * sums block 1's products in another order: the grids of the two settings agree to f32 rounding (~1e-6), not bit for bit.
 * Takes effect from the next forward pass. (axt_detector_create starts with fused = 1 unless the environment holds
 * AXT_FUSE_S2=0 -- for A/B runs of unmodified callers.) */
int axt_detector_set_fused_front(axt_detector *det, int fused);
/* bytes of device memory held by the handle (packed weights + activation workspace) */
size_t axt_detector_device_bytes(const axt_detector *det);

/* detect_axons (model.py:119-125; call site AxonDetections.py:118):
 * d_x f32 [B,5,512,512] NCHW -> d_yolo f32 [B,12,12,3] (dim1 = x cell, dim2 = y cell,
 * last = conf, x_in_cell, y_in_cell). 0 <= B <= max_batch. */
int axt_cnn_forward(axt_detector *det, const float *d_x, int B, float *d_yolo, void *stream);

/* The same forward pass fed straight from the timelapse, fusing
 * Timelapse.get_frametiles_stack (Timelapse.py:111-125,150-157) into the first convolution:
 * d_frames f32 [T_all,H,W] is channel 0 of the context-padded sequence; detection frame t of
 * tile k reads frames t..t+4 at tile origin (tile_yx[2k]*512, tile_yx[2k+1]*512), zero beyond
 * H/W (ZeroPad2d at Timelapse.py:529-533). Output d_yolo f32 [n_frames, n_tiles, 12,12,3] for
 * detection frames t0 .. t0+n_frames-1. n_frames*n_tiles may exceed max_batch (chunked). t0 >= 0, n_frames >= 0 and
 * t0 + n_frames + 4 <= T_all; 1 <= n_tiles <= 256, every tile's origin inside the frame (row * 512 < H, col * 512 < W).
 * A tile index above 32767 is AXT_EINVAL whatever H and W are, here and in every entry point that takes h_tile_yx. */
int axt_cnn_forward_frames(axt_detector *det, const float *d_frames, int T_all, int H, int W,
                           int t0, int n_frames, const int32_t *h_tile_yx, int n_tiles,
                           float *d_yolo, void *stream);

/* The trunk alone, for training the linear head on cached features: the arguments and the chunking of
 * axt_cnn_forward_frames, stopping after conv block 10. d_feat f32 [n_frames*n_tiles, 40960] in the reference's flatten
 * order c*256 + h*16 + w (model.py:50-53): exactly the values the forward pass hands its first linear layer, in the
 * detector's current arithmetic and fused-front setting. Asynchronous. */
int axt_cnn_features_frames(axt_detector *det, const float *d_frames, int T_all, int H, int W, int t0, int n_frames,
                            const int32_t *h_tile_yx, int n_tiles, float *d_feat, void *stream);

/* The trunk up to conv block `block` of the package's numbering (0..7), for training the blocks after it:
 * axt_cnn_features_frames' arguments and chunking. block = 7: exactly axt_cnn_features_frames. block = 6: stops before conv
 * block 7 (ConvNet.ConvBlock_10); d_feat f32 [n_frames*n_tiles, 20480] is [item, 80, 16, 16] NCHW, the output of
 * ConvBlock_8 after its max-pool. block = 4: stops before conv block 5 (ConvNet.ConvBlock_7); d_feat f32
 * [n_frames*n_tiles, 81920] is [item, 80, 32, 32] NCHW, the output of ConvBlock_5 after its max-pool. block = 2
 * (axtrack_hip_trunk.h): stops before conv block 3; [item, 80, 64, 64]. Any other block: AXT_EINVAL. */
int axt_cnn_block_features_frames(axt_detector *det, const float *d_frames, int T_all, int H, int W, int t0, int n_frames,
                                  const int32_t *h_tile_yx, int n_tiles, int block, float *d_feat, void *stream);

/* The same forward pass in two calls, for input that arrives in chunks (Timelapse.from_host_u16: the reference's inference()
 * starts from a host Timelapse and construct_tiles() moves it to the device, Timelapse.py:492-566): axt_cnn_front_frames runs
 * conv blocks 0-5 (through the second max-pool) for the (frame, tile) items of frames t0 .. t0+n_frames-1 and leaves their
 * features in the detector's batch buffer from item `item0` on; after the last chunk axt_cnn_back runs the remaining conv
 * blocks and the three linear layers ONCE for items 0 .. n_items-1 (the first linear layer streams its 168 MB of weights per
 * call, whatever the batch) and writes d_yolo [n_items,12,12,3]. item0 + items <= max_batch. Same results, bit for bit, as
 * axt_cnn_forward_frames over the same items. item0 >= 0, 0 <= n_items <= max_batch. Asynchronous. */
int axt_cnn_front_frames(axt_detector *det, const float *d_frames, int T_all, int H, int W, int t0, int n_frames,
                         const int32_t *h_tile_yx, int n_tiles, int item0, void *stream);
int axt_cnn_back(axt_detector *det, int n_items, float *d_yolo, void *stream);

/* FLOPs of one tile-forward (algorithmic: 2*M*N*K of the unpadded layers). */
double axt_cnn_flops_per_tile(void);

/* Per-kernel timing for the roofline report (bench.py): on = 1, every kernel launch of the
 * forward pass is bracketed by HIP events on the launch stream; on = 2 + k, only the launches of
 * kernel id k are (two events per launch cost ~10 us of launch gap: bracketing all 19 launches of a
 * pass slows it by ~8 %, bracketing the dominant kernel alone by < 1 %); on = 0, none. Kernel ids: 0..7 the eight conv
 * blocks, 8/10/12 the linear-layer GEMMs, 9/11/13 their split-K reductions.
 * axt_detector_read_profile synchronises on the recorded events and returns, per kernel id, the
 * summed milliseconds, the number of launches and the number of tile-forwards since the last read (ms, launches, items:
 * host arrays of n >= AXT_N_CNN_KERNELS entries). on is not range-checked: a negative value acts as 1, a value above 15
 * brackets no kernel. */
#define AXT_N_CNN_KERNELS 14
int axt_detector_set_profiling(axt_detector *det, int on);
int axt_detector_read_profile(axt_detector *det, double *ms, int64_t *launches, int64_t *items, int n);
/* A kernel id outside 0..13 gives 0: there is no error to report. */
double axt_cnn_kernel_flops_per_tile(int kernel);

/* ------------------------------------------------------------------------------------------
 * Preprocessing ("next" row of the scope table, in front of the hot path): the dense part of
 * Timelapse._read_tiff, _clip_image_values, _log_adjust_image, _standardize
 * (Timelapse.py:205-326) as one fused pass: x = u16/65535 -> mask -> max(x-offset,0) ->
 * (x<clip_lower ? 0 : x) -> log2(1+x) -> x/scale. d_raw u16 [T,H,W]; d_mask u8 [H,W] or NULL;
 * offset / clip_lower in [0,1] units (0 = skip), finite; log_correct: zero / non-zero; scale > 0 (+inf allowed: every
 * pixel becomes 0); d_out f32 [T,H,W]. T, H, W >= 1.
 * ------------------------------------------------------------------------------------------ */
int axt_preprocess_u16(const uint16_t *d_raw, const uint8_t *d_mask, int T, int H, int W, float offset,
                       float clip_lower, int log_correct, float scale, float *d_out, void *stream);

/* The statistics Timelapse._standardize takes of the preprocessed frames before it scales them (Timelapse.py:286-302), per
 * frame, over the values axt_preprocess_u16 would write with scale = 1 -- no frame is written, 2 B of traffic per pixel:
 * n = how many values are != 0, sum and sumsq of the values (each f32 widened to f64 first), max of the values (0 for an
 * empty frame). Deterministic: per-block partials go to d_scratch and a second launch adds them in a fixed order; no
 * atomics, two calls give identical bits. *scratch_bytes: in, the size of d_scratch; out, the size needed. With
 * d_scratch == NULL the call only answers that size (d_raw, d_stats may be NULL then). d_stats [T] on the device.
 * *scratch_bytes is written whenever T, H, W, offset and clip_lower are valid, also by a call that is then refused
 * because the scratch is too small: that is how the caller learns the size. */
typedef struct {
    int64_t n;
    double sum, sumsq;
    float max, reserved;
} axt_frame_stats;
int axt_preprocess_stats_u16(const uint16_t *d_raw, const uint8_t *d_mask, int T, int H, int W, float offset,
                             float clip_lower, int log_correct, axt_frame_stats *d_stats, void *d_scratch,
                             size_t *scratch_bytes, void *stream);

/* axt_preprocess_u16 with one scale per frame (STANDARDIZE_FRAMEWISE, Timelapse.py:309-312): d_scale f32 [T] on the device,
 * each > 0 (the caller's promise: the values are not read back here). Bit-equal to axt_preprocess_u16 on each frame alone
 * with that frame's scale. */
int axt_preprocess_u16_framewise(const uint16_t *d_raw, const uint8_t *d_mask, int T, int H, int W, float offset,
                                 float clip_lower, int log_correct, const float *d_scale, float *d_out, void *stream);

/* ------------------------------------------------------------------------------------------
 * Tiling: which 512x512 tiles the reference keeps (Timelapse.py:551-558): a tile is kept if
 * any pixel of it is > 0 at any t. d_occ u8 [ceil(H/512)*ceil(W/512)] row-major, 1 = keep.
 * 1 <= T_all <= 65539 (the frames after the fourth are one launch's second grid dimension).
 * ------------------------------------------------------------------------------------------ */
int axt_tile_occupancy(const float *d_frames, int T_all, int H, int W, uint8_t *d_occ, void *stream);

/* ------------------------------------------------------------------------------------------
 * YOLO grid -> frame detections. Replaces, per frame,
 *   _yolo_Y2pandas_det  (AxonDetections.py:178-248)  decode, round-half-even, conf >= thr
 *   stitch_tiles        (Timelapse.py:166-197)       + tile origin
 *   _non_max_supression (AxonDetections.py:250-278)  greedy, dx^2+dy^2 < min_dist^2 dies
 * d_yolo f32 [n_frames, n_tiles, 12,12,3]; h_tile_yx i32 [n_tiles,2] (tile row, tile col).
 * Outputs, capacity cap >= n_tiles*144 per frame: d_conf f32, d_x i32, d_y i32 [n_frames,cap]
 * in descending confidence (ties: tile order, then cell order), d_count i32 [n_frames].
 * n_tiles <= 256; frames of up to 28 kept tiles keep their candidates in LDS, larger ones in a workspace in HBM
 * (allocated on the stream for the call): same order, same result.
 * Bounds: 1 <= n_tiles <= 256; tile indices 0 .. 32767 (the kernels keep them as short), otherwise free: any rows and
 * columns in any order; cap >= n_tiles * 144 and n_frames * cap <= 2^31 - 1; 0 <= min_dist <= 32767; conf_thr any number,
 * +-inf included, NaN: AXT_EINVAL. n_frames == 0: AXT_OK, nothing is touched; negative: AXT_EINVAL. The NMS distance is exact
 * for any two stitched coordinates (differences in 64 bits).
 * ------------------------------------------------------------------------------------------ */
int axt_decode_stitch_nms(const float *d_yolo, int n_frames, int n_tiles, const int32_t *h_tile_yx,
                          float conf_thr, int min_dist, int cap,
                          float *d_conf, int32_t *d_x, int32_t *d_y, int32_t *d_count, void *stream);

/* ------------------------------------------------------------------------------------------
 * Association costs.
 * ------------------------------------------------------------------------------------------ */
/* observation_model (mincostflow_models.py:6-27) after the confidence capping of
 * AxonDetections.py:655-659. method 0 = 'scale_to_max' (conf / max over all frames),
 * 1 = 'ceil' (min(conf,1)). d_cost f64 [n_frames,cap] (entries >= count are untouched). cap >= 1, max_conf_cost finite.
 * n_frames == 0: AXT_OK, nothing is touched; negative: AXT_EINVAL. */
int axt_obs_costs(const float *d_conf, const int32_t *d_count, int n_frames, int cap,
                  int method, double max_conf_cost, double *d_cost, void *stream);

/* A masked grid: the reference's weight image {1 on mask, 65536 off} (AxonDetections.py:587-598) in the forms the
 * kernels need -- byte mask, bit-packed rows and connected-component labels (4- or 8-connected, flood fill on the
 * host). Built once per timelapse from a HOST mask u8 [H,W] (1 = on mask). Synchronous. */
typedef struct axt_grid axt_grid;
int axt_grid_create(const uint8_t *h_mask, int H, int W, int conn8, axt_grid **out);
void axt_grid_destroy(axt_grid *grid);

/* _compute_detections_astar_paths + _get_astar_path_distances for ONE frame pair
 * (AxonDetections.py:526-629,717-752; A* call utils.py:379): D[i,j] = number of cells on the
 * minimum-cost 4-connected (conn8: 8-connected) path from detection i of the earlier frame
 * (rows) to detection j of the later frame on weights {1 on mask, 65536 off}; max_dist where
 * the euclidean distance is >= max_dist, an end point is outside the grid, or the path has
 * more than max_dist cells. grid = NULL for an all-ones mask (closed form); with a grid its
 * connectivity must equal conn8 (exact single-source search per detection of the earlier frame) and its size H x W.
 * D i32 [na, nb] row-major. na, nb >= 0 (either 0: AXT_OK, nothing is touched) and na * nb <= 2^31 - 1;
 * 1 <= max_dist <= 32767. */
int axt_path_cost(const int32_t *d_xa, const int32_t *d_ya, int na,
                  const int32_t *d_xb, const int32_t *d_yb, int nb,
                  const axt_grid *grid, int H, int W, int max_dist, int conn8,
                  int32_t *d_D, void *stream);

/* The paths themselves (the coo matrices _compute_astar_path returns, utils.py:379-387; kept by
 * _compute_detections_astar_paths, AxonDetections.py:570-577, for the cache file and for drawing): D as above, and
 * d_cells i32 [na, nb, max_dist] receives, for every pair with D < max_dist, the D cells of one minimum-cost path
 * as y*W + x, source first; other entries are left untouched. Needs a grid (all-ones masks have closed-form
 * staircases); which of several equally cheap paths pyastar2d would return is not pinned. Bounds as axt_path_cost. */
int axt_path_cells(const int32_t *d_xa, const int32_t *d_ya, int na,
                   const int32_t *d_xb, const int32_t *d_yb, int nb,
                   const axt_grid *grid, int H, int W, int max_dist, int conn8,
                   int32_t *d_D, int32_t *d_cells, void *stream);

/* All admissible transition arcs of a timelapse in one pass (what transition_model,
 * mincostflow_models.py:67-119, and the tracker's cost_threshold keep): for every detection
 * a of frame t and b of frame t+g (g = 1..max_gap) with D(a,b) <= h_dmax[g-1], one arc a->b.
 * Detections are numbered globally in frame order (frame offsets = prefix sum of counts).
 * CSR by tail: d_row_ptr i64 [n_det+1] (allocate n_frames*cap+1); d_col i32 [n_arcs] (global
 * index of b), d_len i16 [n_arcs] (D), d_gap u8 [n_arcs]. Rows are sorted by (gap, b):
 * deterministic. d_work i32 [n_frames*cap*max_gap + n_frames + 1 + max_gap + 4] (plus, with a masked grid,
 * n_frames*cap*max_gap*cap/2 for the i16 path-length table) is scratch that
 * must stay untouched between the two phases:
 *   phase 1: d_col == NULL -> counts, row_ptr, *n_arcs (synchronises the stream);
 *   phase 2: d_col/d_len/d_gap sized by *n_arcs -> filled (asynchronous).
 * Optional integer arc costs: d_cost_units i64 [max_gap, max_dist+1] holds round(cost*1e6) of
 * transition_model for every (gap, D); d_cost i64 [n_arcs] then receives
 * axt_arc_cost_int-compatible values (units << 16 | hash16(3, a, b)). Both NULL to skip.
 * grid = NULL: all-ones mask, closed-form path lengths. With a grid the minimum-cost paths are ordered by (off-mask
 * cells entered, moves); the grid holds, per connected component of the mask, the fewest off-mask cells to every cell.
 * A detection on the mask gets all its path lengths from one bit-parallel breadth-first search (depth h_dmax-1 <= 250
 * moves) over the steps that keep that count minimal; a detection off the mask from a label-correcting search on
 * (off-mask cells, moves) inside the window paths of <= dmax cells cannot leave, checked against the same counts
 * (masks with more than 64 components: on-mask search within the component + the exact search of axt_path_cost).
 * Optional inputs, each a nullable pointer:
 *   d_src_count (i32 [n_frames]) -- NULL: every row. Otherwise rows are built only for the first d_src_count[t] detections
 *     of frame t: a rank of a frame-sharded run (one process per GPU after the all-gather of the detections, SURVEY.md
 *     section 8e) passes its own frames' counts and zeros elsewhere, while targets, numbering and integer costs stay those
 *     of the whole timelapse (d_count), so that the ranks' arc lists, concatenated in rank order, are exactly the
 *     single-process list. row_ptr covers all detections; rows outside the source frames are empty.
 *   d_len_table (i16 [n_frames, cap, max_gap, cap]) -- NULL: the path lengths are computed. Otherwise entry [t][i][g-1][j] =
 *     number of cells of the path between detection i of frame t and detection j of frame t+g, <= 0 = none; grid, H, W
 *     and conn8 are not read. This is how path lengths cached by the reference ('{name}_astar_dets_paths.pkl': coo
 *     matrices, length = getnnz(), AxonDetections.py:717-752) re-enter the pipeline. d_x / d_y are not read for lengths
 *     but must be valid [n_frames, cap] arrays.
 *   d_hist, d_hist_sum (axt_box_histograms below) with vis_weight in (0,1], miss_rate, edge_cost_thr -- d_hist NULL: costs
 *     from d_cost_units, the three numbers are not read. Otherwise the appearance term: the cost is computed per pair,
 *     d_cost_units is ignored and d_cost may be NULL. With d_len_table this is the combination the reference's parameter
 *     search runs (assign_ids(astar_paths_cache='from') with MCF_VIS_SIM_WEIGHT > 0, AxonDetections.py:882,911-912).
 *     miss_rate finite and >= 0; edge_cost_thr any number, +-inf included, NaN: AXT_EINVAL.
 * Bounds: n_frames >= 1, cap >= 1, 1 <= max_gap <= 8, n_frames * cap * max_gap <= 2^31 - 1 (computed in size_t);
 * 1 <= max_dist <= 32767; H, W as everywhere (not read with d_len_table), a grid must be H x W; 0 <= h_dmax[g] <= 32767.
 * Where the path lengths come from a table (d_len_table, or a grid) and d_cost_units prices them, additionally
 * h_dmax[g] <= max_dist: a length can reach h_dmax[g] and indexes the units table, which has max_dist + 1 entries per gap.
 * The closed form never exceeds max_dist and accepts any h_dmax[g] in range. A refused call leaves *n_arcs as it was. */
int axt_build_arcs(const int32_t *d_x, const int32_t *d_y, const int32_t *d_count, const int32_t *d_src_count,
                   int n_frames, int cap, const axt_grid *grid, int H, int W, int max_dist, int conn8,
                   int max_gap, const int32_t *h_dmax,
                   const float *d_hist, const double *d_hist_sum, double vis_weight, double miss_rate,
                   double edge_cost_thr,
                   int64_t *d_row_ptr, int32_t *d_work, int32_t *d_col, int16_t *d_len, uint8_t *d_gap,
                   const int64_t *d_cost_units, int64_t *d_cost, int64_t *n_arcs,
                   const int16_t *d_len_table, void *stream);

/* ------------------------------------------------------------------------------------------
 * Appearance term of the transition cost, MCF_VIS_SIM_WEIGHT > 0.
 *
 * axt_box_histograms = feature_model (axtrack/mincostflow_models.py:30-65): for every detection the
 * 180-bin histogram on [0,1) of the box x box crop of frame (f + t_offset) of d_frames -- the centre frame
 * of detection frame f, which is what the tracker is shown (AxonDetections.py:682-685) -- min-max
 * normalised. The crop starts at (max(y - box/2, 0), max(x - box/2, 0)) and is clipped at the far edges.
 * d_hist f32 [n_frames, cap, 180], d_hist_sum f64 [n_frames, cap] (bin sums, used by the distance).
 * Bounds: T_all >= 1, t_offset >= 0 and t_offset + n_frames <= T_all; 1 <= n_frames <= 65535 (the launch's second grid
 * dimension), cap >= 1, 1 <= box <= 32768.
 *
 * axt_build_arcs with d_hist = these histograms computes the cost of transition_model (:100-118) per pair:
 *   cost = -log((1-w) * (1 - D/max_dist) * miss_rate^(gap-1) + w * (1 - d_B(hist_a, hist_b)) + 1e-6)
 * d_B = cv2.compareHist(.., HISTCMP_BHATTACHARYYA); an arc is kept iff cost < edge_cost_thr, and
 * d_cost (may be NULL) receives round(cost * 1e6) << 16 | hash16(3, a, b). h_dmax[g-1] only bounds the
 * candidates: pass the largest D whose cost with similarity 1 is still below the threshold.
 * cv2 is absent from the reference tree: parity unpinned.
 * ------------------------------------------------------------------------------------------ */
int axt_box_histograms(const float *d_frames, int T_all, int H, int W, int t_offset, const int32_t *d_x,
                       const int32_t *d_y, const int32_t *d_count, int n_frames, int cap, int box,
                       float *d_hist, double *d_hist_sum, void *stream);

/* ------------------------------------------------------------------------------------------
 * Global data association. Replaces libmot's MinCostFlowTracker as driven by
 * AxonDetections.py:663-690 (process() per frame, then compute_trajectories()).
 * HOST function (exact successive-shortest-path min-cost flow on the unit-capacity tracking
 * network; the solve is serial by nature -- DESIGN.md).
 *   n_det detections numbered globally; per detection: integer observation cost;
 *   entry/exit arcs cost h_entry[k], h_exit[k]; transition arcs in CSR (row_ptr, col, cost).
 *   min_flow/max_flow: bounds on the number of trajectories (MCF_MIN_FLOW / MCF_MAX_FLOW).
 * Outputs: h_next i32 [n_det]: successor detection on the same trajectory or -1;
 *          h_track i32 [n_det]: trajectory id (numbered by first detection) or -1;
 *          *n_tracks, *total_cost.
 * Returns AXT_INFEASIBLE if fewer than min_flow trajectories can be routed (the reference's
 * falsy compute_trajectories(), AxonDetections.py:691-696). n_det >= 0, 0 <= min_flow <= max_flow; every arc must point
 * forward (k < h_col[e] < n_det), else AXT_EINVAL.
 * ------------------------------------------------------------------------------------------ */
int axt_mcf_solve(int n_det, const int64_t *h_obs, const int64_t *h_entry, const int64_t *h_exit,
                  const int64_t *h_row_ptr, const int32_t *h_col, const int64_t *h_cost,
                  int min_flow, int max_flow,
                  int32_t *h_next, int32_t *h_track, int *n_tracks, int64_t *total_cost);

/* axt_mcf_solve plus an optimality certificate (what a caller of the reference's tracker cannot get: libmot returns
 * trajectories only, AxonDetections.py:690). Node potentials of the optimum, pi(S) = 0: h_pot_u[k] = pi(u_k), h_pot_v[k] = pi(v_k)
 * (i64 [n_det] each), *pot_t = pi(T). With the reduced cost rc(x -> y) = cost + pi(x) - pi(y) of the arcs S -> u_k (entry),
 * u_k -> v_k (observation), v_k -> T (exit), v_a -> u_b (transition) and T -> S (cost 0, between min_flow and max_flow units):
 * rc >= 0 on every arc without flow, rc <= 0 on every arc that carries its unit, and for T -> S: pi(T) >= 0 unless the flow
 * count sits at max_flow, pi(T) <= 0 unless it sits at min_flow. Together with a feasible flow (node-disjoint paths) these are
 * the complementary-slackness conditions of the flow LP: checking them over all arcs -- O(arcs), no second solve -- proves that
 * the returned trajectories are a minimum (tests/helpers.py: check_flow_certificate). Not written when AXT_INFEASIBLE. */
int axt_mcf_solve_duals(int n_det, const int64_t *h_obs, const int64_t *h_entry, const int64_t *h_exit,
                        const int64_t *h_row_ptr, const int32_t *h_col, const int64_t *h_cost,
                        int min_flow, int max_flow,
                        int32_t *h_next, int32_t *h_track, int *n_tracks, int64_t *total_cost,
                        int64_t *h_pot_u, int64_t *h_pot_v, int64_t *pot_t);

/* The same solve shared between frame-sharded ranks (one process per GPU; AxonDetections.py:663-690 has one process). Every
 * rank holds the whole network (the detections are all-gathered, the arcs rebuilt or gathered: DESIGN.md section 7) and calls
 *   axt_mcf_shard_begin   -- sets the solver up and solves THIS rank's run of time blocks (1/world of the leaves of the
 *                            time-block tree, on the rank's host threads); *state_bytes = size of the state to exchange;
 *   axt_mcf_shard_export  -- writes that state (duals and matching of the rank's rows and columns) to h_state;
 *   [one all-gather of the states between the ranks: torch.distributed, RCCL or gloo -- not this library's business]
 *   axt_mcf_shard_finish  -- h_states[r] / h_state_bytes[r] = rank r's state (the own entry is ignored): joins the runs
 *                            through the separator rows between them, runs the second phase, and returns exactly what
 *                            axt_mcf_solve returns (the optimum is unique: every rank ends with the same trajectories);
 *   axt_mcf_shard_free.
 * world must be a power of two. The network arrays must stay valid from begin to finish. Host only. */
typedef struct axt_mcf_shard axt_mcf_shard;
int axt_mcf_shard_begin(int n_det, const int64_t *h_obs, const int64_t *h_entry, const int64_t *h_exit,
                        const int64_t *h_row_ptr, const int32_t *h_col, const int64_t *h_cost, int rank, int world,
                        axt_mcf_shard **out, int64_t *state_bytes);
int axt_mcf_shard_export(const axt_mcf_shard *shard, void *h_state);
int axt_mcf_shard_finish(axt_mcf_shard *shard, const void *const *h_states, const int64_t *h_state_bytes, int min_flow,
                         int max_flow, int32_t *h_next, int32_t *h_track, int *n_tracks, int64_t *total_cost);
/* axt_mcf_shard_finish with the certificate of axt_mcf_solve_duals */
int axt_mcf_shard_finish_duals(axt_mcf_shard *shard, const void *const *h_states, const int64_t *h_state_bytes, int min_flow,
                               int max_flow, int32_t *h_next, int32_t *h_track, int *n_tracks, int64_t *total_cost,
                               int64_t *h_pot_u, int64_t *h_pot_v, int64_t *pot_t);
void axt_mcf_shard_free(axt_mcf_shard *shard);

/* ------------------------------------------------------------------------------------------
 * Frame-to-frame Hungarian association (BASELINE config 3; a build-side variant -- the reference
 * only runs the global tracker above, AxonDetections.py:663-690). Same cost model: linking a (frame t)
 * to b (frame t+g) costs transition_model(D(a,b), g) (mincostflow_models.py:67-119) and is admitted for D <= h_dmax[g-1]; leaving a detection
 * without successor costs thr_units (= round(MCF_EDGE_COST_THR * 1e6)). Every frame pair
 * (t,t+1) is solved exactly and independently (one wavefront each), then (t,t+2) among the
 * detections left unlinked, then chains are numbered by (first frame, index). Asynchronous.
 *
 * axt_hungarian_pairs solves the frame pairs of the source frames [t_begin, t_end) into d_pred = pred1 | pred2 (i32
 * [2, n_frames*cap], predecessor index in frame t-1 / t-2 or -1; entries of other frames stay -1). A frame-sharded rank
 * passes its own range, and the ranks combine d_pred with one element-wise MAX all-reduce. max_gap is 1 or 2, cap at most
 * 2048; d_cost_units i64 [max_gap, max_dist+1]; d_work i32 [2*n_frames*cap + n_frames + 1] scratch.
 * Bounds: n_frames >= 1, n_frames * cap <= 2^30 - 1, 0 <= t_begin <= t_end <= n_frames, 0 <= thr_units <= 2^46 (a dummy
 * cost is thr_units << 16 | hash in i64). Without d_ctab: H, W as everywhere, a grid must be H x W,
 * 1 <= max_dist <= 32767, 0 <= h_dmax[g] <= 32767, and with a grid h_dmax[g] <= max_dist (the kernels stage the
 * max_dist + 1 units of a gap in LDS and a searched length can reach h_dmax[g]; the closed form never exceeds max_dist and
 * accepts any h_dmax[g] in range). The LDS bounds cap and max_dist together: 66 cap + 48 cap (cap <= 576) + 8 max_dist + 32
 * <= 163840 bytes.
 * Optional inputs, each a nullable pointer:
 *   grid -- NULL: all-ones mask, closed-form path lengths. Otherwise the path lengths of the pairs come from the
 *     masked-grid searches of the arc builder (_compute_detections_astar_paths on weights {1 on mask, 65536 off},
 *     AxonDetections.py:526-629).
 *   d_ctab (i64 [n_frames][cap][max_gap][cap]) -- NULL: costs from the path lengths and d_cost_units. Otherwise the link
 *     costs are GIVEN: entry (t, i, g-1, j) = the integer cost (axt_arc_cost_int, kind 3, global detection indices) of
 *     linking detection i of frame t to detection j of frame t+g, or 0x3fffffffffffffff where the link is not admitted;
 *     grid, H, W, max_dist, conn8, h_dmax and d_cost_units are not read and may be NULL or 0. For cost models the closed
 *     form does not cover -- the appearance term of transition_model (mincostflow_models.py:107-113,
 *     MCF_VIS_SIM_WEIGHT > 0): the costs of axt_build_arcs with d_hist scattered into the table.
 *
 * axt_chain_tracks numbers the chains of d_pred (after the all-reduce in sharded runs): d_track i32 [n_frames, cap] =
 * trajectory id of every detection slot (-1 beyond count), d_n_tracks i32 [1]; d_work i32 [2*n_frames*cap] scratch.
 * n_frames >= 1, cap >= 1, n_frames * cap <= 2^30 - 1.
 * ------------------------------------------------------------------------------------------ */
int axt_hungarian_pairs(const int32_t *d_x, const int32_t *d_y, const int32_t *d_count, int n_frames, int cap,
                        const axt_grid *grid, int H, int W, int max_dist, int conn8, int max_gap,
                        const int32_t *h_dmax, const int64_t *d_cost_units, int64_t thr_units,
                        int t_begin, int t_end, int32_t *d_pred, int32_t *d_work, void *stream,
                        const int64_t *d_ctab);
int axt_chain_tracks(const int32_t *d_count, int n_frames, int cap, const int32_t *d_pred, int32_t *d_work,
                     int32_t *d_track, int32_t *d_n_tracks, void *stream);

/* ------------------------------------------------------------------------------------------
 * IDed_dets_all (AxonDetections._agg_all_IDed_dets, AxonDetections.py:825-842) as a dense f64
 * table [n_rows, 3*n_frames] on the device: columns 3*slot(f)+{0,1,2} = anchor_x, anchor_y, conf of
 * the detection of frame f that carries the row's identity, NaN elsewhere. slot(f) = f, or with
 * label_quirk != 0 the rank of f among the frames that have an IDed detection (the reference's
 * concat drops the others, :831, and labels the rest by position).
 * d_track i32 [n_frames, cap] (-1 = no identity), d_id_row: NULL (row = id, n_rows == n_ids) or
 * i32 [n_ids] id -> row (-1 = drop); d_work i32 [n_frames] scratch. Asynchronous.
 * n_frames >= 1, cap >= 1, n_ids >= 0, n_rows >= 0 (n_rows == 0: AXT_OK, nothing is touched);
 * n_frames * cap <= 2^31 - 1 and n_rows * n_frames <= 2^31 - 1.
 * ------------------------------------------------------------------------------------------ */
int axt_ided_table(const int32_t *d_track, const float *d_conf, const int32_t *d_x, const int32_t *d_y,
                   const int32_t *d_count, int n_frames, int cap, int n_ids, const int32_t *d_id_row, int n_rows,
                   int label_quirk, int32_t *d_work, double *d_table, void *stream);

/* ------------------------------------------------------------------------------------------
 * Axon reconstructions (AxonDetections._reconstruct_axons / get_axon_reconstructions, stubs at
 * AxonDetections.py:924-934; read by video_plotting.py:164-168,301-304). recon.hip.
 * ------------------------------------------------------------------------------------------ */
/* The links of the tracks: for every detection slot (f, i) of d_track i32 [n_frames, cap] (-1 = none) with id k, the
 * first detection of k in frames f+1 .. f+max_gap (max_gap = MCF_MAX_NUM_MISSES + 1). d_links i32 [n_frames*cap, 3]
 * receives (tail slot f*cap+i, head slot, gap) of each link in ascending tail order (deterministic);
 * d_work i32 [2*n_frames*cap + 2*n_frames + 1]; *n_links = number of links. Synchronises the stream.
 * n_frames >= 0 (n_frames == 0: AXT_OK and *n_links = 0), cap >= 1, n_frames * cap <= 2^30 - 1, 1 <= max_gap <= 255. A
 * refused call leaves *n_links as it was. */
int axt_track_links(const int32_t *d_track, const int32_t *d_count, int n_frames, int cap, int max_gap,
                    int32_t *d_links, int32_t *d_work, int64_t *n_links, void *stream);

/* One minimum-cost path per link (d_links as axt_track_links writes them; d_x / d_y i32 [n_frames, cap]): exactly the
 * cells, in the same order, that the package returns for that pair -- grid == NULL: the closed-form staircase of
 * AxonDetections.astar_dets_paths (4-connected: columns first, then rows; 8-connected: the diagonal first, then
 * straight); with a grid: what axt_path_cells gives for that (source, target) pair (windowed searches in LDS, the exact
 * search for what they cannot decide). Only the links whose HEAD frame f has d_head_group[f] == group (all links for
 * d_head_group == NULL): one call per distinct mask of a time-varying mask. d_len i32 [n_links] (zeroed before the first
 * call) receives the number of cells, max_dist = no path; d_stage i32 [n_links, max_dist] the cells y*W + x, source
 * first. Reads back one count (links for the exact search) when grid != NULL. n_links >= 0 (0: AXT_OK, nothing is
 * touched), cap >= 1, 2 <= max_dist <= 32767, a grid must be H x W. */
int axt_link_paths(const axt_grid *grid, const int32_t *d_x, const int32_t *d_y, int cap, const int32_t *d_links,
                   int n_links, const int32_t *d_head_group, int group, int H, int W, int max_dist, int conn8,
                   int32_t *d_len, int32_t *d_stage, void *stream);

/* The paths of axt_link_paths as CSR. Phase 1 (d_cells == NULL): d_cell_ptr i64 [n_links+1] = prefix sum of the lengths
 * (0 for no path), *n_cells = total (synchronises). Phase 2: d_cells i32 [n_cells] filled from d_stage, and
 * d_interp i32 [n_links, max_gap-1]: for a link of gap g >= 2 with a path of L cells, entry k-1 (k = 1 .. g-1) = the
 * cell at index (2k(L-1) + g) / (2g) of the path (the interpolated anchor of frame tail+k), -1 otherwise.
 * n_links >= 0, 2 <= max_dist <= 32767, 1 <= max_gap <= 255. A refused call leaves *n_cells as it was. */
int axt_link_cells(const int32_t *d_links, int n_links, const int32_t *d_len, const int32_t *d_stage, int max_dist,
                   int max_gap, int64_t *d_cell_ptr, int32_t *d_cells, int32_t *d_interp, int64_t *n_cells, void *stream);

/* ------------------------------------------------------------------------------------------
 * Target screens: every growth cone's distance and path to a target through the structure -- the "StructureScreen" the
 * reference's drawing code reads and never shipped (video_plotting.py:170-177,308-309: get_trg_path(t, ymin, ymax),
 * structure_outputchannel_coo). target.hip, DESIGN.md 6.8c.
 * ------------------------------------------------------------------------------------------ */
/* The field of a set of target cells over the whole grid: for every cell c the key (off, moves) of the minimum-cost
 * 4-connected (conn8: 8-connected) path from c to any target cell on the weights {1 on mask, 65536 off} of
 * AxonDetections.py:598 -- off = off-mask cells entered, moves = steps, ordered lexicographically as in axt_path_cost
 * (for one target cell moves + 1 is what axt_path_cost returns wherever its gate lets it answer); (0, 0) on the targets.
 * d_target_cells i32 [n_targets] = y*W + x on the device (entries outside the grid are ignored), n_targets >= 1;
 * grid = NULL: all-ones mask (the same kernel). d_off / d_moves i32 [H, W]. Tiled label-correcting search, one launch per
 * round over the tiles whose halo improved (axt_target_tile_size: the tile edge); the host reads a counter back every few
 * rounds and returns AXT_ERUNTIME beyond n_tiles * 4 * tile rounds. Scratch (8 bytes per cell) is allocated on the
 * stream. *n_rounds (may be NULL) = rounds that had work. The result is the unique fixed point: byte-identical from run
 * to run. Synchronises the stream. */
int axt_target_tile_size(void);
int axt_target_field(const axt_grid *grid, int H, int W, int conn8, const int32_t *d_target_cells, int n_targets,
                     int32_t *d_off, int32_t *d_moves, int *n_rounds, void *stream);

/* The field at every detection slot: d_det_off / d_det_moves i32 [n_frames, cap] = (off, moves) at (d_y, d_x) of the
 * slot, -1 for slots >= d_count[f] and for detections outside the grid (the decode does not clamp). d_off / d_moves i32
 * [n_fields, H, W]; d_field_index i32 [n_frames] = the field of frame f (one per distinct mask of a time-varying mask;
 * NULL with n_fields == 1; an index outside [0, n_fields) gives -1). Asynchronous. n_fields >= 1, cap >= 1,
 * n_frames >= 0 (n_frames == 0: AXT_OK, nothing is touched), n_frames * cap <= 2^31 - 1. */
int axt_target_sample(const int32_t *d_off, const int32_t *d_moves, int n_fields, const int32_t *d_field_index, int H,
                      int W, const int32_t *d_x, const int32_t *d_y, const int32_t *d_count, int n_frames, int cap,
                      int32_t *d_det_off, int32_t *d_det_moves, void *stream);

/* The target paths of the detection slots as CSR, in the shape of axt_link_cells. The path of a detection starts at its
 * cell; every step goes to the first neighbour n (up, down, left, right, then the diagonals in axt_path_cells' order)
 * with key(c) == key(n) + (mask[n] ? 0 : 1, 1); it has moves + 1 cells and ends in a target cell.
 * Phase 1 (d_cells == NULL): d_cell_ptr i64 [n_frames*cap + 1] = prefix sum of d_det_moves + 1 (0 where it is -1),
 * *n_cells = total (synchronises). Phase 2: d_cells i32 [*n_cells] receives y*W + x, detection first, for the slots
 * whose frame f has d_field_index[f] == group (all slots for d_field_index == NULL) from the ONE field d_off / d_moves
 * i32 [H, W] and its grid (NULL = all ones): one call per distinct mask. One thread per detection. Asynchronous.
 * n_frames >= 0, cap >= 1, n_frames * cap <= 2^31 - 1. A refused call leaves *n_cells as it was. */
int axt_target_paths(const axt_grid *grid, const int32_t *d_off, const int32_t *d_moves, int H, int W, int conn8,
                     const int32_t *d_x, const int32_t *d_y, int n_frames, int cap, const int32_t *d_det_moves,
                     const int32_t *d_field_index, int group, int64_t *d_cell_ptr, int32_t *d_cells, int64_t *n_cells,
                     void *stream);

/* ------------------------------------------------------------------------------------------
 * Mask preparation: the microchannel mask from a transmission image, which the reference makes by hand in a notebook
 * with napari and scikit-image (data_prep_nbs/00_segment_bg.ipynb). segment.hip, DESIGN.md 6.8d, where every stage is
 * defined in terms of SciPy and numpy. Image sizes: H, W > 0 and H * W <= 2^31 - 1.
 * ------------------------------------------------------------------------------------------ */
/* segment_microchannels, `filters.prewitt(transm_chnl)` and `filters.gaussian(prewitt, sigma=gaussion_sigma)`, in one
 * launch. d_img u16 [H, W]. d_P f32 [H, W] = sqrt((gy^2 + gx^2) / 2), gy / gx = the 3 x 3 Prewitt differences along
 * the rows / columns divided by 3, the image continued by reflection (d c b a | a b c d); the 3 x 3 sums are exact.
 * d_G f32 [H, W] = d_P smoothed by the separable Gaussian of 2 radius + 1 taps, radius = int(4 sigma + 0.5), weights
 * exp(-x^2 / 2 sigma^2) normalised in f64 and rounded to f32, d_P continued by its nearest edge value.
 * d_minmax f32 [2] = min(d_G), max(d_G), exact (integer atomics on the bit patterns of values >= 0).
 * sigma > 0, radius <= 16 and min(H, W) >= 2 radius + 2, else AXT_EINVAL. Asynchronous. */
int axt_segment_edges(const uint16_t *d_img, int H, int W, double sigma, float *d_P, float *d_G, float *d_minmax,
                      void *stream);

/* The histogram `threshold_otsu(prewitt_gaussian)` starts from (segment_microchannels): d_hist i64 [256] = the counts
 * np.histogram(d_G, 256, range=(mn, mx)) gives for the n values of d_G taken as f64: v falls into bin i with
 * e_i <= v < e_i+1, the last bin closed, e_i = mn + i (mx - mn) / 256 in f64 and e_256 = mx; values outside [mn, mx]
 * are not counted. mn == mx: everything equal to mn falls into bin 0. Integer counts: identical from run to run. The
 * threshold itself is 256 numbers of host arithmetic (axtrack_amd.segment.otsu_threshold_from_hist). 1 <= n <= 2^31 - 1,
 * mn <= mx finite, else AXT_EINVAL. Asynchronous. */
int axt_segment_histogram(const float *d_G, int64_t n, double mn, double mx, int64_t *d_hist, void *stream);

/* `prewitt_bin = prewitt > threshold` and `morphology.binary_closing(prewitt_bin, morphology.square(bin_closing_dim))`
 * (segment_microchannels): d_out u8 [H, W] (0 / 1) = the erosion of the dilation of (f64)d_P > thr by k x k ones. With
 * a = k / 2 and b = k - 1 - a per axis: dilation = OR over [y - b, y + a], 0 outside the image; erosion = AND over
 * [y - a, y + b], 1 outside (scipy.ndimage.binary_erosion(binary_dilation(B, ones), ones, border_value=1)). The image
 * is bit-packed between the steps; scratch (H * ceil(W / 64) * 16 bytes) is allocated on the stream. 2 <= k <= 32 and
 * thr a number, else AXT_EINVAL. Asynchronous. */
int axt_segment_close(const float *d_P, int H, int W, double thr, int k, uint8_t *d_out, void *stream);

/* flood_initial_mask, `flood(filled_mask, floodpoint)`: d_out u8 [H, W] = 1 on the cells connected to the seed
 * (seed_y, seed_x) through cells with the seed's value of d_img u8 [H, W] (zero / non-zero; the seed may sit on either),
 * 4-connected or (conn8) 8-connected: lab == lab[seed] for lab = scipy.ndimage.label(img == img[seed], structure).
 * Tiled reachability search on bit planes, one launch per round over the tiles whose halo grew (axt_segment_tile_size:
 * the tile edge); the host reads a counter back every few rounds and returns AXT_ERUNTIME beyond n_tiles * 4 * tile
 * rounds. Scratch (H * ceil(W / 64) * 16 bytes) is allocated on the stream. *rounds_out (may be NULL) = rounds that had
 * work. The result is the unique fixed point: byte-identical from run to run. A seed outside the image: AXT_EINVAL.
 * Synchronises the stream. */
int axt_segment_tile_size(void);
int axt_segment_flood(const uint8_t *d_img, int H, int W, int seed_y, int seed_x, int conn8, uint8_t *d_out,
                      int *rounds_out, void *stream);

/* ------------------------------------------------------------------------------------------
 * Detection metrics: compute_TP_FP_FN (AxonDetections.py:409-466) for every frame
 * and every confidence threshold. Detections as axt_decode_stitch_nms leaves them; labels d_gx, d_gy
 * i32 [n_frames, gcap], d_gcount i32 [n_frames]; d_thrs f64 [n_thr] on the device (the reference's
 * all_conf_thrs, :76); min_dist = NON_MAX_SUPRESSION_DIST. d_confusion i32 [n_frames, 3, n_thr]:
 * TP, FP, FN. Labels are matched in order; a label whose closest candidate is already claimed is a
 * false negative; an empty side is replaced by one phantom row at the origin with conf 0 (:434-437).
 * k_mask >= 0: additionally d_fp_mask u8 [n_frames, cap] / d_fn_mask u8 [n_frames, gcap] for that
 * threshold index (either may be NULL); any k_mask < 0 means no masks, k_mask >= n_thr: AXT_EINVAL. Asynchronous.
 * n_frames >= 1, 1 <= cap <= 2048, gcap >= 1, 1 <= n_thr <= 65535 (the launch's second grid dimension), 0 <= min_dist <= 1024.
 * ------------------------------------------------------------------------------------------ */
int axt_detection_confusion(const float *d_conf, const int32_t *d_x, const int32_t *d_y, const int32_t *d_count,
                            int n_frames, int cap, const int32_t *d_gx, const int32_t *d_gy, const int32_t *d_gcount,
                            int gcap, const double *d_thrs, int n_thr, int min_dist, int k_mask,
                            int32_t *d_confusion, uint8_t *d_fp_mask, uint8_t *d_fn_mask, void *stream);

/* ------------------------------------------------------------------------------------------
 * Tracking scores (the definition stands in csrc/mot.hip): the counts behind the MOTChallenge
 * metrics of axtrack_amd/mot_metrics.py for n_assoc associations of the same detections at once.
 * d_track i32 [n_assoc, n_frames, cap] (-1 = no identity; identities in [0, nh)); d_x, d_y, d_count the shared
 * detections; labels d_gid (dense identities in [0, no)), d_gx, d_gy i32 [n_frames, gcap], d_gcount i32 [n_frames].
 * Identities are unique within a frame on both sides; identities out of range take no part. The counts are clamped:
 * a frame uses max(min(d_count[f], cap), 0) detection slots and max(min(d_gcount[f], gcap), 0) label slots. A pair is admissible
 * when dx^2 + dy^2 <= max_dist^2. Limits: cap, gcap <= 1024, max_dist <= 255, no, nh <= 2^24 (AXT_EINVAL beyond);
 * 1 <= n_assoc <= 65535, n_frames >= 1, all of cap, gcap, no, nh >= 1, max_dist >= 0.
 * Outputs: d_counts i64 [n_assoc, 10] = n_match, n_switch, n_miss, n_fp, sum of matched d2, n_obj, n_pred,
 * n_unique_objects, n_fragmentations, idtp; d_tallies i32 [n_assoc, no, 2] = frames present, frames not missed.
 * Event log (each pointer may be NULL): d_ev_kind u8 [n_assoc, n_frames, gcap] per label slot (0 none, 1 MATCH,
 * 2 SWITCH, 3 MISS), d_ev_partner i32, same shape (the partner's detection slot, -1 = none), d_ev_fp u8
 * [n_assoc, n_frames, cap] per detection slot. *scratch_bytes: in, the size of d_scratch; out, the size needed;
 * with d_scratch == NULL the call only answers that size (the other pointers may be NULL then); it is written whenever the
 * sizes are valid, also by a call that is then refused because the scratch is too small. Integer work,
 * two calls give identical bits. Asynchronous.
 * ------------------------------------------------------------------------------------------ */
int axt_mot_scores(const int32_t *d_track, int n_assoc, const int32_t *d_x, const int32_t *d_y, const int32_t *d_count,
                   int n_frames, int cap, const int32_t *d_gid, const int32_t *d_gx, const int32_t *d_gy,
                   const int32_t *d_gcount, int gcap, int no, int nh, int max_dist, int64_t *d_counts,
                   int32_t *d_tallies, uint8_t *d_ev_kind, int32_t *d_ev_partner, uint8_t *d_ev_fp, void *d_scratch,
                   size_t *scratch_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Rendering (video_plotting.py draw_all / setup_frame_drawing / draw_frame / draw_detections, which redraw every
 * frame as matplotlib patches): annotated uint8 RGB frames, DESIGN.md 6.8b.
 * axt_render_tile_size: edge of the square output tiles the primitive lists are binned by (64).
 * axt_render_frames: d_out u8 [n_out, Ho, Wo, 3] = the slice [ymin, ymin+Ho) x [xmin, xmin+Wo) of the detection frames
 * d_ts i32 [n_out] (ascending). d_frames: f32 [.., H, W], detection frame t at d_frames + t*H*W (the caller skips the
 * context frames). Background (R8, 0, 0), R8 = rint(clamp(v, 0, 1) * 255); bg != 0: brightened with the weight map
 * blurred over the whole frame and the mask of frame t (d_mask + t*mask_stride, u8; NULL = all ones); grid > 0: the
 * lines x % grid == 0 or y % grid == 0 (frame coordinates) blended with white. Trails: d_trail i32 [n, 4] (frame,
 * key, x, y in output coordinates; binned per output tile, d_trail_ptr i32 [n_tiles+1], sorted by frame within a
 * tile): the cells with frame <= the output frame's, 5 x 5 squares, the largest key wins, colour
 * palette[d_trail_col[key]]. Primitives: d_prims i32 [m, 8] (x0, y0, kind, a, b, key, 0, 0: kind 0 dashed box
 * outline a x a, 1 solid ground-truth outline, 2 glyph a = char - 32 at scale b, 3 rectangle a x b, 4 rectangle a x b of the target layer that lies between the
 * grid and the trails: key 1 = a target path, (217, 217, 217), key 2 = target cells, white, over the paths) binned per
 * (output frame, tile): d_prim_ptr i32 [n_out*n_tiles+1]; key = layer << 24 | (n + 1), the largest key wins, layer 3
 * is grey (107). d_tables u8: palette [20, 3], then the glyph rows [95, 7]. Asynchronous.
 * Bounds: Ho, Wo >= 1, ymin, xmin >= 0, ymin + Ho <= H and xmin + Wo <= W (checked without overflow); grid >= 0,
 * mask_stride >= 0; n_out * tiles < 2^31 - 1. n_out == 0: AXT_OK, nothing is touched; negative: AXT_EINVAL. */
int axt_render_tile_size(void);
int axt_render_frames(const float *d_frames, const uint8_t *d_mask, int64_t mask_stride, const int32_t *d_ts, int n_out,
                      int H, int W, int ymin, int xmin, int Ho, int Wo, int grid, int bg, const int32_t *d_trail_ptr,
                      const int32_t *d_trail, const uint8_t *d_trail_col, const int32_t *d_prim_ptr,
                      const int32_t *d_prims, const uint8_t *d_tables, uint8_t *d_out, void *stream);

/* ------------------------------------------------------------------------------------------
 * Fine-tuning of the linear head fcs.1/3/5 on labelled frames with the convolutional trunk frozen
 * (core_functionality.py:81-165, loss.py:18-68, Timelapse.py:451-548), DESIGN.md 6.8e.
 *
 * axt_yolo_targets: labels -> YOLO targets (Timelapse.construct_tiles :513-548 + tiled_target2yolo_format :451-490 for
 * the kept tiles). d_lx, d_ly i32 [F, cap] whole-frame pixel anchors, d_lcount i32 [F]; negative coordinates mean "no
 * label". d_target f32 [F, n_tiles, 12, 12, 4]: dim 2 the x cell, dim 3 the y cell, last (1, x_in_cell, y_in_cell,
 * label index), every other cell zero. A label belongs to tile (ty, tx) iff ty*512 <= y < (ty+1)*512 and likewise x;
 * labels of tiles that are not listed are dropped. Cell arithmetic in f32 as the reference's (bit-equal); of two labels
 * in a cell the one with the higher index wins all four channels (one thread per cell scans the labels: no race).
 * F >= 0 (F == 0 writes nothing), cap >= 1, 1 <= n_tiles <= 256, tile indices 0 .. 32766, F * n_tiles * 144 < 2^39.
 *
 * axt_head_trainer: device-resident master weights ([out,in] row-major f32, state_dict layout), Adam moments m, v (f32,
 * zero), the step count and the activations of the last forward batch. NOUT = 432, max_batch <= 64.
 * _forward: d_index i32 [B] (NULL = rows 0..B-1) picks rows of the feature table d_feat [., K0];
 *   d_yolo [B, NOUT] = (sigma(sigma(X W1^T + b1) W2^T + b2)) W3^T + b3 (model.py:105-117). Split-K, slabs summed in a
 *   fixed order.
 * _loss: YOLO_AXTrack_loss.forward on d_yolo [B,432] and rows d_index of the target table d_target [., 12,12,4];
 *   h_components f64 [5] (NULL: not read back, no synchronisation): total_no_object_loss, total_object_loss,
 *   total_xy_anchors_loss, total_summed_loss, total_pos_labels_rate, accumulated in f64 in a fixed tree; d_dy f32
 *   [B,432] (NULL: none) its gradient with respect to d_yolo. Synchronises the stream when h_components is given.
 * _step: backward pass from d_dy through the activations _forward stashed for this batch (same B), all of it from
 *   the weights as they stand, then for every weight matrix one kernel that forms g = sum_b dZ[b,n] In[b,k] +
 *   weight_decay w in ascending b without storing it and updates m, v, w in place as torch.optim.Adam does
 *   (t = the handle's step count after its increment). Biases likewise. No atomics: byte-identical from run to run.
 * _read_weights / _read_moments (layer 0..2; any pointer may be NULL): device -> host, synchronous.
 * K0, H1, H2 >= 1; 1 <= B <= max_batch in every call that takes a batch. Adam: 0 <= beta1, beta2 < 1, eps >= 0,
 * weight_decay >= 0, else AXT_EINVAL; lr and the three lambdas are taken as they are (any value, not checked).
 * ------------------------------------------------------------------------------------------ */
int axt_yolo_targets(const int32_t *d_lx, const int32_t *d_ly, const int32_t *d_lcount, int F, int cap,
                     const int32_t *h_tile_yx, int n_tiles, float *d_target, void *stream);
typedef struct axt_head_trainer axt_head_trainer;
int axt_head_trainer_create(int K0, int H1, int H2, int NOUT, const float *h_w1, const float *h_b1, const float *h_w2,
                            const float *h_b2, const float *h_w3, const float *h_b3, int max_batch,
                            axt_head_trainer **out);
void axt_head_trainer_destroy(axt_head_trainer *tr);
size_t axt_head_trainer_device_bytes(const axt_head_trainer *tr);
int axt_head_trainer_read_weights(const axt_head_trainer *tr, float *h_w1, float *h_b1, float *h_w2, float *h_b2,
                                  float *h_w3, float *h_b3);
int axt_head_trainer_read_moments(const axt_head_trainer *tr, int layer, float *h_mw, float *h_vw, float *h_mb,
                                  float *h_vb, int64_t *step);
int axt_head_trainer_forward(axt_head_trainer *tr, const float *d_feat, const int32_t *d_index, int B, float *d_yolo,
                             void *stream);
int axt_head_trainer_loss(axt_head_trainer *tr, const float *d_yolo, const float *d_target, const int32_t *d_index, int B,
                          double lambda_obj, double lambda_noobj, double lambda_coord, double *h_components, float *d_dy,
                          void *stream);
int axt_head_trainer_step(axt_head_trainer *tr, const float *d_feat, const int32_t *d_index, int B, const float *d_dy,
                          double lr, double beta1, double beta2, double eps, double weight_decay, void *stream);

/* ------------------------------------------------------------------------------------------
 * Fine-tuning of the last convolutional block together with the head.
 *
 * axt_head_trainer_input_grad: the gradient of the loss with respect to the rows _forward read. From d_dy [B, NOUT], the
 *   a1, a2 stashed by the last _forward (same B) and the weights as they stand: dZ2 = (dY W3) * a2 (1 - a2),
 *   dZ1 = (dZ2 W2) * a1 (1 - a1), d_dfeat [B, K0] = dZ1 W1. Same kernels and fixed slab order as _step, no atomics.
 *   Works in scratch of its own, allocated by the first call (_device_bytes grows then): calling it before _step leaves
 *   _step's results byte-identical.
 *
 * axt_conv_trainer: one block Conv2d(Ci, Co, 3, padding 1) + BatchNorm2d + LeakyReLU(0.1) (model.py:5-18) in training
 * form. Created from host tensors in the state dict's layout: conv.weight [Co,Ci,3,3], conv.bias, batchnorm.weight,
 * batchnorm.bias, batchnorm.running_mean, batchnorm.running_var [Co]. Holds the four trainable tensors with Adam
 * moments m, v (f32, zero), the step count, and z of the last forward batch. Limits: 1 <= Ci, Co <= 512,
 * 1 <= H, W <= 64, 1 <= max_batch <= 64. By default BatchNorm runs with its running statistics, as at inference
 * (eps 1e-5), and leaves them alone; with batch statistics switched on (axtrack_hip_stage.h: _set_batch_stats) it
 * normalises every batch with that batch's own statistics and moves the running ones, as nn.BatchNorm2d does in train
 * mode. The handle keeps running_mean and running_var either way (_read_stats).
 * _forward: d_index i32 [B] (NULL = rows 0..B-1) picks rows of the table d_in [., Ci*H*W] (NCHW per row);
 *   z = conv3x3(x) + bias, y = gamma (z - mean) / sqrt(var + 1e-5) + beta, d_feat [B, Co*H*W] = y > 0 ? y : 0.1 y in the
 *   order c*H*W + h*W + w -- the rows axt_head_trainer_forward reads. f32, BatchNorm not folded; per output FMA chains
 *   of 16 terms in ascending (ci, ky, kx), their sums added in ascending order.
 * _step: d_dfeat [B, Co*H*W] is the gradient with respect to _forward's output for the same batch (same d_in, d_index,
 *   B). dy = dF * (y > 0 ? 1 : 0.1), dgamma = sum dy zhat, dbeta = sum dy, dz = dy gamma / sqrt(var + 1e-5),
 *   dbias = sum dz, dW[co,ci,ky,kx] = sum_{b,h,w} dz[b,co,h,w] x[b,ci,h+ky-1,w+kx-1] (taps outside the map contribute
 *   nothing), all from the parameters as they stand, then torch.optim.Adam with L2 weight decay on the four tensors
 *   (t = the handle's step count after its increment). Sums run over b, h, w ascending within a fixed split that
 *   depends on the sizes and B only, the parts added in ascending order. No atomics: byte-identical from run to run.
 * _read_weights; _read_moments (tensor 0..3: conv.weight, conv.bias, batchnorm.weight, batchnorm.bias; any pointer may
 *   be NULL): device -> host, synchronous.
 * ------------------------------------------------------------------------------------------ */
int axt_head_trainer_input_grad(axt_head_trainer *tr, const float *d_dy, int B, float *d_dfeat, void *stream);
typedef struct axt_conv_trainer axt_conv_trainer;
int axt_conv_trainer_create(int Ci, int Co, int H, int W, const float *h_weight, const float *h_bias, const float *h_gamma,
                            const float *h_beta, const float *h_mean, const float *h_var, int max_batch,
                            axt_conv_trainer **out);
void axt_conv_trainer_destroy(axt_conv_trainer *tr);
size_t axt_conv_trainer_device_bytes(const axt_conv_trainer *tr);
int axt_conv_trainer_read_weights(const axt_conv_trainer *tr, float *h_weight, float *h_bias, float *h_gamma, float *h_beta);
int axt_conv_trainer_read_moments(const axt_conv_trainer *tr, int tensor, float *h_m, float *h_v, int64_t *step);
int axt_conv_trainer_forward(axt_conv_trainer *tr, const float *d_in, const int32_t *d_index, int B, float *d_feat,
                             void *stream);
int axt_conv_trainer_step(axt_conv_trainer *tr, const float *d_in, const int32_t *d_index, int B, const float *d_dfeat,
                          double lr, double beta1, double beta2, double eps, double weight_decay, void *stream);

/* Fine-tuning of the whole last conv stage (conv blocks 5, 6, the max-pool, conv block 7) with the head: the conv trainer's
 * input gradient, and the 2 x 2 max-pool with its gradient. Declared in a header of their own, part of this interface. */
#include "axtrack_hip_stage.h"

/* Fine-tuning of every conv block: a conv trainer with a stride of 1 or 2 on larger maps, the batch gather of the raw
 * 5-frame tile stacks, and block = 2 of axt_cnn_block_features_frames. Declared in a header of their own, part of this
 * interface. */
#include "axtrack_hip_trunk.h"

/* Weights into a live detector on the device: one conv block or one linear layer from device tensors, and the trainers'
 * exports of what they hold. Declared in a header of their own, part of this interface. */
#include "axtrack_hip_repack.h"

/* TIFF strips (LZW, PackBits, uncompressed; byte swap, horizontal predictor) into the raw uint16 timelapse that
 * axt_preprocess_u16 reads. Declared in a header of its own, part of this interface. */
#include "axtrack_hip_tiff.h"

/* uint8 RGB frames, as axt_render_frames writes them, into baseline JPEG scan segments: the frames of the MJPEG video
 * (DESIGN.md 6.8i). Declared in a header of its own, part of this interface. */
#include "axtrack_hip_jpeg.h"

/* Training augmentation of a whole timelapse in one launch (data_utils.transform_X: translate, then flip, then rotate;
 * DESIGN.md 6.8e). d_in f32 [T, H, W]; d_out the same shape, not overlapping d_in (AXT_EINVAL: the warp is a gather).
 * Output pixel (y, x) of every frame reads the source that the inverses give in reverse order:
 *   rotate != 0: torchvision's TF.rotate(img, angle) for tensors (nearest, no expand, fill 0) = grid_sample(nearest, zeros,
 *     align_corners=False) on _gen_affine_grid of _get_inverse_affine_matrix([0,0], -angle, [0,0], 1, [0,0]). m00 m01 /
 *     m10 m11 are that matrix's entries (cos r, sin r / -sin r, cos r with r = radians(-angle)) rounded to f32 by the
 *     caller. All in f32: base coordinates x - W/2 + 0.5 and y - H/2 + 0.5, the entries divided by 0.5 W (first row) and
 *     0.5 H (second row), two rounded products and their rounded sum, ((g + 1) * size - 1) / 2, round half to even; a
 *     source outside the frame gives 0;
 *   flip_y / flip_x: H-1-y / W-1-x;
 *   dy, dx (any sign and size): subtracted; a source outside the frame gives 0.
 * d_occ (may be NULL) u8 [T, ceil(H/512) * ceil(W/512)]: zeroed by the call, then 1 where the OUTPUT frame has a pixel
 * > 0 in that tile (partial edge tiles count). No atomics: byte-identical from run to run. Asynchronous.
 * axt_augment_frame_chunk: the frames one workgroup loops over with the source indices it computed once.
 * 1 <= T <= 393210 and 1 <= H <= 262140 (one launch: 65535 grid rows of 4 image rows, 65535 chunks of 6 frames), W >= 1;
 * m00 .. m11 finite when rotate != 0 (not read otherwise). */
int axt_augment_frame_chunk(void);
int axt_augment_frames(const float *d_in, int T, int H, int W, int dy, int dx, int flip_y, int flip_x, int rotate,
                       float m00, float m01, float m10, float m11, float *d_out, uint8_t *d_occ, void *stream);

/* Integer arc cost used by the flow network (the costs libmot hands its solver at AxonDetections.py:663-690, from
 * observation_model / transition_model, mincostflow_models.py:6-27,67-119): round(cost * 1e6) << 16 | hash16(kind, a, b).
 * kind 0 entry, 1 exit, 2 observation, 3 transition. The low 16 bits make the optimum unique
 * (DESIGN.md "Unpinned third-party semantics"). Pure arithmetic without an error return: any cost, kind, a and b give a value
 * (a NaN or a cost beyond +-9.2e12 gives an unspecified one). */
int64_t axt_arc_cost_int(double cost, int kind, int64_t a, int64_t b);

#ifdef __cplusplus
}
#endif
#endif
