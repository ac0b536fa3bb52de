/*
 * pp_hip.h -- C ABI of the MI355X-native PointPillars hot path (libpp_hip.so).
 *
 * The reference (mr3543/3d-Object-Detection) defines no C ABI of its own: its
 * only native surface is the pybind11 module of data/pillars.cpp:429-435 with
 * two functions, create_pillars (pillars.cpp:236-249) and make_ious
 * (pillars.cpp:400-404).  The entry points below are what a binding for that
 * path binds to -- plain pointers, sizes, BYTE strides and scalars, no torch or
 * numpy types.  Each one cites the reference interface it replaces.
 *
 * All functions return 0 on success or a negative PP_ERR_* code;
 * pp_last_error() returns a thread-local description of the last failure.
 * Nothing here ever falls back to a CPU implementation: without a HIP device
 * every compute entry point fails with PP_ERR_HIP.
 */
#ifndef PP_HIP_H
#define PP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PP_OK 0
#define PP_ERR_INDEX (-2)   /* reference: pybind11 index_error -> IndexError      */
#define PP_ERR_VALUE (-3)   /* invalid argument                                    */
#define PP_ERR_WINDING (-4) /* reference: "IOU < 0" -> std::exit(1), pillars.cpp:166-169 */
#define PP_ERR_NOMEM (-5)
#define PP_ERR_HIP (-6)     /* HIP runtime error / no device                       */
#define PP_ERR_INTERNAL (-7)

/* Pillar emission order.  The reference emits pillars in boost::unordered_map
 * iteration order (pillars.cpp:335), which is implementation-defined; these are
 * the deterministic replacements (DESIGN.md "pillar order"). */
#define PP_ORDER_ROW_MAJOR 0 /* ascending (canvas_y, canvas_x)        */
#define PP_ORDER_SCRAMBLED 1 /* ascending (cell * mult) mod ncells    */

#define PP_NUM_FEATURES 9 /* x,y,z,r,xp,yp,xc,yc,zc -- pillars.cpp:48-56 */
#define PP_MAX_BATCH 32

/* The scalar arguments of create_pillars, pillars.cpp:239-249, in its order. */
typedef struct pp_voxel_params {
  int32_t max_points_per_pillar; /* N */
  int32_t max_pillars;           /* P */
  double x_step, y_step;
  double x_min, y_min, z_min;
  double x_max, y_max, z_max;
  double canvas_height;
  int32_t order; /* PP_ORDER_*; not a reference argument (see above) */
  int32_t reserved;
} pp_voxel_params_t;

typedef struct pp_ctx pp_ctx_t; /* per-device, per-stream workspace owner */

const char *pp_last_error(void);
const char *pp_version(void);
int pp_device_count(void);

/* A context owns the scratch buffers (cell ids, counts, buckets).  Use one
 * context per HIP stream; calls on one context are serialised by that stream. */
int pp_ctx_create(int device, pp_ctx_t **out);
void pp_ctx_destroy(pp_ctx_t *ctx);

/* Pre-size the workspace so that later pp_voxelize_dev calls allocate nothing
 * (needed before HIP-graph capture). */
int pp_voxelize_reserve(pp_ctx_t *ctx, int batch, int64_t max_points,
                        const pp_voxel_params_t *prm);

/*
 * Device-resident voxelizer: replaces the whole voxel stage of
 * PPDataset.__getitem__ (data/dataset.py:88-106): np.zeros + create_pillars
 * (pillars.cpp:236-398) + transpose to [9,P,N] + f64->f32 + indices->int64.
 *
 *   points_dev   [batch][points_stride rows][4] f32 (x,y,z,r), device memory;
 *                sweep b uses its first n_points[b] rows (n_points is a HOST array)
 *   pillars_dev  [batch][9][P][N] f32, fully written (zero padded)
 *   indices_dev  [batch][P][3] int64 {1, canvas_x, canvas_y} / {0,0,0}
 *   num_cells_dev[batch][2] int32 or NULL: {non-empty cells (uncapped), in-range points}
 *   stream       hipStream_t (NULL = default stream)
 */
int pp_voxelize_dev(pp_ctx_t *ctx, void *stream, const float *points_dev,
                    int64_t points_stride, const int32_t *n_points, int batch,
                    const pp_voxel_params_t *prm, float *pillars_dev,
                    int64_t *indices_dev, int32_t *num_cells_dev);

/*
 * The same voxel stage, software-pipelined over consecutive batches -- what the reference gets from
 * DataLoader prefetching (train.py:120-121: the workers voxelize the next batches while the model
 * consumes the current one).  Inside one batch the three stages depend on each other (split ->
 * tile -> order -> emit); across batches they do not.  One call = ONE launch (k_step) whose workgroups
 * take roles side by side:
 *     the SPLIT stage of the batch handed in now            (points_dev),
 *     the TILE  stage of the batch handed in one call ago,
 *     the ORDER stage (descriptors into pillar order) of the batch handed in two calls ago,
 *     the EMIT  stage (the dense store) of the batch handed in THREE calls ago -> pillars_dev ...
 * The launch boundary is the only synchronisation; the latency-bound binning stages hide behind the
 * store.  Outputs are those of pp_voxelize_dev for the same input, bit for bit (the same code on the
 * same data; only the tile size differs, which the outputs do not depend on).
 *   points_dev    as pp_voxelize_dev's, or NULL (pipeline drain: three such calls flush it); read by
 *                 THIS call's launch only
 *   n_points, batch, prm   describe points_dev (ignored when it is NULL)
 *   pillars_dev, indices_dev, num_cells_dev   receive the batch handed in THREE calls ago, with that
 *                 call's batch / prm shapes; may be NULL while no batch is due
 *   emitted       (may be NULL) 1 when this call wrote outputs, else 0
 * Everything runs on `stream` -- the SAME stream for all calls of one pipeline (stream order is what
 * carries a batch from one stage to the next): a call on another stream while batches are in flight is
 * refused with PP_ERR_VALUE and changes nothing (drain first, or pp_voxelize_step_reset); plain calls on
 * the same context are unaffected (own workspace).
 * Workspace: the batches in flight rotate through four workspace slots of the context, each sized on first use and
 * again when a later batch needs more (pp_voxelize_reserve sizes the plain calls' workspace only).  A call that sizes
 * a slot allocates, and an allocation may wait for the device; after four batches of the largest shape no call does.
 * HIP graphs: a single call must NOT be captured and replayed -- the workspace slot of every stage
 * rotates from call to call on the host, and a replay would repeat one call's slots.  (The plain
 * pp_voxelize_dev is the capturable form.)
 */
int pp_voxelize_step_dev(pp_ctx_t *ctx, void *stream, const float *points_dev,
                         int64_t points_stride, const int32_t *n_points, int batch,
                         const pp_voxel_params_t *prm, float *pillars_dev,
                         int64_t *indices_dev, int32_t *num_cells_dev, int *emitted);

/*
 * The software-pipelined form of pp_voxelize_pfn_canvas_reuse_dev (PPFeatureNet.forward and
 * PPScatter.forward, model/model.py:31-62, inside the voxelizer): the SAME pipeline as pp_voxelize_step_dev --
 * split, tile and order roles unchanged, batches in flight are shared between the two entry points -- with
 * the EMIT role as the fused feature net: the batch handed in three calls ago comes out as its BEV canvas
 * instead of the dense [9,P,N] tensor.  One launch per call instead of three dependent ones.
 *   canvas_dev        [batch'][64][H][W] f32 (channels_last: memory [batch'][H][W][64]) for the batch that is
 *                     due (batch' = that call's batch).  It must be ALL ZERO on entry: only the pillars'
 *                     pixels are written.
 *   clear_canvas_dev, clear_indices_dev, clear_batch   (optional) ANOTHER canvas of the same shape whose
 *                     only non-zero pixels are those clear_indices_dev [clear_batch][P][3] names (the
 *                     indices this function returned when it filled that canvas): a CLEAR role of the
 *                     same launch zeroes them.  With two canvases used in turn -- emit into one, clear the
 *                     other, which the network has consumed in between -- no call waits for a clear
 *                     (pp_voxelize_pfn_canvas_reuse_dev clears and fills ONE canvas: a kernel boundary).
 *   pfn_params_dev, channels, canvas_h/w, channels_last, indices_dev, num_cells_dev: as
 *                     pp_voxelize_pfn_canvas_dev; points_dev / n_points / batch / prm / emitted / the stream
 *                     rule: as pp_voxelize_step_dev.
 * Results equal pp_voxelize_pfn_canvas_dev's for the same input bit for bit.
 */
int pp_voxelize_step_pfn_canvas_dev(pp_ctx_t *ctx, void *stream, const float *points_dev,
                                    int64_t points_stride, const int32_t *n_points, int batch,
                                    const pp_voxel_params_t *prm, const float *pfn_params_dev,
                                    int channels, float *canvas_dev, int canvas_h, int canvas_w,
                                    int channels_last, int64_t *indices_dev, int32_t *num_cells_dev,
                                    float *clear_canvas_dev, const int64_t *clear_indices_dev,
                                    int clear_batch, int *emitted);

/* The instance of k_step a pp_voxelize_step_dev call emits a batch of `batch` sweeps with, as a profiler's
 * kernel trace prints it ("pp::k_step<0, 16>": 16-byte stores, write-through; "<0, 0>": plain stores, beyond
 * 128 MB of dense output; "<1, 0>": N not a multiple of 4) -- bench.py names its roofline kernel with it. */
int pp_voxelize_step_kernel_name(const pp_voxel_params_t *prm, int batch, char *name, int cap);

/* Forgets the batches in flight in pp_voxelize_step_dev's pipeline (end of an epoch, an abandoned
 * stream): the next call starts an empty pipeline.  Nothing is launched. */
int pp_voxelize_step_reset(pp_ctx_t *ctx);

/*
 * The optional last step of the voxel stage (data/dataset.py:102-105): pillar -= data_mean,
 * the per-element dataset mean of the [9,P,N] tensor (pillar_means.pkl), f32 - f32 like the
 * reference, the same mean for every sweep.
 *   pillars_dev [batch][elems_per_sweep] f32 in place; mean_dev [elems_per_sweep] f32
 */
int pp_subtract_mean_dev(pp_ctx_t *ctx, void *stream, float *pillars_dev, int batch,
                         int64_t elems_per_sweep, const float *mean_dev);

/*
 * Device-resident voxelizer with the feature net fused in (inference only;
 * SURVEY 8f rank 1): replaces the voxel stage above AND PPFeatureNet.forward
 * (model/model.py:31-40: conv1x1 9->64, ReLU, then BatchNorm2d in eval mode,
 * max over the N slots, zero-padded slots included).  The dense [9,P,N] tensor
 * is never built.
 *   pfn_params_dev [64][12] f32 per output channel: conv weight w[0..8], conv
 *                  bias, BN scale gamma/sqrt(var+eps), BN shift beta-mean*scale
 *   features_dev   [batch][64][P] f32  == PPFeatureNet's output
 *   indices_dev, num_cells_dev, points_dev, n_points: as pp_voxelize_dev
 */
int pp_voxelize_pfn_dev(pp_ctx_t *ctx, void *stream, const float *points_dev,
                        int64_t points_stride, const int32_t *n_points, int batch,
                        const pp_voxel_params_t *prm, const float *pfn_params_dev,
                        int channels, float *features_dev, int64_t *indices_dev,
                        int32_t *num_cells_dev);

/*
 * PPFeatureNet.forward in eval mode (model/model.py:31-40) on the dense tensor the plain
 * voxelizer wrote -- for callers that keep the reference's [9,P,N] hand-over: the input is
 * read once and the [64,P,N] intermediate never exists.  Same arithmetic as
 * pp_voxelize_pfn_dev (bit-identical features).
 *   pillars_dev  [batch][9][P][N] f32      pfn_params_dev [64][12] f32 (as above)
 *   features_dev [batch][64][P] f32
 */
int pp_pfn_dense_dev(pp_ctx_t *ctx, void *stream, const float *pillars_dev, int batch,
                     int max_pillars, int max_points_per_pillar, const float *pfn_params_dev,
                     int channels, float *features_dev);

/*
 * PPScatter.forward (model/model.py:53-62) alone, for callers that already hold the feature
 * net's output: canvas[b,:,row,col] = features[b,:,p] for every flagged pillar
 * (indices[b,p] = {1, col, row}); the canvas is fully written (zeroed, then scattered).
 *   features_dev [batch][channels][P] f32, indices_dev [batch][P][3] int64
 *   canvas_dev   [batch][channels][H][W] f32, or [batch][H][W][channels] with channels_last
 */
int pp_scatter_canvas_dev(pp_ctx_t *ctx, void *stream, const float *features_dev,
                          const int64_t *indices_dev, int batch, int channels, int max_pillars,
                          float *canvas_dev, int canvas_h, int canvas_w, int channels_last);

/*
 * PPFeatureNet in TRAINING mode (BatchNorm with batch statistics) without the [64,P,N]
 * intermediate.  The forward needs the per-channel batch statistics of r = ReLU(conv(x)); the
 * backward needs, besides the gradient at each pillar's selected element, per-channel sums that
 * do not depend on the incoming gradient -- both come from ONE pass over the dense tensor:
 *   weight_bias_dev [64][10] f32 {w[0..8], bias}
 *   sums_dev        [21][64] f64: #{z>0}, sum (r-c0), sum (r-c0)^2 with c0 = max(bias,0) (the
 *                   value of a zero-padded slot: shifted sums, no cancellation in the
 *                   variance), S1[d] = sum_{z>0} x_d (9 rows), S2[d] = sum r*x_d (9 rows),
 *                   over all batch*P*N slots
 * The forward output is then pp_pfn_dense_dev with scale/shift from the batch statistics.
 * r is torch.relu's (z < 0 ? 0 : z): a NaN in the pillars makes rows 1 and 2 NaN in every
 * column, a NaN in a row of weight_bias_dev in that channel's column alone; c0 = max(bias, 0) is
 * taken of a parameter.  The caller keeps the running statistics of a channel whose derived mean
 * or variance is not finite, as pp_relu_bn_train_fwd_dev does.
 */
int pp_pfn_train_stats_dev(pp_ctx_t *ctx, void *stream, const float *pillars_dev, int batch,
                           int max_pillars, int max_points_per_pillar, const float *weight_bias_dev,
                           int channels, double *sums_dev);

/*
 * ... and the gradient-dependent part of the backward: per (b,c,p) the element the forward's
 * max selected is found again (same fmaf chain), and
 *   sums_dev [12][64] f64: dbeta = sum G, dgamma = sum G*xhat*, then the selected elements'
 *            contribution to db (1 row) and dW[d] (9 rows)
 *   pfn_params_dev [64][12] (the forward table: w, bias, scale, shift), mean_dev / invstd_dev [64]
 *   grad_out_dev [batch][64][P] f32
 * The caller combines: dW = sparse + A*S1 + B*S2, db = sparse + A*cnt + B*sum r with
 * A = scale*(-dbeta/M + mean*dgamma*invstd/M), B = -scale*dgamma*invstd/M, M = batch*P*N.
 */
int pp_pfn_train_backward_dev(pp_ctx_t *ctx, void *stream, const float *pillars_dev, int batch,
                              int max_pillars, int max_points_per_pillar,
                              const float *pfn_params_dev, const float *mean_dev,
                              const float *invstd_dev, const float *grad_out_dev, int channels,
                              double *sums_dev);

/*
 * The same, with PPScatter.forward fused in as well (model/model.py:53-62): the feature
 * vector of every flagged pillar goes straight to its pixel of the BEV canvas,
 * canvas[b, :, row, col] = features[b, :, p]; the [batch][64][P] tensor is never built.
 *   canvas_dev   f32, fully written (zeroed, then scattered): [batch][64][canvas_h][canvas_w]
 *                or, with channels_last != 0, [batch][canvas_h][canvas_w][64] (one 256-byte
 *                store per pillar; the layout MIOpen's NHWC convolutions take directly)
 *   canvas_h     must equal prm->canvas_height; a pillar whose pixel falls outside
 *                canvas_h x canvas_w is not written (PPScatter would raise there)
 */
int pp_voxelize_pfn_canvas_dev(pp_ctx_t *ctx, void *stream, const float *points_dev,
                               int64_t points_stride, const int32_t *n_points, int batch,
                               const pp_voxel_params_t *prm, const float *pfn_params_dev,
                               int channels, float *canvas_dev, int canvas_h, int canvas_w,
                               int channels_last, int64_t *indices_dev, int32_t *num_cells_dev);

/*
 * The same for a canvas that is handed back call after call (a persistent buffer, as PPScatter's
 * output is per step, model/model.py:53-62): `prev_indices_dev` are the indices the PREVIOUS call of
 * this function (or of pp_voxelize_pfn_canvas_dev) wrote for the SAME canvas_dev with the same batch and
 * prm -- the only pixels of it that are non-zero.  Instead of clearing the whole canvas (64 MB per
 * sweep at 500x500) only those pixels are zeroed (3 MB), by extra workgroups of the tile launch.
 * prev_indices_dev may alias indices_dev (it is read before indices_dev is written); NULL = the
 * canvas's contents are unknown: full clear, exactly pp_voxelize_pfn_canvas_dev.
 */
int pp_voxelize_pfn_canvas_reuse_dev(pp_ctx_t *ctx, void *stream, const float *points_dev,
                                     int64_t points_stride, const int32_t *n_points, int batch,
                                     const pp_voxel_params_t *prm, const float *pfn_params_dev,
                                     int channels, float *canvas_dev, int canvas_h, int canvas_w,
                                     int channels_last, int64_t *indices_dev, int32_t *num_cells_dev,
                                     const int64_t *prev_indices_dev);

/*
 * Host drop-in for create_pillars (pillars.cpp:236-249, exported :433).
 * points [n,>=4], tensor [P',N',>=9], indices [P',>=3]: f64 host arrays with
 * arbitrary BYTE strides, mutated in place; nothing is zeroed (pillars.cpp never
 * zeroes); out-of-range writes return PP_ERR_INDEX after the in-range part was
 * written (pybind11 .mutable_at semantics).  num_cells (may be NULL) receives
 * the number of non-empty cells.
 * Host side (one call at a time per context; the call returns with every
 * device operation finished): a pool of host threads gathers the points and
 * scatters the rows (PP_HOST_THREADS); a cloud whose every value is an f32
 * value crosses the link as f32, both ways where it applies; the context's
 * pinned staging buffers are read and written by the kernels themselves
 * (device-visible host memory; PP_DROPIN_DIRECT=0: copy engines instead).
 */
int pp_create_pillars_f64(pp_ctx_t *ctx, const void *points, int64_t n_points,
                          int64_t p_stride0, int64_t p_stride1, void *tensor,
                          const int64_t t_shape[3], const int64_t t_strides[3],
                          void *indices, const int64_t i_shape[2],
                          const int64_t i_strides[2],
                          const pp_voxel_params_t *prm, int64_t *num_cells);

/*
 * Host drop-in for make_ious (pillars.cpp:400-404, exported :432): gated
 * all-pairs rotated IoU; every ious[i][j] is written.  f64 host arrays, BYTE
 * strides.  a_corners [A,4,2], g_corners [G,4,2], a_centers [A,>=2],
 * g_centers [G,>=2], ious [A,G].
 * The anchors of the previous call stay on the device (80 bytes each, freed
 * with the context): every call compares the caller's anchor arrays bit for
 * bit with a pinned mirror and uploads them again only when something changed
 * (utils/box_utils.py:181-183 passes the same arrays for every sample).
 * Returns PP_ERR_WINDING for a box with the wrong corner order (the
 * reference: std::exit(1), pillars.cpp:166-169); the contents of ious are then
 * unspecified.
 */
int pp_make_ious_f64(pp_ctx_t *ctx, const void *a_corners, int64_t A,
                     const int64_t ac_strides[3], const void *g_corners,
                     int64_t G, const int64_t gc_strides[3],
                     const void *a_centers, const int64_t an_strides[2],
                     const void *g_centers, const int64_t gn_strides[2],
                     void *ious, const int64_t io_strides[2]);

/* Error flag of the IoU / target-assignment launches on this context since the
 * last check: synchronises `stream`, returns PP_ERR_WINDING (and clears the flag)
 * if a pair that passed the centre gate had a wrongly wound box (the reference's
 * "IOU < 0" exit, pillars.cpp:166-169), else PP_OK.  pp_make_ious_f64 calls it itself.
 * PP_ERR_VALUE: the box-centric target kernel's list of pairs above the threshold overflowed
 * (it is sized from the candidate anchors per box, so only boxes whose image-space centre is
 * not finite can get there); entries were dropped, the scratch is re-armed before the next call. */
int pp_iou_check(pp_ctx_t *ctx, void *stream);

/* Device-resident make_ious: contiguous f64 device arrays, ious_dev [A][G]. */
int pp_make_ious_dev(pp_ctx_t *ctx, void *stream, const double *a_corners_dev,
                     const double *a_centers_dev, int64_t a_center_cols,
                     int64_t A, const double *g_corners_dev,
                     const double *g_centers_dev, int64_t g_center_cols,
                     int64_t G, double *ious_dev);

/*
 * Device-resident fused target assignment: replaces create_target
 * (utils/box_utils.py:162-232) including make_ious (pillars.cpp:400-427) and
 * make_target (box_utils.py:70-109); the [A,G] IoU matrix is never
 * materialised.  All inputs contiguous f64 device arrays:
 *   a_corners [A,4,2] a_centers [A,3] a_wlh [A,3] a_yaw [A]          (anchors,
 *       image space, box_utils.py:111-159)
 *   g_corners [G,4,2] g_centers_img [G,3]  (boxes_to_image_space, :19-32)
 *   g_centers [G,3] g_wlh [G,3] g_yaw [G]  (canvas space Box fields)
 *   g_class [G] int32
 * Outputs f32 (data/dataset.py:117-118 casts to float):
 *   cls_targets [A,num_classes], reg_targets [A,9]
 * Limits (PP_ERR_VALUE beyond): 1 <= A <= 16 776 960 anchors, 0 <= G <= 65535, 1..1024 classes.
 * (Anchors on the fly are assigned from the box side while a sample's boxes x workgroups per box fit one grid
 * dimension -- about eleven thousand boxes at BASELINE configs[2] -- and from the anchor side beyond; the results are
 * the same either way.)
 */
typedef struct pp_target_params {
  double pos_thresh;    /* cfg.DATA.IOU_POS_THRESH, config.py:122 */
  double canvas_height; /* cfg.DATA.CANVAS_HEIGHT, config.py:60   */
  int32_t num_classes;  /* cfg.DATA.NUM_CLASSES, config.py:97     */
  int32_t reserved;
} pp_target_params_t;

int pp_assign_targets_dev(pp_ctx_t *ctx, void *stream, int64_t A,
                          const double *a_corners, const double *a_centers,
                          const double *a_wlh, const double *a_yaw, int64_t G,
                          const double *g_corners, const double *g_centers_img,
                          const double *g_centers, const double *g_wlh,
                          const double *g_yaw, const int32_t *g_class,
                          const pp_target_params_t *prm, float *cls_targets,
                          float *reg_targets);

/*
 * The same with the anchors evaluated on the fly instead of read from arrays (SURVEY 8f
 * rank 4: no anchor_boxes.pkl / anchor_xy.pkl, train_prep.py:115-120): the grid of
 * make_anchor_boxes (utils/box_utils.py:111-159) -- anchor i = (y*fm_width + x)*per_cell + d,
 * centre ((x+.5)/fm_scale, (y+.5)/fm_scale, z_d), size / yaw of type d.
 *   anchor_types_dev [per_cell][13] f64: the rotated bottom-corner offsets from the centre
 *                    x0,y0,..,x3,y3 (Box.bottom_corners order), then w, l, h, yaw, z
 * Results equal pp_assign_targets_dev on the uploaded arrays bit for bit.
 */
int pp_assign_targets_grid_dev(pp_ctx_t *ctx, void *stream, int fm_height, int fm_width,
                               double fm_scale, int per_cell, const double *anchor_types_dev,
                               int64_t G, const double *g_corners_dev,
                               const double *g_centers_img_dev, const double *g_centers_dev,
                               const double *g_wlh_dev, const double *g_yaw_dev,
                               const int32_t *g_class_dev, const pp_target_params_t *prm,
                               float *cls_targets_dev, float *reg_targets_dev);

/*
 * The target assignment of ALL samples of a step in one launch.  The reference prepares
 * BATCH_SIZE samples per step (config.py:135, train.py:120-121), each through create_target
 * (data/dataset.py:113-118, utils/box_utils.py:162-232); the kernel is a chain of latencies, not
 * bytes, so the samples' chains run side by side (grid.y = sample) instead of one after the other.
 *   batch      1..PP_MAX_BATCH samples; the anchors are shared by all of them
 *   g_counts   HOST array [batch]: sample b has g_counts[b] ground truths (0 allowed: its targets
 *              are all zero), 0..65535 each
 *   g_*        the samples' ground truths CONCATENATED in sample order: sample b owns rows
 *              [g_counts[0]+..+g_counts[b-1], ..+g_counts[b]) of every g_ array (device memory, layouts
 *              as pp_assign_targets_dev)
 *   cls_targets [batch][A][num_classes], reg_targets [batch][A][9] f32
 * Every sample's result equals what pp_assign_targets_dev / pp_assign_targets_grid_dev writes for
 * that sample alone, bit for bit (same code; the list, counter, ticket and column scratch the
 * last-workgroup tail depends on are per sample).
 */
int pp_assign_targets_batch_dev(pp_ctx_t *ctx, void *stream, int32_t batch, const int32_t *g_counts,
                                int64_t A, const double *a_corners, const double *a_centers,
                                const double *a_wlh, const double *a_yaw, const double *g_corners,
                                const double *g_centers_img, const double *g_centers,
                                const double *g_wlh, const double *g_yaw, const int32_t *g_class,
                                const pp_target_params_t *prm, float *cls_targets,
                                float *reg_targets);
int pp_assign_targets_grid_batch_dev(pp_ctx_t *ctx, void *stream, int32_t batch,
                                     const int32_t *g_counts, int fm_height, int fm_width,
                                     double fm_scale, int per_cell, const double *anchor_types_dev,
                                     const double *g_corners_dev, const double *g_centers_img_dev,
                                     const double *g_centers_dev, const double *g_wlh_dev,
                                     const double *g_yaw_dev, const int32_t *g_class_dev,
                                     const pp_target_params_t *prm, float *cls_targets_dev,
                                     float *reg_targets_dev);

/*
 * Lidar sweep ingest pre-pass: replaces, per sweep, the point
 * preparation of PPDataset.__getitem__ (data/dataset.py:65-82) --
 * LidarPointCloud.from_file rows (first four f32 columns of `raw_cols`),
 * .transform(transmat) in f64 stored as f32, .remove_close(min_dist) and the
 * hstack aggregation (write sweep s at points_out_dev + 4*offset_s).
 *   raw_dev        [n_points][raw_cols] f32 (the .bin file's rows), device memory
 *   transform      row-major 4x4 f64 HOST matrix (ref_car_from_global . global_from_car
 *                  . car_from_sensor, dataset.py:76)
 *   points_out_dev [n_points][4] f32; a removed point keeps its row with x = NaN,
 *                  which pp_voxelize_dev drops, so input order is preserved.
 */
int pp_ingest_dev(pp_ctx_t *ctx, void *stream, const float *raw_dev, int64_t n_points,
                  int raw_cols, const double *transform_rowmajor4x4, double min_dist,
                  float *points_out_dev);

/* All sweeps of a sample in one launch (dataset.py:65-82 loops over num_sweeps files and hstacks):
 * raw_dev[s] / n_points[s] / transforms_rowmajor4x4 + 16*s describe sweep s (HOST arrays of device
 * pointers, sizes, 4x4 f64 matrices); sweep s lands at points_out_dev + 4 * (n_points[0] + ... +
 * n_points[s-1]).  Same arithmetic as pp_ingest_dev.  1 <= n_sweeps <= PP_MAX_INGEST_SWEEPS. */
#define PP_MAX_INGEST_SWEEPS 16
int pp_ingest_sweeps_dev(pp_ctx_t *ctx, void *stream, int32_t n_sweeps, const float *const *raw_dev,
                         const int64_t *n_points, int raw_cols, const double *transforms_rowmajor4x4,
                         double min_dist, float *points_out_dev);

/*
 * Inference post-processing on the device: replaces the
 * per-sample tail of evaluate() (evaluate.py:231-245): sigmoid / tanh / class max /
 * score threshold / box_nms (:127-139, torchvision.ops.nms over the ANCHOR
 * rectangles) / first max_out survivors / make_pred_boxes (:33-89) /
 * move_box_to_car_space (:91-125).
 *   cls_dev [Ac*C][H][W] f32, reg_dev [Ac*8][H][W] f32: one sample of PPModel's output
 *   a_centers [A,3] a_wlh [A,3] a_yaw [A] a_xy [A,4]: anchors, f64 device arrays
 *       (box_utils.py:111-159; a_xy = the (x1,y1,x2,y2) rows of anchor_xy.pkl)
 *   boxes_out [max_out][9] f64: car-space x,y,z,w,l,h,yaw,score,class (zeros beyond count)
 *   kept_out  [max_out] int32 anchor ids in keep order (-1 beyond count); count_out [1]
 * Non-finite class logits (all pp_decode_*_dev): the score of an anchor is torch.max over its class
 * scores, which propagates NaN -- an anchor with a NaN score in ANY class has score NaN, is above no
 * pos_thresh and is never a candidate, whatever its other classes hold.  A logit of +inf gives the score
 * exactly 1.0f (as does every finite logit from about 17 up) and is a candidate like any other; -inf and
 * every logit whose sigmoid rounds to zero give the score 0, a candidate only for a negative pos_thresh.
 * Candidates are taken in decreasing score order, equal scores (bit for bit) by ascending anchor id; of
 * several classes with the same maximal score the lowest index is reported.
 */
typedef struct pp_decode_params {
  int32_t fm_height, fm_width, anchors_per_cell, num_classes;
  double pos_thresh;    /* cfg.DATA.VAL_POS_THRESH, config.py:153 */
  double nms_thresh;    /* cfg.DATA.VAL_NMS_THRESH, config.py:154 */
  int32_t max_out;      /* 100, evaluate.py:241 */
  int32_t reserved;
  double canvas_height, x_step, y_step, x_min, y_min; /* config.py:46-53,60 */
} pp_decode_params_t;

int pp_decode_dev(pp_ctx_t *ctx, void *stream, const float *cls_dev, const float *reg_dev,
                  const double *a_centers, const double *a_wlh, const double *a_yaw,
                  const double *a_xy, const pp_decode_params_t *prm, double *boxes_out,
                  int32_t *kept_out, int32_t *count_out);

/* The same on strided network outputs: element (channel ch, cell y*W+x) of cls / reg lives at
 * [ch*stride_c + cell*stride_pix] (in floats).  NCHW planes: (H*W, 1) -- what pp_decode_dev
 * passes; channels-last tensors or channel slices of one: (1, row pitch), where an anchor's
 * class logits and box offsets are contiguous. */
int pp_decode_strided_dev(pp_ctx_t *ctx, void *stream, const float *cls_dev, const float *reg_dev,
                          int64_t cls_stride_c, int64_t cls_stride_pix, int64_t reg_stride_c,
                          int64_t reg_stride_pix, const double *a_centers, const double *a_wlh,
                          const double *a_yaw, const double *a_xy, const pp_decode_params_t *prm,
                          double *boxes_out, int32_t *kept_out, int32_t *count_out);

/* A batch of samples in one call (evaluate.py:231-245 loops over the samples of a batch; here every
 * sample gets its own workgroups of the three kernels and they run side by side): sample b of cls /
 * reg starts b*stride_b floats after sample 0; boxes_out [batch][max_out][9], kept_out
 * [batch][max_out], count_out [batch].  1 <= batch <= 1024. */
int pp_decode_batch_dev(pp_ctx_t *ctx, void *stream, int32_t batch, const float *cls_dev,
                        const float *reg_dev, int64_t cls_stride_b, int64_t cls_stride_c,
                        int64_t cls_stride_pix, int64_t reg_stride_b, int64_t reg_stride_c,
                        int64_t reg_stride_pix, const double *a_centers, const double *a_wlh,
                        const double *a_yaw, const double *a_xy, const pp_decode_params_t *prm,
                        double *boxes_out, int32_t *kept_out, int32_t *count_out);

/* pp_decode_batch_dev with a choice of the suppression rule.  Candidates (score > pos_thresh), their
 * order (decreasing score, ties by ascending anchor id), the greedy pass, the max_out cap and the
 * outputs are pp_decode_batch_dev's; nms_mode picks what "overlap" means:
 *   PP_NMS_ANCHOR_RECT  box_nms (evaluate.py:127-139): f32 IoU of the ANCHOR rectangles a_xy.  With
 *       class_aware 0 this is pp_decode_batch_dev, bit for bit.
 *   PP_NMS_ROTATED_BEV  NOT in the reference: the f64 bird's-eye-view IoU of the DECODED boxes -- the
 *       very rows x,y,z,w,l,h,yaw written to boxes_out (every candidate is decoded by the code that
 *       writes them).  Footprint as in pp_box3d_iou_dev: centre (x,y), length l along yaw, width w
 *       across it, corners counter-clockwise.  inter = the kept box's footprint clipped by the four
 *       edges of the candidate's (f64 Sutherland-Hodgman, inside = cross product >= 0), shoelace area;
 *       iou = inter / (w_a l_a + w_b l_b - inter).  iou is 0 -- the box is never suppressed and
 *       suppresses nothing -- when either box has a non-finite x, y, w, l or yaw or w*l not > 0
 *       (checked before any clipping), or when the union is not finite and > 0.  Pairs whose
 *       footprints are disjoint by a conservative test (circumscribed circles apart, or a separating
 *       edge direction, each comparison with a relative slack of 1e-9) are not clipped: iou 0.
 *       A candidate is dropped iff iou(kept, candidate) > (double)(float)nms_thresh (strict) for an
 *       already kept box.  a_xy is not read and may be NULL.  nms_thresh must be finite and >= 0.
 *   class_aware 1 (either mode, not in the reference): a kept box only suppresses candidates with the
 *       same argmax class.
 * PP_ERR_VALUE for any other nms_mode or class_aware; limits otherwise as pp_decode_batch_dev. */
#define PP_NMS_ANCHOR_RECT 0 /* box_nms, evaluate.py:127-139: what pp_decode_*_dev do */
#define PP_NMS_ROTATED_BEV 1 /* BEV IoU of the decoded boxes (not in the reference)   */
int pp_decode_nms_batch_dev(pp_ctx_t *ctx, void *stream, int32_t batch, const float *cls_dev,
                            const float *reg_dev, int64_t cls_stride_b, int64_t cls_stride_c,
                            int64_t cls_stride_pix, int64_t reg_stride_b, int64_t reg_stride_c,
                            int64_t reg_stride_pix, const double *a_centers, const double *a_wlh,
                            const double *a_yaw, const double *a_xy, const pp_decode_params_t *prm,
                            int32_t nms_mode, int32_t class_aware, double *boxes_out, int32_t *kept_out,
                            int32_t *count_out);

/*
 * Fused conv epilogue for the inference backbone: y = max(x + b_c, 0) * s_c + t_c in
 * place on a contiguous NCHW f32 tensor -- the ReLU -> BatchNorm2d(eval) tail (plus the
 * conv bias) of every block of model/model.py:76-84,105-109 in one pass.
 *   x_dev [batch][channels][hw] f32; params_dev [channels][3] f32 {bias, scale, shift}
 *   y_dev NULL: in place.  Otherwise the result goes to channels
 *   [y_channel_offset, y_channel_offset+channels) of y_dev [batch][y_channels][hw] -- the
 *   up blocks write straight into the concatenated backbone output (model/model.py:140).
 */
int pp_bias_relu_bn_dev(pp_ctx_t *ctx, void *stream, float *x_dev, int64_t batch, int channels,
                        int64_t hw, const float *params_dev, float *y_dev, int64_t y_channels,
                        int64_t y_channel_offset);

/* The same epilogue on a channels-last tensor: x_dev [pixels][channels] f32 (pixels =
 * batch*h*w), channels a multiple of 4; the result goes in place (y_dev NULL) or to
 * channels [y_channel_offset, +channels) of y_dev [pixels][y_channels]. */
int pp_bias_relu_bn_nhwc_dev(pp_ctx_t *ctx, void *stream, float *x_dev, int64_t pixels, int channels,
                             const float *params_dev, float *y_dev, int64_t y_channels,
                             int64_t y_channel_offset);

/*
 * A 3x3, stride-1, padding-1 convolution of NHWC f32 x[batch][height][width][in_channels] with
 * the same epilogue as pp_bias_relu_bn_nhwc_dev (inference):
 *   y = max(conv(x) + bias_c, 0) * scale_c + shift_c,   params_dev [out_channels][3]
 * as Winograd F(2x2,3x3) on f32 MFMA.  u_dev is the transformed filter U = G g G^T in the
 * layout [16][in_channels/8][2][out_channels][4]: U[4i+j][ci][co] (i, j = 0..3) at
 * ((((4i+j)*(in_channels/8) + ci/8)*2 + (ci/4)%2)*out_channels + co)*4 + ci%4.
 * y_dev: channels [y_channel_offset, +out_channels) of rows of y_channels floats per pixel, each
 * written exactly once (no zero fill; other channels untouched).  in_channels a multiple of 8,
 * out_channels a multiple of 64, x and u 16-byte aligned.  Launches only: no allocation, no
 * synchronisation (graph-capturable); deterministic.
 */
int pp_conv3x3_wino_nhwc_dev(pp_ctx_t *ctx, void *stream, const float *x_dev, int batch, int height,
                             int width, int in_channels, const float *u_dev, int out_channels,
                             const float *params_dev, float *y_dev, int64_t y_channels,
                             int64_t y_channel_offset);

/*
 * The same layer as pp_conv3x3_wino_nhwc_dev -- a 3x3, stride-1, padding-1 convolution of NHWC f32
 * x[batch][height][width][in_channels] with the epilogue
 *   y = max(conv(x) + bias_c, 0) * scale_c + shift_c,   params_dev [out_channels][3] f32
 * -- with fp16 operands: the opt-in "fp16 inference" mode.  Activations are f32 in memory on both
 * sides.  Arithmetic:
 *   - Each x value and each weight is rounded once to IEEE binary16, round to nearest even (not the
 *     round-toward-zero pkrtz conversion).  x is rounded by the kernel; w_f16_dev holds the weights
 *     already rounded (torch.Tensor.half()).
 *   - Values beyond the fp16 range become +-inf, as torch.Tensor.half() makes them.  The caller opts
 *     in; the layer inputs here are BatchNorm outputs.
 *   - fp16-subnormal values are kept by both conversions (neither flushes); the products are formed
 *     by the matrix unit from the operands as stored, and what it makes of subnormal operands is not
 *     part of this contract: it moves a result by less than 1e-6 * sum|w||x|.
 *   - Products are accumulated in f32 on v_mfma_f32_32x32x16_f16: a direct implicit GEMM (M = pixels,
 *     N = out_channels, K = 9 * in_channels), not Winograd.
 *   - The bias, ReLU and BatchNorm epilogue runs in f32.
 *   - The schedule is fixed: no split-K and no atomics.  Results are bit-identical from call to call.
 * w_f16_dev is the conv weight w[co][ci][kh][kw] as fp16 in the layout
 * [out_channels/64][in_channels/16][9][2][64][8]: w[co][ci][kh][kw] at element
 *   (((((co/64)*(in_channels/16) + ci/16)*9 + 3*kh + kw)*2 + (ci/8)%2)*64 + co%64)*8 + ci%8
 * (16 input channels x 64 output channels are one contiguous 18 KB piece; a lane's MFMA B fragment,
 * 8 consecutive input channels of one output channel and tap, is 16 contiguous bytes).
 * y_dev: channels [y_channel_offset, +out_channels) of rows of y_channels floats per pixel, each
 * written exactly once (no zero fill; other channels untouched).  in_channels a multiple of 16,
 * out_channels a multiple of 64, x, w and y 16-byte aligned, height*width*in_channels < 2^31.
 * Launches only: no allocation, no synchronisation (graph-capturable).
 */
int pp_conv3x3_f16_nhwc_dev(pp_ctx_t *ctx, void *stream, const float *x_dev, int batch, int height,
                            int width, int in_channels, const void *w_f16_dev, int out_channels,
                            const float *params_dev, float *y_dev, int64_t y_channels,
                            int64_t y_channel_offset);

/*
 * A 3x3, padding-1 transposed convolution (ConvTranspose2d) of stride s in {2, 4} and output padding
 * op in [0, s) of NHWC f32 x[batch][height][width][in_channels], with the same epilogue and the same
 * arithmetic as pp_conv3x3_f16_nhwc_dev: the opt-in "fp16-up" inference mode.  With
 * Ho = (height-1)*s + 1 + op, Wo = (width-1)*s + 1 + op and w_t the ConvTranspose2d weight
 * [in_channels][out_channels][3][3]:
 *   v[b,oy,ox,co] = sum over kh, kw in {0,1,2} with (oy+1-kh) % s == 0, iy = (oy+1-kh)/s in [0,height),
 *                                  (ox+1-kw) % s == 0, ix = (ox+1-kw)/s in [0,width), and over ci
 *                   of half(x[b,iy,ix,ci]) * half(w_t[ci,co,kh,kw])
 *   y = max(v + bias_co, 0) * scale_co + shift_co,   params_dev [out_channels][3] f32
 * Arithmetic, as for pp_conv3x3_f16_nhwc_dev: each x value is rounded once to IEEE binary16 by the
 * kernel, round to nearest even (never pkrtz); w_f16_dev holds the weights already rounded that way;
 * values beyond the fp16 range become +-inf and fp16 subnormals are kept by both conversions; products
 * are accumulated in f32 on v_mfma_f32_32x32x16_f16; the epilogue runs in f32; the schedule is fixed
 * (no split-K, no atomics): results are bit-identical from call to call.
 * w_f16_dev is w_t as fp16 in the layout [out_channels/64][in_channels/16][9][2][64][8]:
 * w_t[ci][co][kh][kw] at element
 *   (((((co/64)*(in_channels/16) + ci/16)*9 + 3*kh + kw)*2 + (ci/8)%2)*64 + co%64)*8 + ci%8
 * (the layout of pp_conv3x3_f16_nhwc_dev applied to w_t with its first two axes exchanged; the taps are
 * not flipped).
 * y_dev: channels [y_channel_offset, +out_channels) of rows of y_channels floats per pixel of
 * [batch][Ho][Wo], every one written exactly once (no zero fill; other channels untouched), the pixels
 * that no tap reaches included: there v = 0 and y = max(bias_co, 0) * scale_co + shift_co.
 * Non-finite operands: the kernel forms the sum over a fixed 3x3 tap pattern per output phase and feeds
 * fp16 zeros where the definition's iy or ix falls outside the image (the border, and the last row and
 * column of blocks behind the output padding).  With finite fp16 weights that is the definition exactly.
 * A weight that overflowed to +-inf in fp16 gives 0 * inf = NaN at those pixels, where the definition
 * leaves the tap out; pp_conv3x3_f16_nhwc_dev pads with zeros the same way.  Finite weights are the
 * caller's part of the opt-in.
 * in_channels a multiple of 16, out_channels a multiple of 64, x, w and y 16-byte aligned,
 * height*width*in_channels < 2^31.  One launch: no allocation, no synchronisation (graph-capturable).
 */
int pp_convt3x3_f16_nhwc_dev(pp_ctx_t *ctx, void *stream, const float *x_dev, int batch, int height,
                             int width, int in_channels, const void *w_f16_dev, int out_channels,
                             int stride, int output_padding, const float *params_dev, float *y_dev,
                             int64_t y_channels, int64_t y_channel_offset);

/*
 * A 3x3, padding-1, stride-2 convolution of NHWC f32 x[batch][height][width][in_channels], with the same
 * epilogue and the same arithmetic as pp_conv3x3_f16_nhwc_dev: the layers that open the down blocks in the
 * opt-in fp16 inference modes (PPModel.set_inference_precision(..., strided=True)).  height and width are
 * the input's; with Ho = (height+1)/2, Wo = (width+1)/2 and w the Conv2d weight
 * [out_channels][in_channels][3][3]:
 *   v[b,oy,ox,co] = sum over kh, kw in {0,1,2} with iy = 2*oy-1+kh in [0,height), ix = 2*ox-1+kw in
 *                   [0,width), and over ci of half(x[b,iy,ix,ci]) * half(w[co,ci,kh,kw])
 *   y = max(v + bias_co, 0) * scale_co + shift_co,   params_dev [out_channels][3] f32
 * Arithmetic, as for pp_conv3x3_f16_nhwc_dev:
 *   - Each x value is rounded once to IEEE binary16 by the kernel, round to nearest even (never the
 *     round-toward-zero pkrtz conversion); w_f16_dev holds the weights already rounded that way
 *     (torch.Tensor.half()).
 *   - Values beyond the fp16 range become +-inf; fp16 subnormals are kept by both conversions (what the
 *     matrix unit makes of subnormal operands is not part of this contract, as there).
 *   - Products are accumulated in f32 on v_mfma_f32_32x32x16_f16, a direct implicit GEMM (M = output
 *     pixels, N = out_channels, K = 9 * in_channels).
 *   - The bias, ReLU and BatchNorm epilogue runs in f32.
 *   - The schedule is fixed: no split-K and no atomics.  Results are bit-identical from call to call.
 * w_f16_dev is w as fp16 in pp_conv3x3_f16_nhwc_dev's layout [out_channels/64][in_channels/16][9][2][64][8]:
 * w[co][ci][kh][kw] at element
 *   (((((co/64)*(in_channels/16) + ci/16)*9 + 3*kh + kw)*2 + (ci/8)%2)*64 + co%64)*8 + ci%8
 * (the taps are not flipped).
 * y_dev: channels [y_channel_offset, +out_channels) of rows of y_channels floats per pixel of
 * [batch][Ho][Wo], every one written exactly once (no zero fill; other channels untouched).
 * Non-finite operands: the kernel forms the sum over all nine taps and feeds fp16 zeros where the
 * definition's iy or ix falls outside the image (the top row and left column of taps, and the bottom row /
 * right column when height / width is odd).  With finite fp16 weights that is the definition exactly.  A
 * weight that overflowed to +-inf in fp16 gives 0 * inf = NaN at those pixels, where the definition leaves
 * the tap out; pp_conv3x3_f16_nhwc_dev and pp_convt3x3_f16_nhwc_dev pad with zeros the same way.  Finite
 * weights are the caller's part of the opt-in.
 * in_channels a multiple of 16, out_channels a multiple of 64, x, w and y 16-byte aligned,
 * height*width*in_channels < 2^31.  Arguments are rejected before any HIP call.  One launch: no
 * allocation, no synchronisation (graph-capturable).
 */
int pp_conv3x3_s2_f16_nhwc_dev(pp_ctx_t *ctx, void *stream, const float *x_dev, int batch, int height,
                               int width, int in_channels, const void *w_f16_dev, int out_channels,
                               const float *params_dev, float *y_dev, int64_t y_channels,
                               int64_t y_channel_offset);

/*
 * The backbone's first layer straight from the pillars (inference): PPScatter (model/model.py:53-62)
 * -> 3x3, stride-2, padding-1 convolution -> the epilogue of pp_bias_relu_bn_nhwc_dev,
 *   y = max(conv(canvas) + bias_c, 0) * scale_c + shift_c,
 * without building the canvas: only the (pillar, filter tap) pairs that exist are multiplied.
 *   features_dev [batch][in_channels][P] f32, indices_dev [batch][P][3] int64 {flag, col, row}; a
 *                pillar counts as in pp_scatter_canvas_dev (flag != 0, 0 <= row < canvas_h,
 *                0 <= col < canvas_w); two counting pillars in one cell are undefined there and here
 *   w_taps_dev   [9][in_channels][out_channels] f32: tap 3*kh + kw of the Conv2d weight
 *                [out][in][kh][kw]
 *   params_dev   [out_channels][3] f32 {bias, scale, shift}
 *   scratch_dev  16-byte aligned, scratch_bytes >= round_up(batch*canvas_h*canvas_w*4, 256) +
 *                batch*P*in_channels*4 (a cell -> pillar map and the features pillar-major).  Its
 *                contents on entry do not matter and it may be reused from call to call.
 *   y_dev        NHWC [batch][ceil(canvas_h/2)][ceil(canvas_w/2)][out_channels] f32, 16-byte aligned,
 *                every element written exactly once
 * in_channels a multiple of 8, out_channels a multiple of 64.  Two launches, no allocation, no
 * synchronisation (graph-capturable).  No floating-point atomics and a fixed summation order: the
 * result is bit-identical from call to call and under any permutation of the pillars along P.
 */
int pp_conv3x3_s2_pillars_nhwc_dev(pp_ctx_t *ctx, void *stream, const float *features_dev,
                                   const int64_t *indices_dev, int batch, int in_channels,
                                   int max_pillars, int canvas_h, int canvas_w,
                                   const float *w_taps_dev, int out_channels, const float *params_dev,
                                   void *scratch_dev, size_t scratch_bytes, float *y_dev);

/*
 * The detection head (model/model.py:144-160, both 1x1 convolutions as one) on the up blocks' outputs
 * where they lie, channels-last f32, without the concatenated tensor (inference):
 *   y[p][n] = bias[n] + sum_k sum_c W[n][off_k + c] * a_k[p][c],   off_k = channels of the sources before k
 *   a_k[p][c] = src_k[p][c]                                        src_table_dev[k] NULL
 *             = max(src_k[p][c] + b_c, 0) * s_c + t_c              src_table_dev[k] [C_k][3] f32 {b, s, t}
 * The second form is pp_bias_relu_bn_nhwc_dev's expression, operation for operation, applied as the
 * source is loaded: the values multiplied are the bits that kernel would have stored.  f32 throughout
 * (v_mfma_f32_16x16x4_f32, f32 accumulation, channels summed in ascending blocks of 16).
 *   src_dev, src_stride, src_channels, src_table_dev: HOST arrays of n_src (1..4) entries; src_dev[k]
 *                points at source k's first pixel, 16-byte aligned, its pixels src_stride[k] floats
 *                apart (>= C_k, a multiple of 4: a channel slice of a wider tensor is a source);
 *                C_k a multiple of 16
 *   w_packed_dev [K/16][Npad/16][64][4] f32, K = sum C_k, Npad = out_channels rounded up to 16:
 *                element [kb][nt][l][j] = W[16*nt + l%16][16*kb + 4*(l/16) + j], zero for rows past
 *                out_channels; 16-byte aligned
 *   bias_dev     [out_channels] f32
 *   y_dev        rows of y_stride (>= out_channels) floats per pixel; [p][0, out_channels) is written
 *                exactly once, nothing else
 * out_channels 1..64; (K/16) * (Npad * 64 + 192) bytes must fit 160 KiB of LDS (K = 384 at Npad 64).
 * One launch of persistent workgroups: no allocation, no synchronisation (graph-capturable); no atomics
 * and a fixed summation order, so the result is bit-identical from call to call.
 */
int pp_head1x1_nhwc_dev(pp_ctx_t *ctx, void *stream, int64_t pixels, int n_src,
                        const float *const *src_dev, const int64_t *src_stride, const int *src_channels,
                        const float *const *src_table_dev, const float *w_packed_dev,
                        const float *bias_dev, int out_channels, float *y_dev, int64_t y_stride);

/*
 * The ReLU -> BatchNorm2d tail of the backbone blocks in TRAINING mode (model/model.py:76-84,
 * 105-109; BatchNorm with batch statistics), forward and backward, on NCHW f32 tensors:
 *   forward   y = gamma*(max(z,0) - mean)*invstd + beta with the batch mean / biased variance
 *             of max(z,0) per channel; mean_out / invstd_out [channels] are kept for the
 *             backward; running_mean / running_var (both or neither NULL) are updated with
 *             `momentum` (unbiased variance), exactly as nn.BatchNorm2d does.
 *   backward  dz = [z > 0] * gamma*invstd * (dy - mean(dy) - xhat*mean(dy*xhat)),
 *             dgamma = sum dy*xhat, dbeta = sum dy.  Only z is needed from the forward.
 *   z_dev, y_dev, dy_dev, dz_dev [batch][channels][hw] f32
 *   dy_batch_stride (floats; 0 = channels*hw): dy may be a channel slice of a wider NCHW
 *             tensor (the gradient of one input of torch.cat), read in place
 *   conv_bias_dev [channels] or NULL: z is then the convolution WITHOUT its bias, the kernels
 *             use z + bias, and the backward also returns dbias_dev = sum dz (may be NULL)
 * Non-finite input, two rules (tests/test_gpu_bn_train_nonfinite.py):
 *   The ReLU is torch.relu's, u < 0 ? 0 : u, in both directions: a NaN stays a NaN (fmaxf would
 *             return the 0), +inf stays +inf, -inf becomes 0.  A NaN or +inf in a channel makes
 *             mean_out and invstd_out of that channel non-finite and every y of it NaN; the
 *             backward on those statistics gives NaN dgamma and dbias, and dz NaN where
 *             z + bias > 0 (0 where it is <= 0: the strict mask).  No other channel changes.
 *   A channel whose batch mean or variance is not finite KEEPS running_mean and running_var:
 *             (1 - momentum)*NaN would stay NaN for good, and the model of a step that the
 *             optimizer dropped has to evaluate afterwards.  mean_out / invstd_out stay non-finite.
 *             The test is made on the two f32 values that would be stored, so a finite f64
 *             statistic beyond FLT_MAX is kept out as well: these kernels never store a
 *             non-finite running statistic over a finite one.
 *   What a dropped step does not keep is outside these kernels: the layers ahead of the bad one
 *             saw ordinary statistics and update theirs, and the caller's num_batches_tracked
 *             (model.py increments it on the host, without a wait, at every call) may advance.
 */
int pp_relu_bn_train_fwd_dev(pp_ctx_t *ctx, void *stream, const float *z_dev,
                             const float *conv_bias_dev, int64_t batch, int channels, int64_t hw,
                             const float *gamma_dev, const float *beta_dev,
                             double eps, double momentum, float *running_mean_dev,
                             float *running_var_dev, float *y_dev, float *mean_out_dev,
                             float *invstd_out_dev);
int pp_relu_bn_train_bwd_dev(pp_ctx_t *ctx, void *stream, const float *z_dev,
                             const float *conv_bias_dev, const float *dy_dev, int64_t dy_batch_stride,
                             int64_t batch, int channels, int64_t hw, const float *gamma_dev,
                             const float *mean_dev,
                             const float *invstd_dev, float *dz_dev, float *dgamma_dev,
                             float *dbeta_dev, float *dbias_dev);

/*
 * PPLoss (model/loss.py:24-63) forward and backward without a host read-back: focal-weighted BCE over every
 * classification logit, smooth-L1 over the 7 regression dims and BCE over the orientation logit of the
 * POSITIVE anchors (reg_t[..., 0] == 1), total = b_cls*cls + b_reg*reg + b_ort*ort.
 *   cls_dev      [batch][anchors_per_cell*classes][height][width] f32 logits
 *   reg_dev      [batch][anchors_per_cell*8][height][width] f32
 *                layout PP_LOSS_NCHW: both contiguous in that order; PP_LOSS_NHWC: the same tensors stored
 *                channels-last ([batch][height][width][channels]); dcls_dev / dreg_dev come back in that layout
 *   cls_t_dev    [batch][A][classes] f32, reg_t_dev [batch][A][9] f32 contiguous, A = height*width*anchors_per_cell
 *                in (h, w, a) order: what pp_assign_targets_*batch_dev writes
 *   forward      workspace_dev: pp_loss_workspace_bytes(params) bytes, 8-byte aligned (per-workgroup partial sums);
 *                scalars_dev f64[5] = {cls, reg, ort, total, n_pos}; losses_dev f32[4] = the first four;
 *                p_dev [batch][A*classes] f32 = sigmoid of the logits in the targets' order, or NULL.
 *                Per element: p = sigmoid(x), w = (t == 1 ? alpha*(1 - p)^gamma : p^gamma), a constant for the
 *                gradient; cls = sum w*bce(x, t) / (batch*A*classes).  reg / ort are means over 7*n_pos / n_pos
 *                elements: NaN without a positive anchor, like the mean over an empty selection.  tanh is applied
 *                to channel 6 of the whole anchors_per_cell*8 axis (the first anchor's dim 6 only), as the
 *                reference does.  Sums across elements are f64 in a fixed order: bit-identical from call to call.
 *   backward     grads4_dev f32[4]: the incoming gradients of (cls, reg, ort, total); scalars_dev from the forward
 *                (only n_pos is read); every element of dcls_dev / dreg_dev is written; a non-positive anchor's
 *                dreg is exactly +0.0 whatever grads4 holds.
 * Three launches on `stream` (partial sums, finalize, backward); no allocation, no atomics, no synchronisation.
 * PP_ERR_VALUE, before any HIP call: NULL arguments (p_dev excepted), sizes < 1, anchors_per_cell*9 or
 * anchors_per_cell*classes > 95, an unknown layout, gamma < 0 (or NaN).
 * pp_loss_workspace_bytes returns the byte count, or PP_ERR_VALUE for bad params.
 */
#define PP_LOSS_NCHW 0
#define PP_LOSS_NHWC 1
typedef struct pp_loss_params {
  int32_t batch, anchors_per_cell, classes, height, width;
  int32_t layout;             /* PP_LOSS_* */
  double gamma, alpha;        /* focal exponent (2) and positive weight (25) */
  double b_cls, b_reg, b_ort; /* total = b_cls*cls + b_reg*reg + b_ort*ort */
} pp_loss_params_t;
int64_t pp_loss_workspace_bytes(const pp_loss_params_t *params);
int pp_loss_fwd_dev(pp_ctx_t *ctx, void *stream, const float *cls_dev, const float *reg_dev,
                    const float *cls_t_dev, const float *reg_t_dev, const pp_loss_params_t *params,
                    void *workspace_dev, double *scalars_dev, float *losses_dev, float *p_dev);
int pp_loss_bwd_dev(pp_ctx_t *ctx, void *stream, const float *cls_dev, const float *reg_dev,
                    const float *cls_t_dev, const float *reg_t_dev, const pp_loss_params_t *params,
                    const double *scalars_dev, const float *grads4_dev, float *dcls_dev, float *dreg_dev);

/*
 * The device entry points never synchronise.  pp_voxelize_check synchronises `stream` and
 * returns PP_ERR_HIP (with the runtime's message) if a launch on it failed, else PP_OK.  The
 * voxelizer kernels themselves have no failure mode of their own any more: no workgroup waits
 * for another one (round 1's look-back scan and its time-out flag are gone), every array is
 * written before it is read within one call.  (The reference's only analogue is to fail
 * loudly: pillars.cpp:166-169.)
 */
int pp_voxelize_check(pp_ctx_t *ctx, void *stream);

/*
 * Limits of the voxelizer entry points (PP_ERR_VALUE beyond them):
 *   batch                  <= PP_MAX_BATCH (32) sweeps per call
 *   points per sweep       <  2^30
 *   cell grid              <= 32768 cells per axis and <= 16 777 216 cells in all (a tile of
 *                             up to 4096 cells lives in LDS, at most 4096 tiles); the workspace
 *                             holds 16 bytes per cell and sweep for the tiles' descriptor lists
 *   max_points_per_pillar  <= 65536; dense output: max_pillars * max_points_per_pillar <= 1e8
 *   fused feature net      exactly 64 output channels (model/model.py:28)
 *   alignment              points_dev, pillars_dev, features_dev and canvas_dev 16 bytes (they are accessed 16
 *                          bytes a lane); indices_dev, prev_indices_dev, clear_indices_dev and num_cells_dev 8 bytes
 * One context per HIP stream: calls on one context must be stream-ordered.
 */

/*
 * Validation mAP over 3D IoU thresholds: the matching step of the metric the
 * reference takes from the lyft SDK (evaluate.py:247-278, get_average_precisions; train.py:175-196).
 * The SDK is absent; its semantics are restated from recall, not pinned.
 *
 * pp_box3d_iou_dev: dense 3D IoU of car-space boxes, contiguous f64 device arrays
 *   a_dev [Na][7], b_dev [Nb][7]: x,y,z (centre), w,l,h, yaw -- footprint a rectangle with length l
 *   along the yaw direction and width w across it; out_dev [Na][Nb] f64:
 *   clip(area(footprint_a ∩ footprint_b) * z-overlap / (w_a l_a h_a + w_b l_b h_b - that), 0, 1)
 *   (Box3D.get_iou).  Limits (PP_ERR_VALUE beyond): 0 <= Na, Nb <= 2^24, Na*Nb <= 2^32.
 *
 * pp_eval_match_batch_dev: TP / FP flags of a batch of samples, two launches on `stream`, no host
 * sync.  Per sample b:
 *   boxes_dev [batch][max_out][9] f64   postprocess.Detector's rows x,y,z,w,l,h,yaw,score,class
 *                                       (car space, pp_decode_batch_dev's boxes_out)
 *   count_dev [batch] int32 (device)    valid rows per sample; rows >= count are written invalid
 *   g_counts  [batch] int32 (HOST)      ground-truth boxes per sample
 *   g_centers [T][3] g_wlh [T][3] g_yaw [T] f64, g_class [T] int32 (device, T = sum of g_counts,
 *                                       the samples concatenated): CANVAS-space boxes, moved to car
 *                                       space here as move_box_to_car_space(image=False) does
 *                                       (evaluate.py:91-125) -- the slices at 11T / 14T / 17T / 18T
 *                                       (f64 elements) of TargetAssigner.upload_batch's buffer
 * Outputs [batch][max_out] (invalid rows: tp 0, max_iou -1, argmax -1):
 *   max_iou_out f64, argmax_out int32   the best IoU over the sample's GT of the row's class and its
 *                                       index in the sample's GT list (first index on ties); -1 / -1
 *                                       when the sample has no GT of that class
 *   tp_mask_out uint16                  bit t: the row is a TP at thresholds[t] -- in the order
 *                                       (score desc, row asc), a row is a TP iff max_iou > t (strict)
 *                                       and its argmax GT was not taken by an earlier TP; no fall-back
 *                                       to the second-best GT (recall_precision)
 *   gt_per_class_out [batch][num_classes] int32: the sample's GT per class
 * Classes outside 0..num_classes-1 never match and are not counted.
 * Limits (PP_ERR_VALUE beyond): 1 <= batch <= PP_MAX_BATCH, 1 <= max_out <= 1024,
 *   1..32 classes, 1..16 thresholds, 0..65535 GT per sample.
 */
typedef struct pp_eval_params {
  int32_t num_classes;     /* cfg.DATA.NUM_CLASSES, config.py:97                       */
  int32_t n_thresholds;
  double thresholds[16];   /* cfg.DATA.VAL_THRESH_LIST: np.arange(.5, 1., .05)         */
  double x_step, y_step;   /* the GT frame: cfg.DATA.X_STEP / Y_STEP, X_MIN / Y_MIN    */
  double x_min, y_min;
} pp_eval_params_t;

int pp_box3d_iou_dev(pp_ctx_t *ctx, void *stream, int64_t Na, const double *a_dev, int64_t Nb,
                     const double *b_dev, double *out_dev);
int pp_eval_match_batch_dev(pp_ctx_t *ctx, void *stream, int32_t batch, const double *boxes_dev,
                            int32_t max_out, const int32_t *count_dev, const int32_t *g_counts,
                            const double *g_centers, const double *g_wlh, const double *g_yaw,
                            const int32_t *g_class, const pp_eval_params_t *prm,
                            uint16_t *tp_mask_out, double *max_iou_out, int32_t *argmax_out,
                            int32_t *gt_per_class_out);

/*
 * Training augmentation of the points and the ground-truth boxes of a batch (the
 * reference has none): the global flip / rotation / scale / translation and the per-object noise of
 * SECOND / PointPillars, where every box and the points inside it get a small rigid motion that is
 * rejected if it collides with another box.  The HOST draws every random number; there is no RNG on the
 * device.  Two launches on `stream` (k_aug_boxes, k_aug_points), ordered by the launch boundary alone;
 * no allocation, no synchronisation.  All geometry is f64, every product and sum rounded separately.
 * The augmentation works in car space (metres), where the points live; the boxes come in and go out in
 * canvas space: x = cx*x_step + x_min, y = cy*y_step + y_min, z = cz, w_car = w*y_step, l_car = l*x_step,
 * h, yaw unchanged (evaluate.gt_to_car_space), and the inverse on the way out.
 *
 * Inputs (device memory unless marked HOST):
 *   batch          1..PP_MAX_BATCH samples
 *   points_dev     [batch][points_stride][4] f32 (x, y, z, reflectance), 16-byte aligned
 *   n_points       HOST [batch]: rows at or beyond n_points[b] are neither read nor written
 *   g_counts       HOST [batch]: boxes per sample, 0..1024 each (a sample's footprints live in LDS);
 *                  the samples' boxes are concatenated in sample order, T = their sum
 *   g_centers_dev [T][3]  g_wlh_dev [T][3]  g_yaw_dev [T]   f64, canvas space
 *   noise_dev      [T][tries][6] f64: {dx, dy, dz, dpsi, cos(dpsi), sin(dpsi)} (metres, radians)
 *   global_dev     [batch][10] f64: {fx, fy, theta, cos(theta), sin(theta), s, tx, ty, tz, 0},
 *                  fx, fy in {+1.0, -1.0}
 *   prm            the grid scalars of the voxelizer and `tries` (1..64)
 *
 * Boxes, one workgroup per sample.  The footprint of a pose (x, y, w, l, yaw) is the rectangle of
 * Box.bottom_corners: length l along the yaw direction, width w across it.  cur[i] starts as the
 * car-space pose of every box.  For j ascending, for k = 0..tries-1: the candidate is
 * (c_j + (dx,dy,dz), yaw_j + dpsi) of noise[j][k]; it collides unless, for every i != j, it and cur[i]
 * are separated along one of the four edge directions (projection intervals strictly disjoint; touching
 * collides; a candidate with a non-finite component collides).  The first candidate that does not collide
 * is taken: cur[j] = candidate, sel[j] = k; if every try collides, sel[j] = -1 and cur[j] stays.  Later
 * boxes are tested against the updated cur[].  Then every cur[j] goes through the global transform: the
 * centre as a point (below), wlh' = s*wlh, yaw' = theta + yaw for (fx,fy) = (+,+), theta - yaw for (+,-),
 * theta + pi - yaw for (-,+), theta + pi + yaw for (-,-); yaw is not wrapped.  keep[j] = 1 iff the new
 * car-space centre lies in [x_min,x_max] x [y_min,y_max] x [z_min,z_max], bounds included
 * (utils/box_utils.py:265-267).  A box with keep 0 is PARKED: its canvas-space centre is written as
 * (-1e6, -1e6, z'), so its IoU with every anchor is 0, the target kernels drop it as create_target's
 * np.nonzero(top_anchor_for_box) filter does, and g_counts stays what it was.
 *
 * Points.  A row whose x is NaN (a point pp_ingest_dev removed) is copied unchanged.  Otherwise, with
 * x, y, z as f64: the owner is the lowest j whose ORIGINAL box contains the point -- ux = x-cx, uy = y-cy,
 * lx = c*ux + s*uy, ly = -s*ux + c*uy, lz = z-cz, inside iff |lx| <= l/2, |ly| <= w/2, |lz| <= h/2 (c, s of
 * the original yaw, computed on the device).  With an owner and sel[j] = k >= 0:
 *   x1 = (cd*ux - sd*uy) + (cx + dx),  y1 = (sd*ux + cd*uy) + (cy + dy),  z1 = z + dz
 * (cd, sd, dx, dy, dz of noise[j][k]); otherwise x1, y1, z1 = x, y, z.  Then, with xf = fx*x1, yf = fy*y1:
 *   x2 = s*(ct*xf - st*yf) + tx,  y2 = s*(st*xf + ct*yf) + ty,  z2 = s*z1 + tz
 * each rounded to f32 once; the reflectance is copied bit for bit.  The moved coordinates use only
 * host-supplied cosines and sines, so an f64 restatement reproduces them bit for bit.
 *
 * Outputs, the five arrays pp_assign_targets_batch_dev reads plus two flags per box:
 *   points_out_dev      [batch][points_stride][4] f32; may alias points_dev
 *   corners_out_dev [T][4][2]  centers_img_out_dev [T][3]  centers_out_dev [T][3]  wlh_out_dev [T][3]
 *   yaw_out_dev [T]     f64, canvas space; corners and image-space centres as boxes_to_image_space
 *                       (utils/box_utils.py:19-32): the bottom corners, then (canvas_height-1) - y.
 *                       They must not alias the box inputs (the points read the originals).
 *   sel_out_dev [T]  keep_out_dev [T]  int32
 * The classes are not touched: the caller hands the same class array on.
 * Limits (PP_ERR_VALUE beyond, checked before any HIP call): 1 <= batch <= PP_MAX_BATCH, 0..1024 boxes
 * per sample, 1 <= tries <= 64, 0 <= n_points[b] <= points_stride, positive finite steps.
 */
typedef struct pp_augment_params {
  double x_step, y_step;            /* cfg.DATA.X_STEP / Y_STEP, config.py:46-47         */
  double x_min, y_min, z_min;       /* the range filter and the canvas frame              */
  double x_max, y_max, z_max;
  double canvas_height;             /* cfg.DATA.CANVAS_HEIGHT, config.py:60               */
  int32_t tries;                    /* candidate motions per box                          */
  int32_t reserved;
} pp_augment_params_t;

int pp_augment_batch_dev(pp_ctx_t *ctx, void *stream, int32_t batch, const float *points_dev,
                         int64_t points_stride, const int32_t *n_points, const int32_t *g_counts,
                         const double *g_centers_dev, const double *g_wlh_dev, const double *g_yaw_dev,
                         const double *noise_dev, const double *global_dev,
                         const pp_augment_params_t *prm, float *points_out_dev,
                         double *corners_out_dev, double *centers_img_out_dev, double *centers_out_dev,
                         double *wlh_out_dev, double *yaw_out_dev, int32_t *sel_out_dev,
                         int32_t *keep_out_dev);

/*
 * Ground-truth sampling ("object pasting") of SECOND / PointPillars for a batch (the
 * reference has no augmentation): objects recorded in a bank -- their points in car space, their boxes in
 * canvas space -- are pasted into the samples where they fit.  The HOST draws which bank objects to try and
 * appends their boxes to each sample's ground truth; the device decides which fit, copies their points in
 * and removes the scene points underneath.  Two launches on `stream` (k_paste_boxes, k_paste_points),
 * ordered by the launch boundary alone; no allocation, no synchronisation, no atomics.  All geometry is
 * f64, every product and sum rounded separately; canvas -> car as for pp_augment_batch_dev.
 *
 * Inputs (device memory unless marked HOST):
 *   batch          1..PP_MAX_BATCH samples
 *   points_dev     [batch][points_stride][4] f32 (x, y, z, reflectance), 16-byte aligned
 *   n_points       HOST [batch]: the scene rows of each sample, 0..points_stride
 *   g_counts       HOST [batch]: boxes per sample, originals AND candidates, 0..1024; the samples' boxes
 *                  are concatenated in sample order
 *   c_counts       HOST [batch]: the LAST c_counts[b] boxes of sample b are its candidates, in try order;
 *                  0..256 and at most g_counts[b].  S = their sum
 *   g_centers_dev [T][3] (in/out)  g_wlh_dev [T][3]  g_yaw_dev [T]   f64, canvas space
 *   bank_points_dev [bank_rows][4] f32, car space, 16-byte aligned
 *   table_dev      [S][3] int32, the samples' candidates concatenated: {first bank row, rows, first
 *                  output row}.  A sample's entries ascend in their first output row (augment.paste_table
 *                  builds them contiguous from n_points[b])
 *   n_out          HOST [batch]: output rows per sample, n_points[b]..out_stride
 *
 * Boxes, one workgroup per sample.  The footprint of a box is that of pp_augment_batch_dev, with cos and
 * sin of the yaw computed on the device.  For k ascending, candidate k is ACCEPTED iff its x, y, z, w, l and
 * yaw are finite, its footprint is separated from the footprint of every original box of the sample, and
 * from that of every candidate accepted before it.  Separated: projection intervals strictly disjoint
 * along one of the four edge directions; touching collides; an original whose x, y, z, w, l or yaw is not
 * finite collides with every candidate.  A candidate that was rejected stands in nobody's way.
 * accept_out_dev[k] = 1 or 0.  A rejected candidate is PARKED: x and y of its canvas-space centre are
 * overwritten with -1e6 (its z, wlh and yaw stay), so the target kernels drop it and g_counts stays what
 * it was.  Nothing else of the box arrays is written.
 *
 * Points.  Scene rows p < n_points[b] are copied bit for bit; with remove_scene_points = 1, a row whose x
 * is not NaN and that lies inside an ACCEPTED candidate's box (the point-in-box test of
 * pp_augment_batch_dev: f64, bounds included) is copied with x replaced by the f32 quiet NaN 0x7FC00000,
 * the mark of a removed point; its y, z and reflectance stay.  Rows n_points[b] <= p < n_out[b] belong to
 * the candidates: row first_out + i (0 <= i < rows) receives bank row first_bank + i bit for bit if the
 * candidate was accepted, and with x replaced by 0x7FC00000 if it was rejected.  The candidate of a row is
 * the last table entry of the sample whose first output row is at or before it; an entry with 0 rows owns
 * none.  Rows at or beyond n_out[b] are neither read nor written.  A table entry is never followed outside
 * its arrays: a row whose bank row would be negative or at or beyond bank_rows, or that no entry covers, is
 * skipped (left unwritten); no row below n_points[b] or at or beyond n_out[b] is written for it.
 *
 * Outputs:
 *   points_out_dev  [batch][out_stride][4] f32; may be points_dev itself when out_stride == points_stride
 *   accept_out_dev  [S] int32
 * S = 0 is legal: the call copies the scene rows.
 * Limits (PP_ERR_VALUE beyond, checked before any HIP call): NULL arguments, 1 <= batch <= PP_MAX_BATCH,
 * 0 <= g_counts[b] <= 1024, 0 <= c_counts[b] <= min(256, g_counts[b]), 0 <= n_points[b] <= points_stride,
 * n_points[b] <= n_out[b] <= out_stride, positive finite steps, remove_scene_points in {0, 1}.
 */
typedef struct pp_paste_params {
  double x_step, y_step, x_min, y_min;     /* canvas -> car, as pp_augment_params_t */
  int32_t remove_scene_points, reserved;
} pp_paste_params_t;

int pp_paste_batch_dev(pp_ctx_t *ctx, void *stream, int32_t batch, const float *points_dev,
                       int64_t points_stride, const int32_t *n_points, const int32_t *g_counts,
                       const int32_t *c_counts, double *g_centers_dev, const double *g_wlh_dev,
                       const double *g_yaw_dev, const float *bank_points_dev, int64_t bank_rows,
                       const int32_t *table_dev, const pp_paste_params_t *prm, float *points_out_dev,
                       int64_t out_stride, const int32_t *n_out, int32_t *accept_out_dev);

/* Timing hooks for bench.py: with a ring of `slots` HIP event pairs per kernel
 * (slots = 0 disables), every pp_voxelize*_dev call brackets each of its three launches
 * (PP_KERNEL_SPLIT, PP_KERNEL_TILE, PP_KERNEL_EMIT) with an event pair bound to the dispatch
 * packet.  pp_ctx_read_kernel_ms synchronises on the recorded stop events and returns up to
 * `cap` elapsed times of kernel `which` (oldest first, in milliseconds); reading
 * PP_KERNEL_EMIT empties the ring.  pp_ctx_read_emit_ms = the PP_KERNEL_EMIT row.
 * pp_voxelize_step_dev launches ONE kernel (k_step); its pair is recorded in the PP_KERNEL_EMIT
 * column and the other two columns read as empty. */
#define PP_KERNEL_SPLIT 0
#define PP_KERNEL_TILE 1
#define PP_KERNEL_EMIT 2
int pp_ctx_set_timing(pp_ctx_t *ctx, int slots);
int pp_ctx_read_kernel_ms(pp_ctx_t *ctx, int which, float *ms, int cap, int *count);
int pp_ctx_read_emit_ms(pp_ctx_t *ctx, float *ms, int cap, int *count);

/* Self-test of the host thread pool behind the two host entry points (pp_create_pillars_f64's gather and scatter,
 * pp_make_ious_f64's zero fill): needs no device.  Runs `jobs` jobs on a pool of `threads` threads, alternating the
 * blocking form and the start / wait form, every part adding its own range of 1..n into a per-part slot; returns 0
 * when every part of every job ran exactly once with the right (part, parts) pair, else the index of the first job
 * that went wrong + 1.  (The reference has no counterpart: its module is single-threaded and holds the GIL,
 * data/pillars.cpp:429-435.) */
int pp_host_pool_selftest(int threads, int jobs, int n);

#ifdef __cplusplus
}
#endif
#endif
