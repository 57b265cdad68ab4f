/*
 * rcn.h -- C ABI of the MI355X (gfx950) matching + bundle-adjustment core.
 *
 * Drop-in boundary for ONE hot path of smileyenot983/reconstructor:
 *   - all-pairs descriptor matching  (replaces FlannMatcher::matchFeatures' call into
 *     cv::DescriptorMatcher::knnMatch, FeatureMatcher.cpp:32-65, and the pair loop of
 *     SequentialReconstructor::matchFeatures, SequentialReconstructor.cpp:199-279)
 *   - bundle adjustment              (replaces BundleAdjuster::adjust's call into
 *     ceres::Solve, BundleAdjuster.cpp:72-146)
 *
 * Plain pointers and sizes only; no C++ or torch types; never throws.  Every entry point
 * returns an int status (RCN_OK == 0, negative = error; rcn_last_error() has the text).
 * Host arrays are borrowed for the duration of the call; device buffers belong to the ctx.
 * One ctx per GPU.  A ctx is safe to call from several host threads (internal mutex): the
 * reference calls its matcher from 4 OpenMP threads (SequentialReconstructor.cpp:202).
 *
 * There is NO CPU fallback behind this ABI: without a usable HIP device rcn_create fails.
 */
#ifndef RCN_H
#define RCN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RCN_OK               0
#define RCN_ERR_ARG         -1   /* bad argument (null pointer, negative size, mismatched D, ...) */
#define RCN_ERR_HIP         -2   /* HIP runtime error; text in rcn_last_error */
#define RCN_ERR_NO_DEVICE   -3   /* no gfx950 device visible */
#define RCN_ERR_UNSUPPORTED -4   /* shape outside what the kernels cover */
#define RCN_ERR_NOT_FOUND   -5   /* image id not resident */
#define RCN_ERR_NUMERIC     -6   /* BA: non-finite cost / Cholesky breakdown that LM could not recover */
#define RCN_ERR_COMM        -7   /* RCCL error (sharded grid); text in rcn_last_error */
#define RCN_ERR_IO          -8   /* store file: cannot open / short read / bad magic, version or checksum */

typedef struct rcn_ctx rcn_ctx;

/* ---- context ------------------------------------------------------------------------- */
int         rcn_device_count(void);                  /* HIP devices visible to this process (0 without a GPU) */
int         rcn_create(int device_id, rcn_ctx **out);
void        rcn_destroy(rcn_ctx *ctx);
const char *rcn_last_error(const rcn_ctx *ctx);      /* never NULL */
/* ABI revision of this header.  Bumped whenever a struct the library writes through a caller's pointer grows or an entry point changes
 * its arguments: a caller built against an older header must not be linked against a newer library (rcn_match_last_stats copies the whole
 * rcn_match_stats; revision 2 -> 3 added rows_brute_force, chunks, coarse_launches to it and rcn_ba_factor_plan to the library;
 * 3 -> 4 added the triangulation entry points and rcn_triangulation_problem; 4 -> 5 the resident match lists, the 2D-3D
 * correspondence search and the attach entry points; 5 -> 6 added coarse_dtype to rcn_match_stats; 6 -> 7 the two-view
 * initialisation entry points and rcn_twoview_options; 7 -> 8 the optimal-matching layer rcn_sg_* and rcn_sg_options;
 * 8 -> 9 the graph network rcn_sg_net_*; 9 -> 10 SuperPoint's convolutional network rcn_sp_net_*; 10 -> 11 the robust losses rcn_ba_solve_robust, rcn_ba_session_set_loss,
 * rcn_ba_session_loss_report; 11 -> 12 constant cameras and the local adjustment: rcn_ba_solve_constant, rcn_ba_session_solve_local,
 * rcn_ba_session_covisible, rcn_ba_session_local_seconds; 12 -> 13 the homography search rcn_homography_* and the two-view
 * classification rcn_twoview_geometry* with their option structs; 13 -> 14 shared intrinsics: rcn_ba_solve_tied,
 * rcn_ba_session_set_groups; 14 -> 15 the ORB detector rcn_orb_*; 15 -> 16 the binary residency rcn_bits_* and the Hamming matcher
 * rcn_match_pair_hamming, rcn_match_grid_hamming, rcn_match_grid_hamming_device, rcn_hamming_knn2_device; 16 -> 17 guided matching
 * rcn_match_guided*, rcn_match_pair_guided, rcn_guided_knn2_device, rcn_match_grid_guided with rcn_guided_options, and
 * rcn_match_table_filter_model_device); 17 -> 18 track building rcn_tracks_* with rcn_tracks_options;
 * 18 -> 19 the plane sweep rcn_mvs_* with rcn_mvs_options and rcn_mvs_sizes, rcn_img_undistort_device
 * and rcn_ba_session_mvs_views).
 * rcn_version() names the library build ("reconstructor_amd 0.<revision> (gfx950)"); compare the two at start-up. */
#define RCN_ABI_REVISION 19
const char *rcn_version(void);
/* Run all work of this ctx on an existing HIP stream (e.g. torch's current stream, passed as
 * the raw hipStream_t).  NULL = the ctx's own stream.  */
int         rcn_set_stream(rcn_ctx *ctx, void *hip_stream);
int         rcn_synchronize(rcn_ctx *ctx);

/* ---- descriptors -----------------------------------------------------------------------
 * One dense row-major K x D fp32 matrix per image: exactly what featDescToCV builds per call
 * (FeatureMatcher.cpp:11-25), built once per image here instead of once per pair.
 * All resident images must share D.  Re-uploading an id replaces it.  K may be 0. */
int rcn_desc_upload(rcn_ctx *ctx, int32_t img_id, const float *desc_host, int32_t K, int32_t D);
/* Same, from a DEVICE pointer (e.g. the landing buffer of an RCCL all-gather); copied. */
int rcn_desc_upload_device(rcn_ctx *ctx, int32_t img_id, const float *desc_dev, int32_t K, int32_t D);
/* n_images equally shaped images [n][K][D] in one DEVICE buffer, ids first_img_id.. ; the
 * buffer is BORROWED (zero copy) until rcn_desc_clear / re-upload of those ids: the caller
 * keeps it alive and unchanged.  One stats launch + one conversion launch for the whole
 * batch; calling it again with the same shape reuses every allocation (per-step ingest of
 * an all-gather landing buffer).  When D % 4 == 0 the block must be 16-byte aligned
 * (RCN_ERR_ARG otherwise; hipMalloc / torch allocations are). */
int rcn_desc_upload_batch_device(rcn_ctx *ctx, int32_t first_img_id, int32_t n_images,
                                 const float *desc_dev, int32_t K, int32_t D);
/* Producer contract.  The layout above -- [n][K][D] fp32 row-major in HBM, D = 256 unit-norm rows for SuperPoint
 * (FeatureSuperPoint.cpp:183-211), 128 for SIFT, 32 for ORB-as-float -- is what a detector running on the GPU
 * writes straight into: either its own buffer handed to rcn_desc_upload_batch_device (borrowed, zero copy), or
 * the slot rcn_shard_reserve returns.  Rows past an image's keypoint count must be zero (rcn_shard_exchange's
 * local_K) or the images are uploaded one by one.  rcn_desc_sample_device is the last step of such a detector:
 * processDescriptors of the reference (cell = keypoint / 8 in integers, the first D <= 256 channels of that cell
 * of the dense descriptor map, divided by FeatDesc::norm(): fp32 squares summed in fp64 in ascending order),
 * bit-exact, writing K rows of D floats to out_rows_dev.  The map is addressed by element strides: the network's
 * own [C][Hc][Wc] output is (Hc*Wc, Wc, 1), a channel-last copy is (1, Wc*C, C).  Asynchronous on the ctx stream. */
int rcn_desc_sample_device(rcn_ctx *ctx, const float *desc_map_dev, int64_t stride_c, int64_t stride_y, int64_t stride_x,
                           int32_t Hc, int32_t Wc, const int32_t *kp_xy_dev, int32_t K, int32_t D, float *out_rows_dev);
/* A keypoint outside [0, 8*Wc) x [0, 8*Hc) reads nothing (the reference's tensor indexing throws there): its row is
 * written as zeros and counted.  rcn_desc_sample_errors waits for the ctx stream and returns RCN_ERR_ARG (count in
 * *n_out_of_range, may be NULL) when any keypoint of the calls since the last read was outside; the count is cleared. */
int rcn_desc_sample_errors(rcn_ctx *ctx, int32_t *n_out_of_range);
/* The same for n images in one launch: map i at desc_maps_dev + i * stride_img, keypoints kp_xy_dev[i][K][2], rows
 * out_rows_dev[i][K][D].  The first min(counts_dev[i], K) rows of image i are bit-identical to rcn_desc_sample_device;
 * the rows past them are written as zeros (the local_K contract of rcn_shard_exchange) and are NOT counted as
 * out-of-map errors, whatever their coordinates hold (rcn_kp_detect_device pads with (-1, -1)). */
int rcn_desc_sample_batch_device(rcn_ctx *ctx, const float *desc_maps_dev, int64_t stride_img, int64_t stride_c, int64_t stride_y, int64_t stride_x,
                                 int32_t Hc, int32_t Wc, const int32_t *kp_xy_dev /*[n][K][2]*/, const int32_t *counts_dev /*[n]*/,
                                 int32_t n, int32_t K, int32_t D, float *out_rows_dev /*[n][K][D]*/);

/* ---- keypoints ---------------------------------------------------
 * processKeypoints of the reference (FeatureSuperPoint.cpp:145-179) for n images per call: heat map from the network's
 * [65][H/8][W/8] logits, threshold, nmsFast, border filter; all in HBM, asynchronous on the ctx stream.
 *   logits: element strides as in rcn_desc_sample_device -- NCHW is (65*Hc*Wc, Hc*Wc, Wc, 1), NHWC (Hc*Wc*65, 1, Wc*65, 65).
 *   heat_mode: RCN_KP_HEAT_REFERENCE is extractHeatMap as written (each plane row divided by the sum of the plane as
 *   modified so far, + 1e-5); RCN_KP_HEAT_SOFTMAX is the softmax over the 65 channels of a cell.  Channel 64 is dropped
 *   and heat[8 yc + c / 8][8 xc + c % 8] = h[c][yc][xc].  This stage carries a tolerance (expf); the rest is exact.
 *   A pixel is a candidate iff (double)heat >= conf_thresh (never a NaN).  Canonical order: confidence descending, then
 *   raster index y * W + x ascending (std::stable_sort on the reference's raster-ordered input).  nmsFast with
 *   distThresh = nms_radius in that order; then keypoints with x < border || x >= W - border || y < border ||
 *   y >= H - border are dropped.  Output in raster order; counts_dev[i] is the number of survivors; when it exceeds K
 *   the K first of the canonical order are emitted (still in raster order).  Rows past min(counts[i], K): xy (-1, -1),
 *   conf 0.  heat_out_dev receives the dense heat maps, rounds_dev the rounds of the NMS iteration per image.
 * RCN_ERR_ARG: H or W no positive multiple of 8 (rcn_kp_nms_device: not positive), H * W > 2^31 - 1, n < 0, K < 1,
 * nms_radius outside 0..8, border < 0, unknown mode, null required pointer.  n == 0 launches nothing. */
#define RCN_KP_HEAT_REFERENCE 0
#define RCN_KP_HEAT_SOFTMAX   1
/* bytes of LDS the NMS kernel may use for its status map (2 bits per pixel): images of up to 4 * this many pixels keep
 * the map in LDS, larger ones in HBM */
#define RCN_KP_LDS_STATUS_BYTES 131072
int rcn_kp_detect_device(rcn_ctx *ctx, const float *logits_dev, int64_t stride_img, int64_t stride_c, int64_t stride_y, int64_t stride_x,
                         int32_t n, int32_t H, int32_t W, int32_t heat_mode, double conf_thresh, int32_t nms_radius, int32_t border,
                         int32_t K, int32_t *kp_xy_dev /*[n][K][2]*/, float *conf_dev /*[n][K], may be NULL*/,
                         int32_t *counts_dev /*[n]*/, float *heat_out_dev /*[n][H][W], may be NULL*/, int32_t *rounds_dev /*[n], may be NULL*/);
/* The exact stages alone (threshold, NMS, border, cap) on heat maps the caller already has, [n][H][W] fp32. */
int rcn_kp_nms_device(rcn_ctx *ctx, const float *heat_dev /*[n][H][W]*/, int32_t n, int32_t H, int32_t W, double conf_thresh,
                      int32_t nms_radius, int32_t border, int32_t K, int32_t *kp_xy_dev, float *conf_dev, int32_t *counts_dev, int32_t *rounds_dev);
/* ---- SuperGlue's optimal-matching layer ----------------------------
 * What FeatureMatcherSuperglue::matchFeatures (FeatureMatcherSuperglue.cpp:51-101) runs behind the graph network: the
 * D-dimensional score matrix of the two sets of matching descriptors, the dustbin-augmented Sinkhorn iteration in the log
 * domain, the mutual-argmax selection and the two thresholds (the network's match_threshold, the reference's
 * matchScoreThreshold, :82).  B pairs per call, all in HBM, asynchronous on the ctx stream; the workspace (u, v, partial
 * column sums, the scores of rcn_sg_match_device) belongs to the ctx and grows: no host synchronisation once it has its size.
 *
 * For one pair with m rows of image 0 and n rows of image 1 (alpha = the learned bin_score):
 *   S[i][j] = (sum_d d0[i][d] d1[j][d]) / sqrt(D);  Z = S bordered by one row and one column of alpha (never materialised);
 *   norm = -log(m + n), log_mu[i] = norm, log_mu[m] = log(n) + norm, log_nu[j] = norm, log_nu[n] = log(m) + norm;  u = v = 0;
 *   `iterations` times: u[i] = log_mu[i] - logsumexp_j(Z[i][j] + v[j]), then v[j] = log_nu[j] - logsumexp_i(Z[i][j] + u[i]);
 *   logP = Z + u + v - norm.  On the inner m x n block: i0[i] = argmax_j, i1[j] = argmax_i, ties to the LOWEST index; row i is
 *   mutual iff i1[i0[i]] == i; mscores0[i] = exp(max_j logP[i][j]) if mutual else 0; matches0[i] = i0[i] if mutual and
 *   mscores0[i] > match_threshold, else -1; matches1 / mscores1 the same through i1.  table[i] = matches0[i] if also
 *   mscores0[i] > score_threshold, else -1: the std::map of the reference in the dense form of rcn_match_grid_device
 *   (table_stride >= M, tail -1, counts[b] = entries kept), consumed as it is by rcn_match_compact_begin.
 * All arithmetic is fp32 (expf / logf); the tolerance against the float64 statement is derived in DESIGN section 20.
 *
 * m_dev / n_dev: the pairs' counts in HBM (NULL: M resp. N for every pair); a count outside 0..M / 0..N is clamped on the
 * device.  Rows and columns past a pair's counts are padding: never read; their outputs are -1 / 0 (logP_out: 0).  A pair
 * with m == 0 or n == 0 runs no iteration and yields -1 / 0, count 0.  A pair whose final u or v holds a non-finite value
 * (non-finite scores) yields -1 / 0, count 0 and status 1; every other pair status 0.
 * logP_out: [B][M + 1][N + 1]; the dustbin row of a pair is row M, its dustbin column is column N, whatever m and n.
 *
 * Two device paths, chosen per pair from (m, n) and `path` alone, so that a pair's result never depends on its batch:
 *   fused   (m + 1)(n + 1) floats fit RCN_SG_LDS_BYTES: one workgroup loads the matrix once and iterates out of LDS;
 *   banded  otherwise: workgroups own bands of 8 rows; per iteration one sweep over the matrix (row logsumexp, and from the
 *           same resident band the partial column (max, sum) pairs), then a small launch that merges the partials in band
 *           order.  Pairs are processed in chunks whose matrices fit rcn_sg_set_chunk_bytes (cache residency; bytes <= 0:
 *           no limit, the default); results do not depend on the chunk size.
 * Each path is bit-reproducible; the two agree within the tolerance.  RCN_SG_PATH_FUSED is judged by the capacity: it
 * needs (M + 1)(N + 1) floats to fit (the counts live on the device), RCN_ERR_UNSUPPORTED otherwise.
 *
 * Descriptors: fp32, addressed by element strides (pair, row, d): the network's [B][D][K] output (the reference's featDescs
 * layout) is (D K, 1, K), row-major [B][K][D] is (K D, D, 1).  Products and sums in fp32, ascending d.
 * RCN_ERR_ARG: null required pointer, B < 0, M < 1, N < 1, D < 1, table_stride < M, a table without counts,
 * iterations < 0, a threshold outside [0, 1), non-finite alpha, unknown path.  RCN_ERR_UNSUPPORTED: M or N above
 * RCN_SG_MAX_POINTS.  B == 0 launches nothing. */
typedef struct { double alpha, match_threshold, score_threshold; int32_t iterations, path; } rcn_sg_options;
#define RCN_SG_PATH_AUTO   0
#define RCN_SG_PATH_FUSED  1
#define RCN_SG_PATH_BANDED 2
#define RCN_SG_LDS_BYTES  131072   /* a pair whose bordered matrix fits this many bytes of LDS takes the fused path */
#define RCN_SG_MAX_POINTS 4096     /* largest M and N */
void rcn_sg_default_options(rcn_sg_options *o);   /* alpha 1.0, thresholds 0.2 and 0.5, 100 iterations, RCN_SG_PATH_AUTO */
int rcn_sg_scores_device(rcn_ctx *ctx, const float *d0_dev, int64_t stride_pair0, int64_t stride_row0, int64_t stride_d0,
                         const float *d1_dev, int64_t stride_pair1, int64_t stride_row1, int64_t stride_d1,
                         const int32_t *m_dev /*[B] or NULL*/, const int32_t *n_dev /*[B] or NULL*/, int32_t B, int32_t M, int32_t N, int32_t D,
                         float *scores_out_dev /*[B][M][N]; padding is not written*/);
int rcn_sg_assign_device(rcn_ctx *ctx, const float *scores_dev, int64_t stride_pair, int64_t stride_row, int64_t stride_col,
                         const int32_t *m_dev /*[B] or NULL = M*/, const int32_t *n_dev /*[B] or NULL = N*/, int32_t B, int32_t M, int32_t N,
                         const rcn_sg_options *opt /*NULL = defaults*/, int32_t *matches0_dev /*[B][M]*/, int32_t *matches1_dev /*[B][N], may be NULL*/,
                         float *mscores0_dev /*[B][M], may be NULL*/, float *mscores1_dev /*[B][N], may be NULL*/,
                         int32_t *table_dev /*[B][table_stride], may be NULL*/, int64_t table_stride, int32_t *counts_dev /*[B], with table*/,
                         float *logP_out_dev /*[B][M+1][N+1], may be NULL: diagnostics and tests*/, int32_t *status_dev /*[B], may be NULL*/);
/* rcn_sg_scores_device into the ctx's workspace, then rcn_sg_assign_device on it: bit for bit the two calls. */
int rcn_sg_match_device(rcn_ctx *ctx, const float *d0_dev, int64_t stride_pair0, int64_t stride_row0, int64_t stride_d0,
                        const float *d1_dev, int64_t stride_pair1, int64_t stride_row1, int64_t stride_d1,
                        const int32_t *m_dev, const int32_t *n_dev, int32_t B, int32_t M, int32_t N, int32_t D, const rcn_sg_options *opt,
                        int32_t *matches0_dev, int32_t *matches1_dev, float *mscores0_dev, float *mscores1_dev,
                        int32_t *table_dev, int64_t table_stride, int32_t *counts_dev, float *logP_out_dev, int32_t *status_dev);
int rcn_sg_set_chunk_bytes(rcn_ctx *ctx, int64_t bytes);
/* ---- SuperGlue's attentional graph network, weights supplied -------
 * What matchFeatures runs in front of the layer above: normalizeFeatCoords (utils.cpp:119-149), the keypoint encoder, L self /
 * cross attention layers and the final projection (Sarlin et al., CVPR 2020, section 3.1).  The library ships no weights: the
 * caller hands over PLAIN linear layers (BatchNorm folded on the host: s = gamma / sqrt(var + 1e-5), W' = s W,
 * b' = s (b - mean) + beta; reconstructor_amd/superglue_gnn.py does it in float64), fp32, in one packed block:
 *   the encoder's five layers 3 -> 32 -> 64 -> 128 -> 256 -> 256, each W row-major [Cout][Cin] then b [Cout];
 *   per layer: q, k, v, merge (each W [256][256], b [256]), mlp0 (W [512][512] over [x; msg], b [512]), mlp1 (W [256][512], b [256]);
 *   the final projection W [256][256], b [256].
 * That is 109376 + 657152 L + 65792 floats; any other n_params is RCN_ERR_ARG.  Channels are in the published order: channel
 * c of q, k, v is head c % 4 at depth c / 4.  layer_types[l]: RCN_SG_LAYER_SELF or RCN_SG_LAYER_CROSS.  The block is copied;
 * a net belongs to its ctx and is destroyed before it.
 *
 * For one pair with m keypoints in image 0 and n in image 1 (D = 256, 4 heads of 64 channels, ReLU behind every encoder layer
 * but the last and behind mlp0):
 *   coordinates  with image shapes (H, W): cx = W / 2, cy = H / 2 in INTEGER division, scale = max(H, W) * 0.7 in double,
 *                k = (float)((x - c) / scale) in double -- the reference's rule; without shapes they are taken as they are;
 *   encoder      x = desc + MLP_enc([kx; ky; score]);
 *   layer l      src = x of the same image (self) or of the other (cross), both images from the values before the layer:
 *                q = Wq x + bq, k = Wk src + bk, v = Wv src + bv; per head P = softmax_j(q_i . k_j / 8), o_i = sum_j P_ij v_j;
 *                msg = Wm o + bm; x += W2 relu(W1 [x; msg] + b1) + b2;
 *   output       mdesc = Wf x + bf: the descriptors rcn_sg_scores_device takes with D = 256; alpha is bin_score.
 * Storage and arithmetic are fp32 (products on the fp32-input matrix instructions: fmaf chains in a fixed order); the tolerance
 * against the float64 statement is derived in DESIGN section 21.  A pair's result is bit for bit the same alone, in any batch
 * and under any chunking.
 *
 * kpts [B][M][2] (x, y) and scores [B][M] for image 0, [B][N][2] and [B][N] for image 1; descriptors by element strides (pair,
 * row, d) as in rcn_sg_scores_device; shape0 / shape1: [B][2] int32 (H, W) in HBM, both or neither; m_dev / n_dev as above.
 * mdesc0_out [B][M][256], mdesc1_out [B][N][256].  A pair with m == 0 or n == 0 computes nothing and its mdesc is not written;
 * points past a pair's counts are never read and never written.  Non-finite inputs propagate (the status of the layer above
 * reports them).  The activations (8 KiB per point) live in the ctx's workspace; pairs are processed in chunks under a fixed
 * cap of that workspace, or rcn_sg_net_set_chunk_pairs pairs at a time (<= 0: the default); the result does not depend on it.
 * RCN_ERR_ARG: null required pointer, a net of another ctx, B < 0, M < 1, N < 1, shapes for one side only, and for
 * rcn_sg_net_create a layer count outside 0..1024, an unknown layer type, a wrong n_params, a non-finite bin_score.
 * RCN_ERR_UNSUPPORTED: D != 256, M or N above RCN_SG_MAX_POINTS.  B == 0 launches nothing. */
typedef struct rcn_sg_net rcn_sg_net;
#define RCN_SG_LAYER_SELF  0
#define RCN_SG_LAYER_CROSS 1
int  rcn_sg_net_create(rcn_ctx *ctx, const int32_t *layer_types /*[n_layers]*/, int32_t n_layers, const float *params_host, int64_t n_params,
                       double bin_score, rcn_sg_net **net_out);
void rcn_sg_net_destroy(rcn_sg_net *net);
int  rcn_sg_net_set_chunk_pairs(rcn_ctx *ctx, int32_t pairs);
int  rcn_sg_net_forward_device(rcn_ctx *ctx, const rcn_sg_net *net, const float *kpts0_dev, const float *scores0_dev, const float *d0_dev,
                               int64_t stride_pair0, int64_t stride_row0, int64_t stride_d0, const float *kpts1_dev, const float *scores1_dev,
                               const float *d1_dev, int64_t stride_pair1, int64_t stride_row1, int64_t stride_d1,
                               const int32_t *shape0_dev /*[B][2] or NULL*/, const int32_t *shape1_dev, const int32_t *m_dev, const int32_t *n_dev,
                               int32_t B, int32_t M, int32_t N, int32_t D, float *mdesc0_out_dev, float *mdesc1_out_dev);
/* The forward into the ctx's workspace, then rcn_sg_match_device on it with alpha = bin_score (opt->alpha is ignored): bit for
 * bit the two calls; outputs and their errors as there. */
int  rcn_sg_net_match_device(rcn_ctx *ctx, const rcn_sg_net *net, const float *kpts0_dev, const float *scores0_dev, const float *d0_dev,
                             int64_t stride_pair0, int64_t stride_row0, int64_t stride_d0, const float *kpts1_dev, const float *scores1_dev,
                             const float *d1_dev, int64_t stride_pair1, int64_t stride_row1, int64_t stride_d1,
                             const int32_t *shape0_dev, const int32_t *shape1_dev, const int32_t *m_dev, const int32_t *n_dev,
                             int32_t B, int32_t M, int32_t N, int32_t D, const rcn_sg_options *opt,
                             int32_t *matches0_dev, int32_t *matches1_dev, float *mscores0_dev, float *mscores1_dev,
                             int32_t *table_dev, int64_t table_stride, int32_t *counts_dev, float *logP_out_dev, int32_t *status_dev);
/* ---- SuperPoint's convolutional network, weights supplied -----------
 * The forward pass of FeatureSuperPoint::detect (FeatureSuperPoint.cpp:228-263, superNet.forward): image in, the two outputs
 * the keypoint and descriptor stages above take.  DeTone et al., CVPR-W 2018.  The library ships no weights: the caller hands
 * over one packed fp32 block of RCN_SP_N_PARAMS floats in the order
 *   conv1a 1->64, conv1b 64->64, conv2a 64->64, conv2b 64->64, conv3a 64->128, conv3b 128->128, conv4a 128->128, conv4b 128->128,
 *   convPa 128->256, convPb 256->65 (1 x 1), convDa 128->256, convDb 256->256 (1 x 1),
 * each layer W row-major [Cout][Cin][3][3] ([Cout][Cin] for 1 x 1), then b [Cout].  The block is copied (and laid out anew for
 * the kernels); a net belongs to its ctx and is destroyed before it.
 *
 * For one grey image [H][W] in [0, 1], H and W positive multiples of 8, Hc = H / 8, Wc = W / 8:
 *   encoder     conv1a, conv1b, pool, conv2a, conv2b, pool, conv3a, conv3b, pool, conv4a, conv4b; every convolution 3 x 3,
 *               stride 1, zero padding 1, plus bias, then ReLU; pool is 2 x 2 max, stride 2;
 *   detector    logits = convPb(relu(convPa(x))), [Hc][Wc][65];
 *   descriptor  d = convDb(relu(convDa(x))), [Hc][Wc][256]; with RCN_SP_NORMALIZE_DESC every cell is divided by its L2 norm:
 *               the fp32 sum of the squares in ascending channel order, sqrtf, fp32 division (a zero cell gives NaN).
 * Storage and arithmetic are fp32 (products on the fp32-input matrix instructions: fmaf chains in a fixed order); the tolerance
 * against the float64 statement is derived in DESIGN section 22.  An image's result is bit for bit the same alone, in any
 * batch, under any chunking and from any strides.
 *
 * images_dev: n images addressed by ELEMENT strides (image, y, x); RCN_SP_INPUT_F32: float; RCN_SP_INPUT_U8: bytes, a pixel
 * is (float)((double)v / 255.0), prepImg's rule (:278-285).  Both outputs are channel-last and dense: what
 * rcn_kp_detect_device reads with strides (Hc Wc 65, 1, Wc 65, 65) and rcn_desc_sample_batch_device with (Hc Wc 256, 1,
 * Wc 256, 256).  The activations (320 bytes per pixel) live in the ctx's workspace; images are processed in chunks under a
 * fixed cap of that workspace (one image always fits: the workspace grows), or rcn_sp_net_set_chunk_images images at a time
 * (<= 0: the default).  Non-finite inputs propagate.
 * RCN_ERR_ARG: null required pointer, a net of another ctx, n < 0, H or W no positive multiple of 8, H * W > 2^31 - 1, an
 * unknown dtype or flag bit, a wrong n_params.  n == 0 launches nothing. */
typedef struct rcn_sp_net rcn_sp_net;
#define RCN_SP_N_PARAMS 1300865
#define RCN_SP_NORMALIZE_DESC 1          /* flags */
#define RCN_SP_INPUT_F32 0
#define RCN_SP_INPUT_U8  1
int  rcn_sp_net_create(rcn_ctx *ctx, const float *params_host, int64_t n_params, rcn_sp_net **net_out);
void rcn_sp_net_destroy(rcn_sp_net *net);
int  rcn_sp_net_set_chunk_images(rcn_ctx *ctx, int32_t images);
int  rcn_sp_net_forward_device(rcn_ctx *ctx, const rcn_sp_net *net, const void *images_dev, int32_t input_dtype,
                               int64_t stride_img, int64_t stride_y, int64_t stride_x, int32_t n, int32_t H, int32_t W, int32_t flags,
                               float *logits_out_dev /*[n][Hc][Wc][65]*/, float *desc_out_dev /*[n][Hc][Wc][256]*/);
/* The forward into the ctx's workspace, then rcn_kp_detect_device and rcn_desc_sample_batch_device on it: bit for bit the
 * three calls.  Keypoint arguments, outputs and their errors as there; rows_out_dev [n][K][D]. */
int  rcn_sp_net_detect_device(rcn_ctx *ctx, const rcn_sp_net *net, const void *images_dev, int32_t input_dtype,
                              int64_t stride_img, int64_t stride_y, int64_t stride_x, int32_t n, int32_t H, int32_t W, int32_t flags,
                              int32_t heat_mode, double conf_thresh, int32_t nms_radius, int32_t border, int32_t K, int32_t D,
                              int32_t *kp_xy_dev, float *conf_dev, int32_t *counts_dev, float *rows_out_dev /*[n][K][D]*/,
                              float *heat_out_dev /*may be NULL*/, int32_t *rounds_dev /*may be NULL*/);
/* Host-side batch ingest: n_images images with their own row counts K[i] >= 0, each a dense row-major K[i] x D
 * fp32 matrix in HOST memory (rows[i]; what featDescToCV packs per call, FeatureMatcher.cpp:11-25 -- here for every
 * image of the loop at once), become ids first_img_id .. first_img_id + n_images - 1.  One device block of
 * [n][max K][D] owned by the ctx (tails zeroed), one asynchronous copy per image straight out of the caller's rows
 * (pinned rows -- rcn_host_alloc -- travel at the link rate; pageable rows are staged by the runtime), ONE stats
 * launch, ONE conversion launch at the next grid call, ONE host synchronisation before the call returns: the host
 * rows are borrowed for the call only.  Calling it again with the same (first id, n, max K, D) reuses every
 * allocation.  Replaces n synchronous rcn_desc_upload calls (each of which waits for its own copy). */
int rcn_desc_upload_batch(rcn_ctx *ctx, int32_t first_img_id, int32_t n_images, const float *const *rows_host,
                          const int32_t *K, int32_t D);
/* Forget one image (no-op when the id is not resident).  Other resident images, and their D, stay. */
int rcn_desc_remove(rcn_ctx *ctx, int32_t img_id);
int rcn_desc_clear(rcn_ctx *ctx);
int rcn_desc_count(const rcn_ctx *ctx);

/* ---- matching --------------------------------------------------------------------------
 * Result of one (query image, train image) pair: out[i] = train row matched to query row i,
 * or -1.  This is the std::map<int,int> FlannMatcher::matchFeatures fills
 * (FeatureMatcher.cpp:53-64) in dense form: exact 2-NN under L2, ratio test
 * dist0 < ratio * dist1 in fp32, then the lowest query index keeps a contested train row.
 * K2 < 2 yields no matches (the reference reads knn[i][1] unconditionally there).          */

/* One pair straight from host rows (the per-call shape of FeatureMatcher::matchFeatures). */
int rcn_match_pair(rcn_ctx *ctx, const float *q_host, int32_t K1,
                   const float *t_host, int32_t K2, int32_t D, float ratio,
                   int32_t *out_train_for_query /* K1 */, int32_t *out_count);

/* Pair grid over resident images (SequentialReconstructor.cpp:199-279).  pairs = n_pairs x
 * (query image id, train image id) on the HOST.  out = n_pairs rows of out_stride int32 on
 * the HOST (out_stride >= K of every query image; tail of each row is set to -1),
 * counts[p] = matches of pair p.  pairs_host == NULL: the reference's canonical grid, every
 * i < j over the resident image ids in ascending order; n_pairs must then be n (n - 1) / 2.  */
int rcn_match_grid(rcn_ctx *ctx, const int32_t *pairs_host, int32_t n_pairs, float ratio,
                   int32_t *out_host, int64_t out_stride, int32_t *counts_host);

/* Same, results left in HBM: out_dev / counts_dev are DEVICE pointers; asynchronous on the
 * ctx stream (no host synchronisation inside once the workspace has reached its size).     */
int rcn_match_grid_device(rcn_ctx *ctx, const int32_t *pairs_host, int32_t n_pairs, float ratio,
                          int32_t *out_dev, int64_t out_stride, int32_t *counts_dev);

/* ---- matching 256-bit rows under the Hamming distance ------------------------------------------
 * cv::BFMatcher(NORM_HAMMING).knnMatch(k = 2) behind the same ratio test and uniqueness, for ORB's packed rows (bytes_out_dev of
 * rcn_orb_describe_device / rcn_orb_detect_and_compute_device).  Everything is integer: d(i, j) = popcount(q_i XOR t_j) in 0 .. 256,
 * train rows ordered by (d, j) ascending (a tie goes to the lower train row, for the best and the second neighbour), the test
 * float(d0) < ratio * float(d1) in fp32 (d0 == d1 never passes), the lowest passing query row keeps a contested train row, fewer than two
 * train rows give no matches.  n_bytes must be 32 (RCN_ERR_ARG otherwise), K at most 32768 rows per image (RCN_ERR_ARG, nothing allocated).
 *
 * The binary rows are a residency of their own beside the float descriptors of rcn_desc_*: uploading or clearing one set leaves the other
 * untouched.  The ids are the same image ids (rcn_coords_upload, the epipolar filter and the match lists apply as they are).
 *   rcn_bits_upload               K rows of n_bytes from HOST memory as image img_id (replaces it); waits for its copy.
 *   rcn_bits_upload_batch_device  n_images images of K row slots each from DEVICE memory, bytes_dev [n][K][n_bytes]; image i has
 *                                 clamp(counts_dev[i], 0, K) rows (counts_dev == NULL: K each; ORB's counts, which may exceed K or be -1,
 *                                 are taken as they are, on the device: no host round trip).  Rows past that never take part, whatever
 *                                 bytes they hold.  The rows are copied (expanded to one int8 per bit, 256 bytes per row, resident in the
 *                                 ctx); asynchronous on the ctx stream.
 *   rcn_bits_remove / rcn_bits_clear / rcn_bits_count   as rcn_desc_remove / rcn_desc_clear / rcn_desc_count.
 * rcn_match_pair_hamming: one pair straight from host rows.  rcn_match_grid_hamming / rcn_match_grid_hamming_device: the dense table of
 * rcn_match_grid / rcn_match_grid_device over the resident binary rows (out[p][i] = train row or -1, the tail up to out_stride -1,
 * counts[p]; out_stride >= K of every query image; pairs_host == NULL: every i < j over the resident binary ids, n_pairs = n (n - 1) / 2);
 * rcn_match_compact_begin, rcn_match_table_filter_device and rcn_match_lists_upload take the table unchanged.
 * rcn_hamming_knn2_device: the two neighbours themselves, knn_dev [n_pairs][stride][4] = (j0, d0, j1, d1) per query row, -1 where
 * absent (rows past the query image's, a train image with fewer rows); stride >= K of every query image.
 * The top-2 workspace is chunked over pairs by rcn_match_set_workspace_rows (at most 2^25 row slots per chunk); the result does not
 * depend on the chunking.  RCN_ERR_NOT_FOUND: an image id without resident binary rows. */
int rcn_bits_upload(rcn_ctx *ctx, int32_t img_id, const uint8_t *bytes_host, int32_t K, int32_t n_bytes);
int rcn_bits_upload_batch_device(rcn_ctx *ctx, int32_t first_img_id, int32_t n_images, const uint8_t *bytes_dev /*[n][K][n_bytes]*/,
                                 const int32_t *counts_dev /*[n], NULL = K each*/, int32_t K, int32_t n_bytes);
int rcn_bits_remove(rcn_ctx *ctx, int32_t img_id);
int rcn_bits_clear(rcn_ctx *ctx);
int rcn_bits_count(const rcn_ctx *ctx);
int rcn_match_pair_hamming(rcn_ctx *ctx, const uint8_t *q_host, int32_t K1, const uint8_t *t_host, int32_t K2, int32_t n_bytes, float ratio,
                           int32_t *out_train_for_query /* K1 */, int32_t *out_count);
int rcn_match_grid_hamming(rcn_ctx *ctx, const int32_t *pairs_host, int32_t n_pairs, float ratio,
                           int32_t *out_host, int64_t out_stride, int32_t *counts_host);
int rcn_match_grid_hamming_device(rcn_ctx *ctx, const int32_t *pairs_host, int32_t n_pairs, float ratio,
                                  int32_t *out_dev, int64_t out_stride, int32_t *counts_dev);
int rcn_hamming_knn2_device(rcn_ctx *ctx, const int32_t *pairs_host, int32_t n_pairs, int32_t *knn_dev, int64_t stride);

/* ---- host materialisation of a match table ------------------------------------------------
 * The (query feature, train feature) lists the pair loop keeps in featureMatches
 * (SequentialReconstructor.cpp:260-267, :272-275), for a table rcn_match_grid_device (or
 * rcn_shard_match, rcn_match_table_filter_device) left in HBM: compacted on the GPU, then copied to
 * host memory.  Pair p owns entries offsets[p] .. offsets[p+1]-1 of qt, each two int32 (query row,
 * train row), ascending query row -- the iteration order of the reference's std::map<int,int>.
 *
 * rcn_match_compact_begin: compacts on the ctx stream, waits until the device knows the total,
 * fills offsets_host (n_pairs + 1 entries) and *total_out, starts the copy of the lists into qt_host
 * on the ctx's copy stream and returns; the copy overlaps whatever is enqueued on the ctx stream
 * next (two device staging buffers alternate).  qt_host should be pinned (rcn_host_alloc) for a true
 * DMA; capacity = entries qt_host can hold (RCN_ERR_ARG with *total_out set when it is too small).
 * rcn_match_compact_wait: the lists of the last begin have landed.                              */
int  rcn_host_alloc(void **out, size_t bytes);      /* pinned host memory; usable without a ctx once a device exists */
void rcn_host_free(void *p);
int  rcn_match_compact_begin(rcn_ctx *ctx, const int32_t *table_dev, int64_t stride, const int32_t *counts_dev,
                             int32_t n_pairs, int64_t *offsets_host, int32_t *qt_host, int64_t capacity,
                             int64_t *total_out);
int  rcn_match_compact_wait(rcn_ctx *ctx);

/* Statistics of the last grid call (diagnostics; rows_total = sum of K1 over pairs). */
typedef struct {
    int64_t rows_total;
    int64_t rows_reranked;        /* query rows whose two candidates were re-computed exactly (fp64) */
    int64_t rows_exact_fallback;  /* query rows the coarse pass and the re-rank could not certify: middle tier (fp32 sweep shared by the rows
                                     of a train image -> a handful of candidates -> fp64 chain), K2b (every train row in fp64) behind it */
    int64_t pair_distances;       /* sum of K1*K2 */
    double  err_bound_d2;         /* largest certified bound on |coarse - exact| squared distance */
    int32_t used_mfma_path;       /* 1 = fp16 MFMA coarse pass + exact re-rank, 0 = exact kernel only */
    int32_t profiled_calls;       /* grid calls summed into the *_ms fields (rcn_match_profile) */
    double  coarse_ms;            /* HIP-event time of k_coarse_top2 launches, summed */
    double  rerank_ms;            /* k_rerank + k_exact_rows */
    double  unique_ms;            /* k_unique_claim + k_unique_emit */
    int64_t rows_brute_force;     /* of rows_exact_fallback: rows that went through K2b after all (candidate list overflowed, budget exceeded, D % 4 != 0) */
    int32_t chunks;               /* pipeline chunks of the last grid call (candidate table / row lists are sized per chunk) */
    int32_t coarse_launches;      /* coarse-kernel launches summed into coarse_ms (chunks x profiled calls) */
    int32_t coarse_dtype;         /* number format of the coarse pass of the last grid call: 0 none (exact kernels only), 1 fp16 MFMA, 2 int8 MFMA
                                   * (D padded to 256, at most 4096 padded rows per image, rows not peaked: DESIGN.md section 5) */
    int32_t reserved0;
} rcn_match_stats;
int rcn_match_last_stats(const rcn_ctx *ctx, rcn_match_stats *out);
/* enable != 0: bracket the kernels of every following grid call with HIP events on the ctx
 * stream (up to 64 calls are kept); rcn_match_last_stats sums and clears them. */
int rcn_match_profile(rcn_ctx *ctx, int enable);
/* Workspace budget of the grid calls: query-row slots of the candidate table per pipeline chunk (8 bytes per slot, plus two row lists of
 * at most as many entries).  Default (rows = 0): 2^27 slots = 1 GiB of candidates -- cfg 3 (2.05e9 query rows) then runs in sixteen chunks
 * that reuse the workspace, at +0.2 % of K1's time against one 16-GiB chunk (same-box A/B in the bench line, `roofline.chunk_ab`). */
int rcn_match_set_workspace_rows(rcn_ctx *ctx, int64_t rows);

/* ---- pair grid sharded over the GPUs of one node -----------------------------------------
 * The N x N loop of SequentialReconstructor::matchFeatures (SequentialReconstructor.cpp:202-279) runs
 * its pairs as independent units (OpenMP collapse(2)); here they are spread over several GPUs, one
 * rcn_shard (= one rcn_ctx + RCCL communicators, called directly over xGMI) per GPU, in one process
 * per GPU or in one process with a host thread per GPU (reconstructor_amd/host/HipPairGridDriver.h).
 *   images  equal contiguous blocks: rank r owns ids [r*per, min(n, (r+1)*per)), per = ceil(n / world)
 *   pairs   the canonical i < j list (row-major) dealt round-robin: pair number p belongs to rank p % world
 *   exchange  local row statistics -> ncclAllReduce(max) of the two scale statistics -> fp16 conversion of
 *             the LOCAL block -> in-place ncclAllGather of fp16 rows + half-norms + norms (ctx stream);
 *             ncclAllGather of the fp32 rows on a side stream (read only by the exact re-rank stages)
 * Every rank converts with the same global scale: tables are bit-identical to a one-GPU run.     */
typedef struct rcn_shard rcn_shard;
#define RCN_SHARD_ID_BYTES 128            /* sizeof(ncclUniqueId) */

/* Partition: pure host functions (no GPU, no communicator). */
int     rcn_shard_owned_images(int32_t n_images, int32_t world, int32_t rank, int32_t *first, int32_t *count);
int64_t rcn_shard_pair_count(int32_t n_images, int32_t world, int32_t rank);
int     rcn_shard_pairs(int32_t n_images, int32_t world, int32_t rank, int32_t *pairs_out /* 2 x count */);

/* Rendezvous: ONE rank (or the single process) draws the id, the host hands it to every rank
 * (environment, file, MPI, torch store ...); rcn_shard_create is collective over the world. */
int      rcn_shard_unique_id(uint8_t id[RCN_SHARD_ID_BYTES]);
int      rcn_shard_create(rcn_ctx *ctx, int32_t rank, int32_t world, const uint8_t id[RCN_SHARD_ID_BYTES],
                          rcn_shard **out);
void     rcn_shard_destroy(rcn_shard *sh);   /* also drops the ctx's resident descriptors (views into the landing buffer) */
rcn_ctx *rcn_shard_ctx(rcn_shard *sh);

/* Shape of the next exchanges: n_images over all ranks, each K x D fp32.  *local_slot_dev (may be NULL)
 * receives this rank's block of the landing buffer, [count][K][D] fp32 in HBM: a detector can write its
 * rows straight there (the producer contract, see rcn_desc_upload_batch_device) and pass NULL to
 * rcn_shard_exchange.  The pointer stays valid until a reserve with another shape. */
int rcn_shard_reserve(rcn_shard *sh, int32_t n_images, int32_t K, int32_t D, float **local_slot_dev);
/* Host rows of ONE owned image into its slot (featDescToCV's gather, FeatureMatcher.cpp:11-25, done once per
 * image): K_img <= K rows are copied, the rest of the slot is zero-filled, K_img is remembered for the exchange. */
int rcn_shard_put_image(rcn_shard *sh, int32_t img_id, const float *desc_host, int32_t K_img);
/* Collective.  local_desc_dev: this rank's [count][K][D] fp32 block in HBM (copied), or NULL when the rows are
 * already in the slot.  local_K: rows in use per owned image (count entries, each <= K; tails are zeroed), or
 * NULL = what rcn_shard_put_image recorded, K for untouched slots.  Afterwards ids 0 .. n_images-1 are resident
 * in the shard's ctx, image i with its own row count.  One host wait when every slot of every rank is full, two
 * when some rank's images are ragged (the row counts are then gathered too). */
int rcn_shard_exchange(rcn_shard *sh, const float *local_desc_dev, const int32_t *local_K);
/* This rank's share of the canonical grid (rcn_shard_pairs order); out_dev / counts_dev as rcn_match_grid_device
 * (out_stride >= K).  Both NULL: the tables stay in buffers owned by the ctx, for rcn_shard_lists. */
int rcn_shard_match(rcn_shard *sh, float ratio, int32_t *out_dev, int64_t out_stride, int32_t *counts_dev);
/* Host lists of the last rcn_shard_match(sh, ratio, NULL, 0, NULL): rcn_match_compact_begin + _wait on the shard's
 * own tables (same arguments and the same behaviour when capacity is too small: *total_out tells how many). */
int rcn_shard_lists(rcn_shard *sh, int64_t *offsets_host, int32_t *qt_host, int64_t capacity, int64_t *total_out);

/* The lists of EVERY rank on one rank: the single featureMatches map the reference keeps
 * (SequentialReconstructor.cpp:224,264,274).  Collective.  table_dev / stride / counts_dev: this rank's tables of the last
 * rcn_shard_match (all three NULL / 0: the shard's own tables, after rcn_shard_match(sh, ratio, NULL, 0, NULL), filtered
 * or not).  Every rank compacts its tables on the GPU; the totals and the per-pair counts are all-gathered (one bounded host
 * wait); the lists travel to `root` device to device (ncclSend / ncclRecv over xGMI), are put in canonical pair order on
 * the root's GPU (pair number p of the row-major i < j list: offsets_host[p] .. offsets_host[p + 1]) and reach the root's
 * host memory in ONE copy.  offsets_host (n(n-1)/2 + 1 entries), qt_host, capacity and *total_out are read on the root only
 * (other ranks may pass NULL / 0); a capacity that is too small fails on every rank together with *total_out set on the
 * root.  rcn_shard_merge_lists is the same merge for lists that are already in host memory (per-rank results of
 * rcn_shard_lists, gathered by whatever the host has): pure host code, no GPU, no communicator. */
int rcn_shard_gather_lists(rcn_shard *sh, int32_t root, const int32_t *table_dev, int64_t stride, const int32_t *counts_dev,
                           int64_t *offsets_host, int32_t *qt_host, int64_t capacity, int64_t *total_out);
int rcn_shard_merge_lists(int32_t n_images, int32_t world, const int64_t *const *offsets_per_rank, const int32_t *const *qt_per_rank,
                          int64_t *offsets_out, int32_t *qt_out, int64_t capacity, int64_t *total_out);

typedef struct {
    int32_t rank, world, n_images, images_per_rank;
    int64_t n_pairs;              /* this rank's share */
    int64_t exchange_bytes_f16;   /* whole all-gather (all ranks' blocks): fp16 rows + half-norms + norms */
    int64_t exchange_bytes_f32;   /* whole all-gather of the fp32 rows (side stream) */
    int32_t comm_ranks;           /* ncclCommCount of the communicator the collectives run on */
    int32_t reserved;
} rcn_shard_stats;
int rcn_shard_info(const rcn_shard *sh, rcn_shard_stats *out);

/* Failure handling.  The collectives after rcn_shard_create are rcn_shard_exchange and rcn_shard_gather_lists, and both open
 * with a status vote: an all-gather of a few words per rank (status, shape, "my block is ragged") in front of the first
 * host wait.  Every allocation of the call happens BEFORE the vote.  A failure that only THIS rank saw -- rcn_shard_reserve
 * could not allocate, rcn_shard_put_image was refused, or the host driver reports one of its own through rcn_shard_fail --
 * is remembered in the shard; the rank must still call rcn_shard_exchange, which then returns an error on EVERY rank (the
 * failing rank its own code, the others RCN_ERR_COMM naming it) before any further collective is entered, so no peer is
 * left waiting.  Ranks that reserved different shapes fail the same way.  rcn_shard_match refuses to run until an exchange
 * has gone through again.
 *   Behind the vote nothing allocates and nothing returns early: a HIP error there is recorded, the remaining collectives
 * are still entered, the call returns the error to this caller and the peers hear of it in the NEXT vote.  An RCCL call that
 * refuses to queue leaves the peers without a partner; the communicators are then aborted (ncclCommAbort).
 *   The host never waits for a collective without a limit: every wait of the shard API polls, watches
 * ncclCommGetAsyncError and gives up after rcn_shard_set_timeout seconds (default 600) -- it then aborts both communicators,
 * and the shard is dead: every later call returns RCN_ERR_COMM at once (destroy it and create a new one).  A peer that
 * crashed or walked away therefore costs a timeout, never a hang. */
int rcn_shard_fail(rcn_shard *sh, int32_t code /* negative RCN_ERR_* */);
int rcn_shard_set_timeout(rcn_shard *sh, double seconds);

/* Phase times of the sharded step, HIP events on the streams the work runs on: enable, run steps (at most 64 are
 * kept), read the sums (waits for the shard's streams; clears them). */
typedef struct {
    int32_t exchanges, matches;   /* calls summed below */
    double  exchange_ms;          /* rcn_shard_exchange on the ctx stream: vote + counts, statistics, all-reduce, fp16 conversion, fp16 all-gather */
    double  f32_gather_ms;        /* all-gather of the fp32 rows on the side stream (beside the coarse kernel) */
    double  match_ms;             /* rcn_shard_match: this rank's share of the grid */
} rcn_shard_times;
int rcn_shard_profile(rcn_shard *sh, int enable);
int rcn_shard_profile_read(rcn_shard *sh, rcn_shard_times *out);

/* ---- bundle adjustment -----------------------------------------------------------------
 * Flat form of what BundleAdjuster::adjust packs (BundleAdjuster.cpp:17-97):
 *   poses      n_cams x 6   angle-axis * angle, translation   (world -> camera, :46-59)
 *   intrinsics n_cams x 6   fx fy cx cy k1 k2                 (:37-42)
 *   points     n_points x 3                                   (:65-70)
 *   observations landmark-major (:74-97): obs_pt non-decreasing.
 * Camera index = position in imgIdxOrder.  All three parameter arrays are updated in place. */
typedef struct {
    int32_t        n_cams, n_points, n_obs, reserved;
    double        *poses;
    double        *intrinsics;
    double        *points;
    const double  *obs_uv;    /* n_obs x 2 (integer pixel coordinates cast to double, :83-84) */
    const int32_t *obs_cam;   /* n_obs */
    const int32_t *obs_pt;    /* n_obs, non-decreasing */
} rcn_ba_problem;

typedef struct {
    int32_t max_iterations;        /* 150 if n_cams < 10 else 50           (BundleAdjuster.cpp:135-142) */
    int32_t intrinsics_mode;       /* 0: all intrinsics constant (n_cams<10, :112-115);
                                      1: cx,cy constant, fx,fy upper-bounded (:117-121) */
    int32_t fix_cam0_pose;         /* 1                                     (:100-101) */
    int32_t fix_cam1_translation;  /* 1                                     (:104-105) */
    double  focal_upper_bound;     /* 1000                                  (:120-121) */
    /* Ceres 2.x trust-region defaults (solver.h), none overridden by the reference */
    double  initial_trust_region_radius;   /* 1e4  */
    double  max_trust_region_radius;       /* 1e16 */
    double  min_trust_region_radius;       /* 1e-32 */
    double  min_relative_decrease;         /* 1e-3 */
    double  min_lm_diagonal;               /* 1e-6 */
    double  max_lm_diagonal;               /* 1e32 */
    double  function_tolerance;            /* 1e-6 */
    double  gradient_tolerance;            /* 1e-10 */
    double  parameter_tolerance;           /* 1e-8 */
    int32_t max_consecutive_invalid_steps; /* 5 */
    int32_t jacobi_scaling;                /* 1 */
} rcn_ba_options;

/* Fills the options exactly as BundleAdjuster::adjust + Ceres defaults would for n_cams. */
void rcn_ba_default_options(int32_t n_cams, rcn_ba_options *out);

#define RCN_BA_CONVERGENCE_FUNCTION   1
#define RCN_BA_CONVERGENCE_GRADIENT   2
#define RCN_BA_CONVERGENCE_PARAMETER  3
#define RCN_BA_CONVERGENCE_RADIUS     4
#define RCN_BA_NO_CONVERGENCE         5   /* max_iterations reached */
#define RCN_BA_FAILURE                6   /* too many consecutive invalid steps */

typedef struct {
    double  initial_cost;       /* 1/2 sum r^2 at the input */
    double  final_cost;
    double  initial_rms_px;     /* sqrt(sum r^2 / n_obs) */
    double  final_rms_px;
    int32_t iterations;         /* LM iterations attempted (successful + unsuccessful) */
    int32_t successful_steps;
    int32_t unsuccessful_steps;
    int32_t invalid_steps;
    int32_t termination;        /* RCN_BA_* */
    int32_t line_search_backtracks; /* backtracks of the projected Armijo search (bounds present: >= 10 cameras) */
    int32_t bound_projections;  /* focal lengths clamped to their upper bound by a Plus */
    int32_t reduced_dim;        /* rows of the reduced camera system */
    int32_t pair_lists_reused;  /* 1: the Schur build's observation-pair lists were still valid (rcn_ba_session_solve on an unchanged graph;
                                   rcn_ba_solve called again with the observation arrays of its last call, compared element by element) */
    int32_t reserved;
    double  solve_seconds;      /* wall time of the solve, inputs resident: pair lists of the Schur build + the LM loop */
    double  schur_seconds;      /* HIP-event time, summed over iterations: point blocks + Schur build */
    double  cholesky_seconds;   /* dense factorisation of the reduced system */
    double  trisolve_seconds;   /* triangular solves + back-substitution + model/candidate evaluation */
    double  cost_trace[160];    /* cost after each iteration, [0] = initial */
    double  jacobian_seconds;   /* HIP-event time of the residual + Jacobian kernel (k_ba_eval<true>: 224 B written per observation), summed */
    int32_t jacobian_evals;     /* launches summed into jacobian_seconds */
    int32_t factor_schedule;    /* 0: the factorisations ran on three streams; 1: on one stream in program order (a cross-stream
                                   wait gave up -- a runtime that does not run the streams side by side -- and the context
                                   latched the one-stream schedule; same bits either way) */
} rcn_ba_summary;

int rcn_ba_solve(rcn_ctx *ctx, const rcn_ba_problem *problem, const rcn_ba_options *options,
                 rcn_ba_summary *summary);

/* Robust losses.  The reference hands Ceres no loss (BundleAdjuster.cpp:89-93) and rcn_ba_solve means exactly that; the first
 * thing a Ceres user switches on with real photographs is a HuberLoss or a CauchyLoss, and rcn_ba_solve_robust is that argument.
 * The cost becomes 1/2 sum_o rho(s_o), s_o = r0^2 + r1^2 of observation o's residual in pixels^2, a = scale > 0 in pixels, b = a^2:
 *   RCN_BA_LOSS_TRIVIAL  rho = s
 *   RCN_BA_LOSS_HUBER    rho = s for s <= b, else 2 a sqrt(s) - b
 *   RCN_BA_LOSS_SOFT_L1  rho = 2 b (sqrt(1 + s/b) - 1)
 *   RCN_BA_LOSS_CAUCHY   rho = b log(1 + s/b)
 * A restatement of Ceres' loss functions and Corrector from memory: PARITY WITH CERES IS UNPINNED.  All three have rho'' <= 0, so the
 * corrector scales the residual and the Jacobian of an observation by sqrt(rho'(s)), rho' clamped from below at DBL_MIN, and nothing
 * else; the line search (intrinsics_mode 1) takes the robust cost and sum_o rho'(s_o) r_o . (J_o d).
 * With a loss, rcn_ba_summary's initial_cost, final_cost and cost_trace are ROBUST costs, and initial_rms_px / final_rms_px stay
 * sqrt(2 cost / n_obs) of them: not a residual RMS any more -- rcn_ba_loss_report::plain_rms_px is.
 * loss == NULL or RCN_BA_LOSS_TRIVIAL: rcn_ba_solve, bit for bit (the same kernels).  RCN_ERR_ARG with a message: an unknown kind, a
 * scale that is not finite, a scale that is not positive under a non-trivial kind. */
#define RCN_BA_LOSS_TRIVIAL 0
#define RCN_BA_LOSS_HUBER   1
#define RCN_BA_LOSS_SOFT_L1 2
#define RCN_BA_LOSS_CAUCHY  3
typedef struct { int32_t kind; int32_t reserved; double scale; } rcn_ba_loss;
/* One pass over the observations at the solve's final point, on the unweighted residuals. */
typedef struct {
    int64_t n_obs, n_beyond_scale;              /* n_beyond_scale: observations with s > scale^2 (0 without a loss) */
    double  plain_rms_px, max_residual_px;      /* sqrt(sum s / n_obs), sqrt(max s) */
} rcn_ba_loss_report;
/* loss, report and weights_host may each be NULL; weights_host: n_obs doubles, rho'(s_o) per observation (1 without a loss). */
int rcn_ba_solve_robust(rcn_ctx *ctx, const rcn_ba_problem *problem, const rcn_ba_options *options, const rcn_ba_loss *loss,
                        rcn_ba_summary *summary, rcn_ba_loss_report *report, double *weights_host);

/* Constant cameras.  cam_constant: n_cams bytes; a camera with a non-zero byte has no tangent column at all -- no pose columns and, in
 * intrinsics_mode 1, no intrinsics columns: its observations are residuals of their landmarks alone, its pose6 / intr6 come back
 * unchanged bit for bit, its focal lengths are neither projected onto focal_upper_bound nor counted in bound_projections.
 * fix_cam0_pose / fix_cam1_translation keep their meaning for cameras 0 and 1 when those are not constant.  ONE constant camera fixes
 * position and orientation but leaves the scale free (rcn_ba_options' default holds camera 1's translation for that); two or more fix
 * the gauge.  cam_constant == NULL or all zeros: rcn_ba_solve_robust, bit for bit.  RCN_ERR_ARG with a message when no parameter of
 * the reduced system is left free (every camera constant). */
int rcn_ba_solve_constant(rcn_ctx *ctx, const rcn_ba_problem *problem, const rcn_ba_options *options, const rcn_ba_loss *loss,
                          const uint8_t *cam_constant, rcn_ba_summary *summary, rcn_ba_loss_report *report, double *weights_host);

/* Shared intrinsics: cameras tied in groups.  cam_group: n_cams int32; -1 = the camera's own intrinsics; equal values >= 0 = one
 * physical camera, whose fx, fy, k1, k2 are ONE set of four unknowns in intrinsics_mode 1 (cx, cy stay constant, as for every camera).
 * What is solved is the problem with one parameter block per group: the reduced system of the per-camera problem, S delta = b, is
 * folded to S' = P' S P, b' = P' b (P: one 1 per row, the members' columns onto their group's), factorised, and the step expanded
 * again, delta = P delta'.
 *   No groups.  cam_group == NULL, all -1, intrinsics_mode 0, or nothing but groups of one camera: rcn_ba_solve_constant, bit for bit,
 *     with the same kernels and launches (a group of one camera is its own camera).
 *   Members must agree on entry: the members of a group enter with bit-identical intr6, all six numbers; otherwise RCN_ERR_ARG, the
 *     message names the first offending camera.  They leave bit-identical.
 *   Constant members.  A group with a constant member (cam_constant) has its intrinsics held for every member: its free members keep
 *     their pose columns and have no intrinsics columns (a free camera then has 6, 3 or 0 columns in mode 1).
 *   Column order of the tied system: cameras in index order, each with its pose columns and, when it is in no group, its own four
 *     intrinsics columns; then the groups in ascending order of their smallest member, four columns each (fx, fy, k1, k2).
 *   rcn_ba_summary::reduced_dim is the tied system's size.  The focal bound, and the projection onto it at entry, apply to a tied
 *     column once: bound_projections counts a tied focal length once, not once per member.
 *   Jacobi scale of a tied column: 1 / (1 + sqrt(sum over the members of the raw diagonal)).  LM diagonal: clamp(scale^2 * that sum,
 *     min_lm_diagonal, max_lm_diagonal) / radius -- the clamp of the sum.  The step norm, |x|, gradient . step and the gradient's
 *     max-norm (the members' gradients summed) count a tied parameter once.  No float atomics: a tied solve is bit-reproducible.
 * RCN_ERR_ARG with a message (nothing written): a group id below -1, members that disagree. */
int rcn_ba_solve_tied(rcn_ctx *ctx, const rcn_ba_problem *problem, const rcn_ba_options *options, const rcn_ba_loss *loss,
                      const uint8_t *cam_constant, const int32_t *cam_group, rcn_ba_summary *summary, rcn_ba_loss_report *report,
                      double *weights_host);

/* Introspection, pure host code (no device, no ctx): the SCHEDULE of the dense factorisation inside rcn_ba_solve for a reduced system of
 * n_blocks 128-row blocks (csrc/chol_plan.h) -- the list of tile operations in an order that is a correct sequential algorithm, each
 * with its stream and the device counters it waits for, and the tile maps of the pipelined launches.  tests/test_chol_plan.py executes
 * it in numpy (list order; random orders that respect only the waits) and checks that the waits order every pair of operations that
 * touch a common tile.  params: {panels per super-step, min rows for a super-step, pairs (0/1), min rows for a pair, min tiles for the
 * pipelined panel kernels, own stream for the two-level panel product (0/1), that product as the tail of the previous bulk launch (0/1), the head rows'
 * product and the next super-diagonal block's update through the latency kernel (0/1), rows below which a super-block's small operations
 * run on the chain's own stream, 2 g-row window of the chain's latency kernels (0/1), the diagonal
 * blocks in one resident workgroup (0/1), bulk updates of the right-looking regime behind the next diagonal block (0/1), rows from which on the chain's next tiles are
 * carved out of the right-looking regime's updates (0: never)},
 * NULL = what the library uses.  An operation is
 * RCN_PLAN_OP_WORDS int32: kind, stream, ticket, kb, first, m, dj, nst, map_off, map_n, g, pos, n_waits, 6 x (counter, value), timeline
 * slot, awaited, index of the bulk update whose launch carries this operation's tiles as its tail (-1: none), 1 = latency-kernel form.  Counters 0 .. 4 are the streams' progress counters (4: the resident workgroup that factors the diagonal blocks), 5 and 6 count the two
 * classes of leading tiles of the bulk updates.  Returns RCN_ERR_ARG when a buffer is too
 * small (the needed sizes are still written). */
#define RCN_PLAN_OP_WORDS 29
int rcn_ba_factor_plan(int32_t n_blocks, const int32_t *params, int32_t *ops, int64_t ops_cap, uint32_t *maps, int64_t maps_cap,
                       int64_t *n_ops, int64_t *n_maps);

/* ---- device-resident bundle adjustment across the incremental loop ----------------------------
 * SequentialReconstructor::reconstruct (SequentialReconstructor.cpp:1040-1094) runs, after every registered view,
 * checkLandmarkValidity -> BundleAdjuster().adjust(all views so far) -> checkLandmarkValidity -> removeOutlierLandmarks:
 * N - 2 global solves on a problem that grows by one camera, its new landmarks and their observations each time.
 * A session keeps that problem in HBM between the solves -- landmark coordinates, landmark-major observation arrays,
 * the observation-pair lists of the Schur build, the solver workspace -- with the graph (tracks in
 * triangulatedFeatures order; additions append like push_back) and the 12 numbers per camera mirrored on the host.
 * A session solve is rcn_ba_solve's arithmetic on the same problem: identical results, bit for bit.
 *   cameras       index = position in imgIdxOrder; pose6 / intr6 as rcn_ba_problem
 *   observations  (landmark, camera, integer pixel x, y), appended to the END of the landmark's track            */
typedef struct rcn_ba_session rcn_ba_session;
int  rcn_ba_session_create(rcn_ctx *ctx, rcn_ba_session **out);
void rcn_ba_session_destroy(rcn_ba_session *s);
int  rcn_ba_session_add_camera(rcn_ba_session *s, const double *pose6, const double *intr6, int32_t *index_out);
/* read (…_out) and / or overwrite (…_in) every camera's pose6 / intr6; any pointer may be NULL.  Adapters that keep
 * the reference's 4x4 pose matrices between solves (unpack :157-185, re-pack :46-59) round-trip the poses here. */
int  rcn_ba_session_cameras(rcn_ba_session *s, double *poses_out, double *intr_out, const double *poses_in, const double *intr_in);
int  rcn_ba_session_add_points(rcn_ba_session *s, int32_t n, const double *xyz_host, int32_t *first_index_out);
int  rcn_ba_session_add_observations(rcn_ba_session *s, int32_t n, const int32_t *pt, const int32_t *cam, const int32_t *xy);
int  rcn_ba_session_counts(const rcn_ba_session *s, int32_t *n_cams, int32_t *n_points, int64_t *n_obs);
/* the graph, flattened landmark-major in track order: n_obs entries each (xy_out: 2 per entry); any pointer may be NULL */
int  rcn_ba_session_graph(rcn_ba_session *s, int32_t *pt_out, int32_t *cam_out, int32_t *xy_out);
/* options == NULL: rcn_ba_default_options for the current camera count (the reference's choice, BundleAdjuster.cpp:99-142) */
int  rcn_ba_session_solve(rcn_ba_session *s, const rcn_ba_options *options, rcn_ba_summary *summary);
/* Local adjustment (COLMAP's AdjustLocalBundle): the cameras free_cams move, together with every landmark that has an observation in
 * one of them; every other camera that sees such a landmark takes part as a constant (rcn_ba_solve_constant); every other landmark
 * has no residual in the sub-problem and stays where it is, bit for bit, and so does every camera that is not free.  The sub-problem
 * is cut out of the resident arrays on the device (landmarks in session order, observations in track order, cameras in ascending
 * session index), solved under the session's loss, and scattered back; the graph and its version do not change.
 * free_cams: n_free distinct session camera indices, any order.  options == NULL: rcn_ba_default_options(n_free)
 * (a local bundle of < 10 views keeps all intrinsics constant, like the reference's small problems); fix_cam0_pose /
 * fix_cam1_translation apply to the sub-problem's cameras 0 and 1 when those are free.
 * info_out (may be NULL): local cameras, of them constant, landmarks, observations of the sub-problem.
 * RCN_ERR_ARG with a message: a null or empty free_cams, an index out of range, a duplicate, free cameras without any observation
 * (no free parameter); the session is unchanged and usable. */
int  rcn_ba_session_solve_local(rcn_ba_session *s, const int32_t *free_cams, int32_t n_free,
                                const rcn_ba_options *options, rcn_ba_summary *summary, int32_t info_out[4]);
/* Landmarks shared with camera `cam`, per session camera (counts_out[n_cams], counts_out[cam] = its own landmark
 * count), and the k cameras other than `cam` that share the most, count descending, ties to the lower index;
 * fewer than k when fewer share any.  A landmark that sees a camera twice counts once for it.  Integer counts on the device; the
 * selection among n_cams numbers on the host.  counts_out may be NULL; cams_out / n_out may be NULL when k == 0.
 * RCN_ERR_ARG with a message: cam out of range, k < 0. */
int  rcn_ba_session_covisible(rcn_ba_session *s, int32_t cam, int32_t k, int32_t *cams_out, int32_t *n_out, int32_t *counts_out);
/* Host-clock seconds of the last rcn_ba_session_solve_local, each part ending synchronised: the extraction, the solve (structure pass
 * and workspace included; rcn_ba_summary::solve_seconds is the LM loop inside it), the scatter.  For tools/ba_local_timing.py. */
int  rcn_ba_session_local_seconds(const rcn_ba_session *s, double seconds_out[3]);
/* The loss of every later rcn_ba_session_solve (kept across solves; NULL or RCN_BA_LOSS_TRIVIAL: none): rcn_ba_solve_robust's
 * arithmetic on the same problem, bit for bit.  Argument errors as there. */
int  rcn_ba_session_set_loss(rcn_ba_session *s, const rcn_ba_loss *loss);
/* rcn_ba_solve_robust's report and weights at the session's current state (its cameras, points and graph as they stand), under
 * the session's loss; either pointer may be NULL, weights_host holds n_obs doubles. */
int  rcn_ba_session_loss_report(rcn_ba_session *s, rcn_ba_loss_report *report, double *weights_host);
/* The groups of every later rcn_ba_session_solve (rcn_ba_solve_tied's arithmetic on the same problem, bit for bit) and
 * rcn_ba_session_solve_local (the groups mapped through the window's camera map; a group with a member among the window's constant
 * cameras is held).  Kept across solves; cameras added later are -1 until set again.  n must equal the camera count, an id below -1 is
 * refused (RCN_ERR_ARG with a message, the session's groups unchanged); cam_group == NULL with n == 0 clears them. */
int  rcn_ba_session_set_groups(rcn_ba_session *s, const int32_t *cam_group, int32_t n);
int  rcn_ba_session_read_points(rcn_ba_session *s, double *xyz_host);
const double *rcn_ba_session_points_device(rcn_ba_session *s);      /* n_points x 3 in HBM; valid until the next add / remove */
/* checkLandmarkValidity (SequentialReconstructor.cpp:869-954) on the session's arrays, on the device.  poses34_host:
 * n_cams x 12, rows of [R | t] of imgIdx2camPose as the pipeline holds them.  Observations the sweep erases are erased
 * from the tracks; inlier_out (n_points bytes), n_inliers_out, n_erased_out may be NULL. */
int  rcn_ba_session_validity(rcn_ba_session *s, const double *poses34_host, double max_projection_error, double min_triangulation_angle,
                             uint8_t *inlier_out, int32_t *n_inliers_out, int32_t *n_erased_out);
/* removeOutlierLandmarks (:956-976) for the flags of the last sweep: landmarks compacted on the device.
 * new_index_out (may be NULL): n_points entries before the call, -1 = removed. */
int  rcn_ba_session_remove_outliers(rcn_ba_session *s, int32_t *new_index_out, int32_t *n_removed_out);
/* triangulateMultiView for a batch of tracks (rcn_triangulate below) straight into the session: camera indices are session
 * indices, poses34_host as in rcn_ba_session_validity, intrinsics the session's own.  Accepted tracks are appended as landmarks
 * (track order, like landmarks.push_back) with their observations in track order; their coordinates go from the kernel into
 * the session's point array without leaving HBM -- only the n_tracks status bytes come back.  The same as rcn_triangulate +
 * rcn_ba_session_add_points + rcn_ba_session_add_observations on the same input, bit for bit.  status_out (n_tracks bytes),
 * first_index_out (index of the first appended landmark), n_added_out may be NULL. */
int  rcn_ba_session_triangulate(rcn_ba_session *s, const double *poses34_host, int32_t n_tracks, const int32_t *trk_off,
                                const int32_t *obs_cam, const int32_t *obs_xy, double max_projection_error, double min_triangulation_angle,
                                uint8_t *status_out, int32_t *first_index_out, int32_t *n_added_out);

/* Step 1 of triangulateMatchedLandmarks against the session's landmarks (rcn_landmark_attach's rules; camera `cam` of the
 * session, poses34_host as in rcn_ba_session_validity, its intrinsics the session's own).  The points stay in HBM; only
 * the status bytes come back (status_out, n_added_out may be NULL).  Attached entries are appended to their landmarks'
 * tracks in list order: bit for bit rcn_landmark_attach + rcn_ba_session_add_observations of the attached entries. */
int  rcn_ba_session_attach(rcn_ba_session *s, const double *poses34_host, int32_t cam, int32_t n, const int32_t *landmark,
                           const int32_t *feat, const int32_t *xy, double max_projection_error, uint8_t *status_out,
                           int32_t *n_added_out);

/* ---- landmark validity sweep -------------------------------------------------------------
 * SequentialReconstructor::checkLandmarkValidity (SequentialReconstructor.cpp:869-954), the check
 * the reference runs on the observation graph before and after every bundle adjustment:
 *   - walk each landmark's triangulatedFeatures in order; an observation whose L1 reprojection
 *     error |u - x| + |v - y| (calcProjectionError :852-867, PinholeCamera::project Camera.h:59-76)
 *     exceeds max_projection_error, or whose camera-frame depth is negative, is erased -- with the
 *     reference's loop, which skips the element that slides into the erased slot (:877-898);
 *     fewer than two observations left after an erase marks the landmark an outlier;
 *   - a landmark none of whose surviving observation pairs subtends more than
 *     min_triangulation_angle "degrees" (calcTriangulationAngle :815-836, pi = 3.1415) is an outlier.
 * Defaults of the reference: 4.0 px and 1.0 (SequentialReconstructor.h:256-257).
 *   poses34    n_cams x 12   rows of [R | t] of imgIdx2camPose (world -> camera)
 *   intrinsics n_cams x 6    fx fy cx cy k1 k2
 *   points     n_points x 3
 *   pt_off     n_points + 1  CSR over the tracks, observations in triangulatedFeatures order
 *   obs_cam    n_obs ; obs_xy n_obs x 2 integer pixel coordinates (Feature<int>::featCoord)
 * out_inlier[n_points]: 1 = keep the landmark (the vector<bool> the reference returns);
 * out_keep[n_obs]: 1 = the observation is still in its track afterwards (the reference erases in
 * place); out_n_inliers may be NULL. */
typedef struct {
    int32_t        n_cams, n_points, n_obs, reserved;
    const double  *poses34;
    const double  *intrinsics;
    const double  *points;
    const int32_t *pt_off;
    const int32_t *obs_cam;
    const int32_t *obs_xy;
} rcn_landmark_problem;
int rcn_landmark_validity(rcn_ctx *ctx, const rcn_landmark_problem *problem, double max_projection_error,
                          double min_triangulation_angle, uint8_t *out_inlier, uint8_t *out_keep,
                          int32_t *out_n_inliers);
/* Same with every pointer (inputs and outputs, out_n_inliers_dev required) in DEVICE memory, e.g.
 * the arrays a bundle adjustment just left in HBM; asynchronous on the ctx stream, no graph check. */
int rcn_landmark_validity_device(rcn_ctx *ctx, const rcn_landmark_problem *problem_dev, double max_projection_error,
                                 double min_triangulation_angle, uint8_t *out_inlier_dev, uint8_t *out_keep_dev,
                                 int32_t *out_n_inliers_dev);

/* ---- multi-view triangulation ----------------------------------------------------------------
 * SequentialReconstructor::triangulateMultiView (SequentialReconstructor.cpp:396-489) for a batch of tracks, one launch:
 *   - unproject every observation (Camera.h:79-93: x = (u - cX) / fX, y = (v - cY) / fY, both minus k1 r + k2 r^2);
 *   - A (2n x 4): rows x P.row(2) - P.row(0), y P.row(2) - P.row(1) with P = [R | t] (no K); X = the right singular vector
 *     of A's smallest singular value, hnormalized (fp64: Givens QR of A streamed row by row, one-sided Jacobi on R);
 *   - status 0 accepted; 1 that singular value is 0 or the WORLD z of X is not > 0 (the reference's test, :425);
 *     2 an observation's L1 reprojection error exceeds max_projection_error (:447-451, no depth test);
 *     3 SOME pair of rays subtends less than min_triangulation_angle "degrees" (pi = 3.1415, :458-478).
 * Defaults of the reference: 4.0 px and 1.0 (SequentialReconstructor.h:256-257).  Layout as rcn_landmark_problem:
 *   poses34 n_cams x 12, intrinsics n_cams x 6, trk_off n_tracks + 1 (CSR over the tracks, observations in the order of
 *   the reference's matchedImgIdFeatId), obs_cam n_obs, obs_xy n_obs x 2 integer pixel coordinates.
 * rcn_triangulate: host arrays; every track needs >= 2 observations (the reference reads singularValues()(3)), trk_off
 * non-decreasing inside n_obs, cameras in range, else RCN_ERR_ARG; n_tracks == 0 is fine.  out_xyz (n_tracks x 3) holds
 * every track's X, accepted or not; out_status n_tracks bytes; out_n_accepted may be NULL. */
typedef struct {
    int32_t        n_cams, n_tracks, n_obs, reserved;
    const double  *poses34;
    const double  *intrinsics;
    const int32_t *trk_off;
    const int32_t *obs_cam;
    const int32_t *obs_xy;
} rcn_triangulation_problem;
int rcn_triangulate(rcn_ctx *ctx, const rcn_triangulation_problem *problem, double max_projection_error,
                    double min_triangulation_angle, double *out_xyz, uint8_t *out_status, int32_t *out_n_accepted);
/* Same with every pointer in DEVICE memory; asynchronous on the ctx stream, no graph check (a track of fewer than 2
 * observations gets status 1).  out_n_accepted_dev (required) receives the count of accepted tracks; out_compact_dev (may be
 * NULL) receives the X of the accepted tracks in track order at rows compact_first, compact_first + 1, ... (room for
 * compact_first + n_tracks rows): a caller can append to an array of landmarks without a host round trip. */
int rcn_triangulate_device(rcn_ctx *ctx, const rcn_triangulation_problem *problem_dev, double max_projection_error,
                           double min_triangulation_angle, double *out_xyz_dev, uint8_t *out_status_dev,
                           double *out_compact_dev, int32_t compact_first, int32_t *out_n_accepted_dev);

/* ---- next view: 2D-3D correspondences, density score, attach ------------------------------------
 * The deterministic part of SequentialReconstructor::addNextView (SequentialReconstructor.cpp:761-813).
 *
 * rcn_match_lists_upload: the directed lists featureMatches[(a, b)] (each injective), once, resident in the ctx until
 * the next upload or rcn_match_lists_clear.  Layout of rcn_match_compact_begin: pairs n_pairs x (a, b) image ids,
 * offsets n_pairs + 1 (int64, offsets[0] = 0), qt offsets[n_pairs] x (feature of a, feature of b) in any order within a
 * pair.  mirror != 0: a directed pair that was not uploaded but whose reverse was is that reverse's inverse (the
 * canonical i < j lists stand for featureMatches[(j, i)]); a pair given in both directions is read as given; a pair given
 * in neither has no matches.  RCN_ERR_ARG: a repeated directed pair, a pair (a, a), a list that is not injective, a
 * feature < 0 or >= K, an image without coordinates (rcn_coords_upload: the cells need them).
 *
 * rcn_corr_2d3d: calc2d3dMatches (:643-695) for every candidate, plus rankNextImages' density score (:714-744).
 *   graph       n_points landmarks as CSR: pt_off (n_points + 1, pt_off[0] = 0), obs_img / obs_feat per observation in
 *               triangulatedFeatures order
 *   candidates  n_cand distinct image ids (the reference's std::set: ascending), cand_shape n_cand x (rows, cols)
 *               (imgIdx2imgShape)
 *   out         entries of candidate k at cand_off[k] .. cand_off[k + 1] (n_cand + 1 int64) in the reference's order:
 *               landmark by landmark, each track in order; an observation (i, f) gives (landmark, g) when
 *               featureMatches[(i, c)] maps f -> g (the same landmark or g may repeat; observations of c itself give
 *               nothing); out_landmark / out_feat hold `capacity` entries (RCN_ERR_ARG with *total_out set when too small);
 *               out_cells[k] = distinct cells (int)(32 x / cols), (int)(32 y / rows) inside 0 .. 31 (the MatchDensity
 *               score); out_outside[k] (may be NULL) = entries whose cell falls outside (they stay in the lists).
 * RCN_ERR_ARG: no lists, an (image, feature) observed twice in the graph (the reference's flow never does that: a
 * feature gets one landmarkId), a feature outside its image's coordinates, a repeated candidate, a shape <= 0, a graph
 * image or candidate without coordinates.  The reference's features[c][g]->landmarkId == -1 test is not modelled (it
 * always holds for an unregistered image); the C++ adapter checks it.  Work and memory are bounded by the workspace
 * budget (rcn_corr_set_workspace_bytes, default 1 GiB of hit rows: 4 bytes per observation per candidate of a batch);
 * results do not depend on it. */
int rcn_match_lists_upload(rcn_ctx *ctx, int32_t n_pairs, const int32_t *pairs, const int64_t *offsets, const int32_t *qt, int32_t mirror);
int rcn_match_lists_clear(rcn_ctx *ctx);
int rcn_corr_set_workspace_bytes(rcn_ctx *ctx, int64_t bytes);
int rcn_corr_2d3d(rcn_ctx *ctx, int32_t n_points, const int32_t *pt_off, const int32_t *obs_img, const int32_t *obs_feat,
                  int32_t n_cand, const int32_t *cand, const int32_t *cand_shape, int64_t *cand_off,
                  int32_t *out_landmark, int32_t *out_feat, int64_t capacity, int64_t *total_out,
                  int32_t *out_cells, int32_t *out_outside);
/* Same with every pointer in DEVICE memory (n_obs = pt_off[n_points] given by the caller); asynchronous on the ctx stream
 * after one small host-to-device copy (the coordinates' slot table); no graph check.  Malformed input cannot make the
 * kernels read or write out of bounds: images without lists, features outside the coordinates and offsets outside
 * 0 .. n_obs are ignored, entries past `capacity` are dropped (*total_dev still counts them).  An (image, feature)
 * observed twice: only its first observation matches. */
int rcn_corr_2d3d_device(rcn_ctx *ctx, int32_t n_points, int32_t n_obs, const int32_t *pt_off_dev, const int32_t *obs_img_dev,
                         const int32_t *obs_feat_dev, int32_t n_cand, const int32_t *cand_dev, const int32_t *cand_shape_dev,
                         int64_t *cand_off_dev, int32_t *out_landmark_dev, int32_t *out_feat_dev, int64_t capacity,
                         int64_t *total_dev, int32_t *out_cells_dev, int32_t *out_outside_dev);
/* Step 1 of triangulateMatchedLandmarks (:497-512) for the new view: entries (landmark, feature, integer pixel xy) in list
 * order (the PnP inliers), the view's pose34 (12) and intrinsics (6), the landmarks' points (n_points x 3).  Entry e is
 * attached iff its camera-frame depth > 0, its L1 reprojection error < max_projection_error (strict; NaN rejected) and no
 * EARLIER ATTACHED entry has the same feature (a rejected entry blocks nothing).  status_out: 0 attached, 1 depth,
 * 2 reprojection, 3 feature already taken -- the first failing rule.  fp64, the validity sweep's projection bit for bit.
 * RCN_ERR_ARG: a landmark index outside 0 .. n_points - 1 or a negative feature.  n_attached_out may be NULL. */
int rcn_landmark_attach(rcn_ctx *ctx, const double *pose34, const double *intr6, int32_t n_points, const double *points, int32_t n,
                        const int32_t *landmark, const int32_t *feat, const int32_t *xy, double max_projection_error,
                        uint8_t *status_out, int32_t *n_attached_out);

/* ---- next view: the candidates of step 3 of triangulateMatchedLandmarks ---------------------------
 * SequentialReconstructor.cpp:514-553, on the resident match lists and coordinates.
 *
 * The landmark-id table is the device copy of features[*][*]->landmarkId: one int32 per keypoint of every image with
 * resident coordinates, -1 = not a landmark (the only thing the reference ever tests).
 *   rcn_landmark_ids_reset  sizes the table from the resident coordinates, every entry -1.  RCN_ERR_ARG: no lists, no
 *                           coordinates.  A later rcn_match_lists_upload / _clear or any change of the coordinates
 *                           (rcn_coords_upload, _batch, _clear) invalidates the table: every call below then fails with
 *                           RCN_ERR_ARG and a message until the next reset; nothing stale is read.
 *   rcn_landmark_ids_set    n host entries (image, feature, id), id -1 frees the entry; a repeated (image, feature) must
 *                           carry one id.  RCN_ERR_NOT_FOUND: an image without a row; RCN_ERR_ARG: a feature outside the
 *                           image's keypoints, an id < -1.  Waits for the scatter (the host arrays are borrowed).
 *   rcn_landmark_ids_read   the K ids of one image (K must be the image's keypoint count).
 *
 * rcn_new_view_tracks_device: the tracks the reference's loop would hand to triangulateMultiView for the new image v.
 *   reg_img_host   the n_reg registered images the caller would visit, in ITS registeredImages iteration order (never
 *                  sorted here), already filtered to status == true and membership in imgMatches[v]; distinct, without v
 *   cam_v, reg_cam_host   the camera rows of v and of every registered image in the caller's pose array
 * For f = 0 .. K_v - 1 with id[v][f] == -1: the smallest k such that featureMatches[(v, reg[k])] maps f -> g and
 * id[reg[k]][g] == -1 gives the track [(reg[k], g), (v, f)] (the registered observation first); a taken partner does not
 * end the search.  featureMatches[(v, r)] is the resident list (v, r), under mirror (r, v) read backwards, as in
 * rcn_corr_2d3d.  Outputs, all in DEVICE memory, in ascending f, rcn_triangulation_problem's layout:
 *   n_tracks_dev   the number of tracks, also when it exceeds `capacity` (tracks past it are dropped, nothing is written
 *                  out of bounds)
 *   trk_off_dev    capacity + 1: trk_off[j] = 2 min(j, n_tracks) -- rows past the count are empty tracks (status 1 of
 *                  rcn_triangulate_device)
 *   obs_cam_dev    2 capacity; obs_xy_dev 2 capacity x 2 from the resident coordinates; trk_src_dev capacity x 3 =
 *                  (reg image id, g, f).  Rows past the count are left as they were.
 * Asynchronous on the ctx stream after one small staged host-to-device copy (the registered images' table).
 * RCN_ERR_ARG: no lists, no (or an invalidated) table, a repeated registered image, v among them, capacity > 2^30;
 * RCN_ERR_NOT_FOUND: an image that is not among the resident lists' images.  A list entry outside its images' keypoints is
 * ignored on the device. */
int rcn_landmark_ids_reset(rcn_ctx *ctx);
int rcn_landmark_ids_set(rcn_ctx *ctx, int32_t n, const int32_t *img, const int32_t *feat, const int32_t *id);
int rcn_landmark_ids_read(rcn_ctx *ctx, int32_t img, int32_t *out, int32_t K);
int rcn_new_view_tracks_device(rcn_ctx *ctx, int32_t v, int32_t n_reg, const int32_t *reg_img_host, int32_t cam_v,
                               const int32_t *reg_cam_host, int32_t capacity, int32_t *n_tracks_dev, int32_t *trk_off_dev,
                               int32_t *obs_cam_dev, int32_t *obs_xy_dev, int32_t *trk_src_dev);
/* rcn_new_view_tracks_device, then rcn_triangulate_device over the `capacity` rows with the caller's poses34_dev /
 * intrinsics_dev (n_cams rows, DEVICE memory; out_xyz_dev capacity x 3, out_status_dev capacity bytes, out_compact_dev /
 * compact_first / out_n_accepted_dev as there), then the commit: accepted track j gets landmark id first_landmark + (the
 * number of accepted tracks before j), written into the table for both of its features.  No host synchronisation between
 * the stages.  RCN_ERR_ARG also for a camera row outside 0 .. n_cams - 1. */
int rcn_new_view_triangulate_device(rcn_ctx *ctx, int32_t v, int32_t n_reg, const int32_t *reg_img_host, int32_t cam_v,
                                    const int32_t *reg_cam_host, int32_t n_cams, const double *poses34_dev, const double *intrinsics_dev,
                                    double max_projection_error, double min_triangulation_angle, int32_t first_landmark, int32_t capacity,
                                    int32_t *n_tracks_dev, int32_t *trk_off_dev, int32_t *obs_cam_dev, int32_t *obs_xy_dev,
                                    int32_t *trk_src_dev, double *out_xyz_dev, uint8_t *out_status_dev, double *out_compact_dev,
                                    int32_t compact_first, int32_t *out_n_accepted_dev);
/* Step 3 for the new view v straight into the session: rcn_new_view_triangulate_device with one row per keypoint of v,
 * camera rows = session indices, poses34_host as in rcn_ba_session_validity, the intrinsics the session's own.  Bit for bit
 * the candidates of the host walk flattened and handed to rcn_ba_session_triangulate: the same points, the same graph in
 * the same order, the same statuses.  The table is committed with the session's landmark indices.  One copy comes back:
 * per candidate (reg image, g, f), both pixels (the host mirror of the graph stores them) and the status byte.
 * n_tracks_out, trk_src_out (room for K_v x 3), status_out (room for K_v bytes), first_index_out, n_added_out may be NULL.
 * rcn_ba_session_attach and rcn_ba_session_remove_outliers do not touch the table: keep it current with
 * rcn_landmark_ids_set. */
int rcn_ba_session_grow_view(rcn_ba_session *s, const double *poses34_host, int32_t v, int32_t cam_v, int32_t n_reg,
                             const int32_t *reg_img, const int32_t *reg_cam, double max_projection_error,
                             double min_triangulation_angle, int32_t *n_tracks_out, int32_t *trk_src_out, uint8_t *status_out,
                             int32_t *first_index_out, int32_t *n_added_out);

/* ---- view registration: P3P-RANSAC + refit ----------------------------------------------------
 * SequentialReconstructor::registerImagePnP (SequentialReconstructor.cpp:559-638) for a batch of views: cv::solvePnPRansac
 * in its P3P mode (4-entry samples from cv::RNG, closed-form 3-point solver, the fourth entry picks the solution; squared
 * reprojection error against max_projection_error^2 in float; OpenCV's update of the iteration count) and a damped
 * Gauss-Newton refit of the best model on its inliers.  The reference passes the default flag (EPnP on 5-entry samples):
 * that one flag is the deliberate difference (where the whole algorithm is written down).
 *   view v      entries off[v] .. off[v + 1] (int64, off[0] = 0): landmark index into points (n_points x 3) and integer pixel;
 *               intr6 = fx fy cx cy k1 k2 per view
 *   count_out   inliers of the best model; -1: no model was accepted; -2: fewer than 4 entries (or, device entry, a view
 *               image without coordinates).  Negative: mask and poses all 0.
 *   mask_out    1 = inlier of the best model (not recomputed after the refit)
 *   pose34_out  rows of [R | t], the refit; ransac_pose34_out (may be NULL) the best model itself
 *   iterations_out (may be NULL) sampling iterations executed
 * RCN_ERR_ARG: a null pointer, decreasing offsets, a landmark outside 0 .. n_points - 1, confidence outside (0, 1), a
 * non-positive threshold or iteration cap.  opt == NULL: the defaults. */
typedef struct { double max_projection_error, confidence; int32_t max_iterations, refine_iterations; } rcn_pnp_options;
void rcn_pnp_default_options(rcn_pnp_options *o);      /* 4.0, 0.99, 10000 (:596), 20 */
int rcn_pnp_ransac(rcn_ctx *ctx, int32_t n_views, const int64_t *off, const int32_t *landmark, const int32_t *xy,
                   int32_t n_points, const double *points, const double *intr6 /* n_views x 6 */, const rcn_pnp_options *opt,
                   double *pose34_out /* n_views x 12 */, double *ransac_pose34_out /* may be NULL */,
                   uint8_t *mask_out, int32_t *count_out, int32_t *iterations_out /* may be NULL */);
/* Every pointer in DEVICE memory, asynchronous on the ctx stream after at most one small host-to-device copy (the table of
 * resident coordinates), no host synchronisation: takes what rcn_corr_2d3d_device left (cand_off_dev, out_landmark_dev,
 * out_feat_dev, cand_dev as view_img_dev) and reads each entry's pixel from the view image's resident coordinates
 * (rcn_coords_upload*).  The data cannot be checked: a landmark or feature outside its array makes the entry a non-inlier
 * that no model is built from, an image without coordinates gives count -2; nothing is read or written out of bounds.
 * ransac_pose34_dev and iterations_dev may be NULL. */
int rcn_pnp_ransac_device(rcn_ctx *ctx, int32_t n_views, const int64_t *off_dev, const int32_t *landmark_dev,
                          const int32_t *feat_dev, const int32_t *view_img_dev, int32_t n_points, const double *points_dev,
                          const double *intr6_dev, const rcn_pnp_options *opt, double *pose34_dev, double *ransac_pose34_dev,
                          uint8_t *mask_dev, int32_t *count_dev, int32_t *iterations_dev);
/* One view against the session's points in HBM (they are not copied): rcn_pnp_ransac on rcn_ba_session_points_device, bit
 * for bit.  The caller then adds the camera (rcn_ba_session_add_camera). */
int rcn_ba_session_pnp(rcn_ba_session *s, int32_t n, const int32_t *landmark, const int32_t *xy, const double *intr6,
                       const rcn_pnp_options *opt, double *pose34_out, uint8_t *mask_out, int32_t *count_out);

/* ---- two-view initialisation: 5-point RANSAC + pose recovery -------------------------------------
 * SequentialReconstructor::chooseInitialPair (SequentialReconstructor.cpp:325-375) behind its choice of the pair, for a batch
 * of pairs: cv::findEssentialMat in its two-camera form (pixels unprojected per image, Camera.h:79-93, and renormalised by the
 * mean of the two camera matrices; 5-entry samples from cv::RNG; Nister's five-point solver, up to ten E per sample; Sampson
 * error in float against (threshold / mean focal)^2; OpenCV's update of the iteration count) followed by cv::recoverPose on
 * the search's own mask (four candidates (R1, t) (R2, t) (R1, -t) (R2, -t), an entry good for a candidate iff both of its
 * depths lie in (0, distance_threshold), the >= cascade).  DESIGN.md section 18 writes the whole algorithm down.
 *   pair p      entries off[p] .. off[p + 1] (int64, off[0] = 0) of xy1 / xy2 (integer pixels of the matched features, in
 *               ascending query-feature order); intr6 = fx fy cx cy k1 k2 of the first / second image of every pair
 *   count_out   n_pairs x 2: inliers of the best E (-1: no model was accepted, -2: fewer than 5 entries; device entry: also
 *               a pair without a resident list or without room), and entries of the cheirality mask.  Negative: every
 *               other output 0.
 *   E_out       n_pairs x 9 row-major, unit Frobenius norm, x2' E x1 = 0 in normalised coordinates (may be NULL)
 *   pose34_out  rows of [R | t] of the second camera, |t| = 1; the first camera is the identity
 *   mask_out    1 = inlier of the best E; cheir_mask_out (may be NULL) 1 = inlier in front of both cameras of the winner
 *   iterations_out (may be NULL) sampling iterations executed
 * RCN_ERR_ARG: a null pointer, decreasing offsets, confidence outside (0, 1), a non-positive threshold, distance or
 * iteration cap.  opt == NULL: the defaults. */
typedef struct { double threshold, confidence, distance_threshold; int32_t max_iterations, reserved; } rcn_twoview_options;
void rcn_twoview_default_options(rcn_twoview_options *o);      /* 1.0, 0.999, 50.0, 1000 */
int rcn_twoview_init(rcn_ctx *ctx, int32_t n_pairs, const int64_t *off, const int32_t *xy1, const int32_t *xy2,
                     const double *intr6_1 /* n_pairs x 6 */, const double *intr6_2, const rcn_twoview_options *opt,
                     double *E_out, double *pose34_out /* n_pairs x 12 */, uint8_t *mask_out, uint8_t *cheir_mask_out,
                     int32_t *count_out /* n_pairs x 2 */, int32_t *iterations_out);

/* Pairs given by image ids (host array, n_pairs x (a, b)), their entries taken on the device from the lists
 * rcn_match_lists_upload left resident (the list (a, b), or (b, a) read backwards under mirror) and the coordinates of
 * rcn_coords_upload, in ascending order of a's feature.  Every other pointer is in DEVICE memory.  Asynchronous on the ctx
 * stream after two small host-to-device copies (the coordinates' slot table, the pairs' slots; both staged in the ctx): no
 * host wait, no device-to-host copy and no allocation once the workspace is sized (by `capacity` and the pairs' feature
 * counts).  off_dev (n_pairs + 1) receives the pairs' offsets; mask_dev / cheir_mask_dev / qt_dev ((feature of a, feature of
 * b) per entry) hold `capacity` entries; a pair whose entries would pass `capacity`, or that has no list, gets none and count
 * -2.  qt_dev, E_dev, cheir_mask_dev, iterations_dev may be NULL.  RCN_ERR_ARG: no lists, a pair (a, a), a null pointer, bad
 * options; RCN_ERR_NOT_FOUND: an image id that is not among the lists' images.  Entries of the resident lists whose
 * features lie outside the coordinates are ignored; nothing is read or written out of bounds. */
int rcn_twoview_init_device(rcn_ctx *ctx, int32_t n_pairs, const int32_t *pairs, const double *intr6_1_dev, const double *intr6_2_dev,
                            const rcn_twoview_options *opt, int64_t capacity, int64_t *off_dev, int32_t *qt_dev, double *E_dev,
                            double *pose34_dev, uint8_t *mask_dev, uint8_t *cheir_mask_dev, int32_t *count_dev, int32_t *iterations_dev);
/* The camera block of rcn_ba_problem / rcn_ba_session_add_camera (angle-axis, translation) of rows of [R | t]: what
 * rcn_ba_session_init_pair stores for the recovered pose, so that a caller who adds that camera itself gets the same bits.
 * Pure host code, no ctx.  Domain: rotation angles away from pi (the axis is taken from R - R', divided by 2 sin(angle));
 * below 1e-12 rad the axis is zero. */
int rcn_pose34_to_pose6(const double *pose34, double *pose6_out);
/* chooseInitialPair + triangulateInitialPair (:325-394) into an EMPTY session (RCN_ERR_ARG otherwise): rcn_twoview_init on the
 * one pair, then -- when count_out[0] >= 0 -- camera 0 = the identity with intr6_1, camera 1 = the recovered pose with intr6_2,
 * and EVERY entry of the pair (not the inliers only, as the reference) as a track of two observations through
 * rcn_ba_session_triangulate with these two poses.  The same as rcn_twoview_init + rcn_pose34_to_pose6 +
 * rcn_ba_session_add_camera twice + rcn_ba_session_triangulate on the same input, bit for bit.  count_out (2) is required;
 * status_out (n bytes, the triangulation's), n_added_out and the other outputs may be NULL.  A negative count_out[0] leaves
 * the session empty and returns RCN_OK. */
int rcn_ba_session_init_pair(rcn_ba_session *s, int32_t n, const int32_t *xy1, const int32_t *xy2, const double *intr6_1,
                             const double *intr6_2, const rcn_twoview_options *opt, double max_projection_error,
                             double min_triangulation_angle, double *E_out, double *pose34_out, uint8_t *mask_out,
                             uint8_t *cheir_mask_out, int32_t *count_out /* 2 */, int32_t *iterations_out, uint8_t *status_out,
                             int32_t *n_added_out);

/* ---- homography RANSAC and two-view classification ---------------------------------------------
 * cv::findHomography(src, dst, RANSAC, 3.0, mask, 2000, 0.995) for a batch of pairs, on the integer pixels themselves (no
 * intrinsics): 4-entry samples from cv::RNG with the homography callback's subset check (no three points on a line in either
 * image, equal orientation of the four triples; a rejected subset is redrawn, at most 10000 times), Hartley-normalised DLT on
 * the four points, the forward transfer error |dst - proj(H src)|^2 in float against threshold^2, OpenCV's update of the
 * iteration count, then a refit on the inliers of the best model (least-squares DLT, at most 10 Gauss-Newton steps on the
 * forward transfer error) and the mask of the refitted H.  DESIGN.md section 27 writes the whole algorithm down.
 *   pair p      entries off[p] .. off[p + 1] (int64, off[0] = 0) of xy1 (src) / xy2 (dst), in ascending query-feature order
 *   count_out   n_pairs: inliers of the refitted H (-1: no model was accepted, -2: fewer than 4 entries; device entry: also
 *               a pair without a resident list or without room).  Negative: every other output 0.  Exactly 4 entries: the
 *               exact model with all four as inliers if the subset check passes, -1 otherwise.
 *   H_out       n_pairs x 9 row-major, h33 = 1, dst ~ H src in pixels
 *   mask_out    1 = inlier of H; iterations_out (may be NULL) sampling iterations executed
 * RCN_ERR_ARG: a null pointer, decreasing offsets, confidence outside (0, 1), a non-positive threshold or iteration cap.
 * opt == NULL: the defaults. */
typedef struct { double threshold, confidence; int32_t max_iterations, reserved; } rcn_homography_options;
void rcn_homography_default_options(rcn_homography_options *o);      /* 3.0, 0.995, 2000 */
int rcn_homography_ransac(rcn_ctx *ctx, int32_t n_pairs, const int64_t *off, const int32_t *xy1, const int32_t *xy2,
                          const rcn_homography_options *opt, double *H_out /* n_pairs x 9 */, uint8_t *mask_out,
                          int32_t *count_out /* n_pairs */, int32_t *iterations_out);
/* Pairs given by image ids against the resident lists and coordinates, as rcn_twoview_init_device: the same front end, the
 * same `capacity` rule and error codes, no host wait.  qt_dev and iterations_dev may be NULL. */
int rcn_homography_ransac_device(rcn_ctx *ctx, int32_t n_pairs, const int32_t *pairs, const rcn_homography_options *opt,
                                 int64_t capacity, int64_t *off_dev, int32_t *qt_dev, double *H_dev, uint8_t *mask_dev,
                                 int32_t *count_dev, int32_t *iterations_dev);

/* The degeneracy check of an initial pair: one call gathers the pairs' entries once and runs the E search (rcn_twoview_init,
 * the same bits), the H search (rcn_homography_ransac, the same bits) and the classification on them.
 *   ratio_out         count_H / count_E (0 when count_E <= 0 or count_H < 0)
 *   median_angle_out  lower median (element (m - 1) / 2 of the ascending order) over the m entries of the cheirality mask of the
 *                     angle between R x1 and x2 (x: the unprojected pixel, Camera.h:79-93) in the loop's own unit
 *                     180 acos(.) / 3.1415; 0 when the mask is empty
 *   label_out         tested in this order: RCN_TV_NO_MODEL count_E < min_inliers or m < min_inliers; RCN_TV_PANORAMIC ratio >=
 *                     max_h_ratio and median_angle < min_angle; RCN_TV_PLANAR ratio >= max_h_ratio; RCN_TV_SMALL_BASELINE
 *                     median_angle < min_angle; RCN_TV_GENERAL otherwise
 * top_m is the number of candidates the callers' pair choice looks at (HipNextView.h, twoview.py); the library only checks it.
 * Every E and H output of rcn_twoview_init / rcn_homography_ransac is required here except E_out, cheir_mask_out and the two
 * iteration counts.  RCN_ERR_ARG: as the two searches, and max_h_ratio <= 0, top_m < 1.  NULL options: the defaults. */
enum { RCN_TV_NO_MODEL = 0, RCN_TV_PANORAMIC = 1, RCN_TV_PLANAR = 2, RCN_TV_SMALL_BASELINE = 3, RCN_TV_GENERAL = 4 };
typedef struct { double max_h_ratio, min_angle; int32_t min_inliers, top_m; } rcn_twoview_geometry_options;
void rcn_twoview_geometry_default_options(rcn_twoview_geometry_options *o);      /* 0.8, 1.0, 15, 10 */
int rcn_twoview_geometry(rcn_ctx *ctx, int32_t n_pairs, const int64_t *off, const int32_t *xy1, const int32_t *xy2,
                         const double *intr6_1, const double *intr6_2, const rcn_twoview_options *tv_opt,
                         const rcn_homography_options *h_opt, const rcn_twoview_geometry_options *g_opt, double *E_out,
                         double *pose34_out, uint8_t *mask_out, uint8_t *cheir_mask_out, int32_t *count_out, int32_t *iterations_out,
                         double *H_out, uint8_t *h_mask_out, int32_t *h_count_out, int32_t *h_iterations_out, double *ratio_out,
                         double *median_angle_out, int32_t *label_out);
/* The same behind rcn_twoview_init_device's front end; every output pointer in DEVICE memory and required except qt_dev and
 * the two iteration counts.  Only enqueues. */
int rcn_twoview_geometry_device(rcn_ctx *ctx, int32_t n_pairs, const int32_t *pairs, const double *intr6_1_dev, const double *intr6_2_dev,
                                const rcn_twoview_options *tv_opt, const rcn_homography_options *h_opt,
                                const rcn_twoview_geometry_options *g_opt, int64_t capacity, int64_t *off_dev, int32_t *qt_dev,
                                double *E_dev, double *pose34_dev, uint8_t *mask_dev, uint8_t *cheir_mask_dev, int32_t *count_dev,
                                int32_t *iterations_dev, double *H_dev, uint8_t *h_mask_dev, int32_t *h_count_dev,
                                int32_t *h_iterations_dev, double *ratio_dev, double *median_angle_dev, int32_t *label_dev);

/* ---- epipolar filter of a pair's matches --------------------------------------------------
 * GeometricFilter::estimateFundamental (GeometricFilter.cpp:39-61) as the pair loop uses it
 * (SequentialReconstructor.cpp:237-269): cv::findFundamentalMat(pts1, pts2, mask) with OpenCV's
 * defaults -- RANSAC over 7-point samples for >= 15 points, LMedS for 8..14, threshold 3 px,
 * confidence 0.99, at most 1000 iterations, cv::RNG seeded the same way at every call -- of which
 * the reference keeps only the inlier mask.
 *   xy1, xy2   n x 2 integer pixel coordinates of the matched features (featuresToCvPoints,
 *              utils.cpp:165-177), in ascending query-feature order (the std::map's order)
 *   out_mask   n bytes, 1 = inlier
 *   out_count  inliers; -1: no model was found (the reference then stores no match for the pair,
 *              :252-255; mask all 0); -2: fewer than 7 points, not filtered (mask all 1, :237).
 *   out_F      may be NULL; 9 doubles, row-major: the winning 7-point hypothesis (F(3,3) = 1), zeros
 *              when there is none.  (OpenCV returns a refit on the inliers instead; no caller in the
 *              reference reads the matrix.) */
int rcn_fmat_filter(rcn_ctx *ctx, const int32_t *xy1, const int32_t *xy2, int32_t n, uint8_t *out_mask,
                    int32_t *out_count, double *out_F);
/* All pairs of a grid in one launch: pair p owns points pair_off[p] .. pair_off[p+1] of xy1 / xy2 /
 * out_mask; out_counts[p] as above; out_iterations (may be NULL) = sampling iterations executed;
 * out_F (may be NULL) = 9 doubles per pair. */
int rcn_fmat_filter_grid(rcn_ctx *ctx, int32_t n_pairs, const int32_t *pair_off, const int32_t *xy1,
                         const int32_t *xy2, uint8_t *out_mask, int32_t *out_counts, int32_t *out_iterations,
                         double *out_F);
/* Same with every pointer in DEVICE memory (all required but out_F_dev); asynchronous on the ctx stream. */
int rcn_fmat_filter_grid_device(rcn_ctx *ctx, int32_t n_pairs, const int32_t *pair_off_dev, const int32_t *xy1_dev,
                                const int32_t *xy2_dev, uint8_t *out_mask_dev, int32_t *out_counts_dev,
                                int32_t *out_iterations_dev, double *out_F_dev);

/* Fused form for a match table that is already in HBM (rcn_match_grid_device): lines :237-269 of
 * the pair loop for every pair, no host round trip.  Needs the integer pixel coordinates of the
 * keypoints of every image involved (Feature<int>::featCoord, K x 2), uploaded once per image. */
int rcn_coords_upload(rcn_ctx *ctx, int32_t img_id, const int32_t *xy_host, int32_t K);
/* n images in one call: one asynchronous copy per image, one host synchronisation (the coordinates' rcn_desc_upload_batch) */
int rcn_coords_upload_batch(rcn_ctx *ctx, int32_t first_img_id, int32_t n_images, const int32_t *const *xy_host, const int32_t *K);
int rcn_coords_clear(rcn_ctx *ctx);
/* pairs_host / table_dev / stride / counts_dev exactly as given to and left by rcn_match_grid_device.
 * The table is filtered in place: in a pair with >= 7 matches only the inliers stay (none when no
 * model was found); pairs with fewer are left alone.  counts_dev is updated; out_status_dev (may be
 * NULL) receives rcn_fmat_filter's out_count per pair.  Asynchronous on the ctx stream after one
 * small host-to-device copy. */
int rcn_match_table_filter_device(rcn_ctx *ctx, const int32_t *pairs_host, int32_t n_pairs, int32_t *table_dev,
                                  int64_t stride, int32_t *counts_dev, int32_t *out_status_dev);

/* The same filter, keeping every pair's model: out_F_dev [n_pairs][9] doubles, row-major, the winning 7-point hypothesis as
 * rcn_fmat_filter_grid_device's out_F_dev writes it on the same lists, zeros for a pair without one (fewer than 7 matches, or no model
 * found).  Table, counts and status are those of rcn_match_table_filter_device bit for bit. */
int rcn_match_table_filter_model_device(rcn_ctx *ctx, const int32_t *pairs_host, int32_t n_pairs, int32_t *table_dev,
                                        int64_t stride, int32_t *counts_dev, int32_t *out_status_dev, double *out_F_dev);

/* ---- guided matching: the exact 2-NN inside the epipolar band of each pair ----------------------
 * For pair (i, j) and its model F (9 doubles, row-major, the filter's convention: p1 the query point of image i, p2 the train
 * point of image j, residual p2^T F p1) a train row is a CANDIDATE of a query row when both points lie within max_error_px of the
 * other's epipolar line -- csrc/guided_band.h, division-free fp64 on the resident integer coordinates; a zero, non-finite or
 * degenerate F has no candidates.  Among a row's candidates only, distance and order are the matcher's own (canonical fp64 chain,
 * ascending (d2, train row), dist = sqrtf((float)d2)).  A row is accepted when dist0 < ratio * dist1 in fp32 (dist1 = +inf for a lone
 * candidate) and, with max_distance > 0, dist0 <= max_distance.  cross_check == 0: the lowest query row keeps a contested train row;
 * cross_check != 0: a match must also be the accepted choice of its train row in the reversed pair under F^T (the band is the exact
 * transpose, d2 symmetric in its bits), so no train row appears twice.
 * Needs the fp32 descriptors (rcn_desc_*) and the coordinates (rcn_coords_upload*) of every image named, with equal counts.
 * Errors: NOT_FOUND for an image without either, ARG for unequal counts, a stride below a query image's K, a ratio or max_error_px that
 * is not finite-positive (max_error_px = +inf is allowed: every pair of rows is in the band of a non-degenerate F), null pointers. */
typedef struct { float ratio; float max_error_px; float max_distance; int32_t cross_check; } rcn_guided_options;
int rcn_guided_default_options(rcn_guided_options *o);      /* 0.7f, 3.0f, 0 (off), 0 */
/* out_dev [n_pairs][out_stride]: train row per query row or -1, the tail of each row -1; counts_dev [n_pairs]: entries >= 0;
 * cand_dev (may be NULL) [n_pairs]: in-band (query, train) combinations of the pair.  Pairs run in chunks under
 * rcn_match_set_workspace_rows (4 bytes per train row of a chunk; no K1 x K2 array exists); the result does not depend on the chunking.
 * Asynchronous on the ctx stream after one small host-to-device copy. */
int rcn_match_guided_device(rcn_ctx *ctx, const int32_t *pairs_host, int32_t n_pairs, const double *F_dev, const rcn_guided_options *opt,
                            int32_t *out_dev, int64_t out_stride, int32_t *counts_dev, int64_t *cand_dev);
/* The same with F, out, counts and cand (may be NULL) on the HOST. */
int rcn_match_guided(rcn_ctx *ctx, const int32_t *pairs_host, int32_t n_pairs, const double *F_host, const rcn_guided_options *opt,
                     int32_t *out_host, int64_t out_stride, int32_t *counts_host, int64_t *cand_host);
/* One pair straight from host rows and coordinates (nothing resident is touched). */
int rcn_match_pair_guided(rcn_ctx *ctx, const float *q_host, int32_t K1, const int32_t *xy1_host, const float *t_host, int32_t K2,
                          const int32_t *xy2_host, int32_t D, const double *F, const rcn_guided_options *opt,
                          int32_t *out_train_for_query, int32_t *out_count);
/* The two neighbours themselves: idx_dev [n_pairs][stride][4] = (j0, j1, candidates of the row, 0), -1 where absent; d2_dev
 * [n_pairs][stride][2] = their squared distances, +inf where absent.  Rows past a query image's K: (-1, -1, 0, 0) and +inf. */
int rcn_guided_knn2_device(rcn_ctx *ctx, const int32_t *pairs_host, int32_t n_pairs, const double *F_dev, float max_error_px,
                           int32_t *idx_dev, double *d2_dev, int64_t stride);
/* The body of the pair loop with the guided step, results on the HOST: rcn_match_grid_device, rcn_match_table_filter_model_device, then
 * rcn_match_guided_device (opt; opt->ratio is the guided step's ratio, `ratio` the first match's) on every pair whose verdict is > 0;
 * the other pairs keep the filtered table.  status_host (may be NULL): the filter's verdict per pair. */
int rcn_match_grid_guided(rcn_ctx *ctx, const int32_t *pairs_host, int32_t n_pairs, float ratio, const rcn_guided_options *opt,
                          int32_t *out_host, int64_t out_stride, int32_t *counts_host, int32_t *status_host);

/* The body of the pair loop (:232-275) for a list of pairs over resident images, results on the HOST: match, then --
 * filter != 0 -- the filter above on the table where it lies in HBM, then the dense table (as rcn_match_grid), the
 * counts and (status_host, may be NULL) the filter's verdict per pair (rcn_fmat_filter's out_count; -2 everywhere when
 * filter == 0).  HipPairGridDriver.h uses it for the pairs the loop matches a second time the other way round. */
int rcn_match_grid_filtered(rcn_ctx *ctx, const int32_t *pairs_host, int32_t n_pairs, float ratio, int32_t filter,
                            int32_t *out_host, int64_t out_stride, int32_t *counts_host, int32_t *status_host);
/* The same filter on the tables the last rcn_shard_match(sh, ratio, NULL, 0, NULL) left in the shard's ctx, in place,
 * before rcn_shard_lists.  The coordinates of EVERY image of the grid must have been uploaded to this rank's ctx
 * (rcn_coords_upload: 8 bytes per keypoint, handed round by the host like the image list itself).
 * status_host (may be NULL): verdict per pair of this rank, rcn_shard_pairs order. */
int rcn_shard_filter(rcn_shard *sh, int32_t *status_host);

/* ---- store: features + matches on disk -------------------------------------------------------
 * The cache of features / matches the reference lists as a TODO (README.md:39): one versioned binary
 * file (format in reconstructor_amd/csrc/store.hip; FNV-1a checksum; written to <path>.tmp, then
 * renamed) holding per image the K x D fp32 descriptor rows -- the Feature::featDesc.desc vectors,
 * datatypes.h:48-72 -- and optionally the K x 2 integer keypoint coordinates (Feature<int>::featCoord),
 * and per matched pair the (query feature, train feature) lists of featureMatches in the layout
 * rcn_match_compact_begin produces.  Pure host code; a matching stage can be resumed from the file. */
typedef struct {
    int32_t n_images, D, has_coords, n_pairs;
    const int32_t        *img_ids;    /* n_images */
    const int32_t        *img_K;      /* n_images */
    const float  *const  *desc;       /* n_images pointers to K x D fp32 */
    const int32_t *const *coords;     /* n_images pointers to K x 2 int32, or NULL when !has_coords */
    const int32_t        *pairs;      /* n_pairs x (query image id, train image id) */
    const int64_t        *offsets;    /* n_pairs + 1 */
    const int32_t        *qt;         /* offsets[n_pairs] x (query row, train row) */
} rcn_store_contents;
typedef struct rcn_store rcn_store;
int  rcn_store_save(const char *path, const rcn_store_contents *contents);
int  rcn_store_open(const char *path, rcn_store **out);      /* reads and verifies the whole file */
int  rcn_store_contents_of(const rcn_store *store, rcn_store_contents *out);   /* pointers live until rcn_store_close */
void rcn_store_close(rcn_store *store);
/* descriptors (and coordinates) of every stored image into the ctx: rcn_desc_upload / rcn_coords_upload per image */
int  rcn_store_upload(rcn_ctx *ctx, const rcn_store *store);

/* ---- SIFT: FeatureClassic::detect (FeatureDetector.cpp:13-35 = cv::SIFT::create()->detectAndCompute) --------------
 * Lowe's detector and descriptor with cv::SIFT::create()'s defaults, restated in tests/sift_ref.py (DESIGN section 23;
 * what could not be pinned against OpenCV itself is listed in section 1).  Fixed: first octave -1 (the image is doubled),
 * border 5, at most 5 interpolation steps, 36 orientation bins, descriptor 4 x 4 x 8, integer factor 512.
 *
 * The Gaussian pyramid is fp32 (separable blurs through LDS, weights computed in double on the host and rounded once,
 * reflect-101 border, taps summed in ascending order); everything behind it reads the fp32 pyramid and computes in fp64.
 * An image's result does not depend on the batch, the chunking, the strides or the input type of equal values.
 *
 * Packed pyramid of one image: octave o has S + 3 layers of oct_h[o] x oct_w[o] floats, layer i of octave o starts at
 * element layer_offset[o][i]; floats_per_image in all.  rcn_sift_layout is pure host code (no device needed). */
#define RCN_SIFT_MAX_OCTAVES 16
#define RCN_SIFT_MAX_LAYERS  8           /* S + 3 */
#define RCN_SIFT_MAX_TAPS    96
#define RCN_SIFT_INPUT_F32 0             /* pixels on the 0..255 scale */
#define RCN_SIFT_INPUT_U8  1
typedef struct {
    int32_t n_octave_layers;             /* S: 3, supported 1..5 */
    int32_t reserved;
    double  contrast_threshold;          /* 0.04, >= 0 */
    double  edge_threshold;              /* 10, > 0 */
    double  sigma;                       /* 1.6; > 0 and small enough that no blur needs more than RCN_SIFT_MAX_TAPS taps */
} rcn_sift_options;
typedef struct {
    int32_t n_octaves, n_layers;         /* nOct, S + 3 */
    int32_t base_taps, reserved;
    double  base_sigma;                  /* sqrt(max(sigma^2 - 1, 0.01)): the blur of the doubled image */
    int32_t oct_h[RCN_SIFT_MAX_OCTAVES], oct_w[RCN_SIFT_MAX_OCTAVES];
    double  layer_sigma[RCN_SIFT_MAX_LAYERS];   /* [0] = sigma; [i] the blur that makes layer i from layer i - 1 */
    int32_t layer_taps[RCN_SIFT_MAX_LAYERS];    /* [0] = 0 */
    int64_t layer_offset[RCN_SIFT_MAX_OCTAVES][RCN_SIFT_MAX_LAYERS];
    int64_t floats_per_image;
} rcn_sift_pyramid_layout;
void rcn_sift_default_options(rcn_sift_options *opt);
/* opt == NULL: the defaults.  RCN_ERR_ARG: min(H, W) < 16, 4 H W > 2^31 - 1, an option out of range. */
int  rcn_sift_layout(int32_t H, int32_t W, const rcn_sift_options *opt, rcn_sift_pyramid_layout *out);
/* images per pass over the ctx's workspace (<= 0: as many as fit its default cap of 1 GiB) */
int  rcn_sift_set_chunk_images(rcn_ctx *ctx, int32_t images);
/* images_dev: n grey images [H][W] addressed by ELEMENT strides (image, y, x), as rcn_sp_net_forward_device reads them.
 * pyr_out_dev: [n][floats_per_image].  Asynchronous on the ctx stream. */
int  rcn_sift_pyramid_device(rcn_ctx *ctx, const void *images_dev, int32_t input_dtype, int64_t stride_img, int64_t stride_y,
                             int64_t stride_x, int32_t n, int32_t H, int32_t W, const rcn_sift_options *opt, float *pyr_out_dev);
/* The extrema alone, for inspection: a pixel of DoG layer 1..S, at least 5 from the border, with |v| > floor(0.5 contrast / S * 255) that
 * is >= (v > 0) or <= (v < 0) all 26 neighbours -- fp32 comparisons only, so the set is exact given the pyramid.  A record is
 * (octave << 56) | (layer << 52) | (row << 26) | column, in no particular order; counts[i] is the number found, of which the first
 * `capacity` were stored. */
int  rcn_sift_candidates_device(rcn_ctx *ctx, const float *pyr_dev, int32_t n, int32_t H, int32_t W, const rcn_sift_options *opt,
                                int32_t capacity, uint64_t *cand_out_dev /*[n][capacity]*/, int32_t *counts_dev /*[n]*/);
/* The stages behind the pyramid (extrema, refinement, orientation, duplicates, order, cap) on pyramids the caller has.
 * Keypoints in ascending order of (x, y, size, angle, response, packed octave); counts[i] is the uncapped number -- when it
 * exceeds K the K largest by (response descending, canonical rank ascending) are emitted, still in canonical order.  Rows
 * past min(counts[i], K): xy and xy_int (-1, -1), the other fields 0.  xy_int is xy truncated toward zero (Feature<int>::featCoord).
 * counts[i] = -1 (and no rows): the image had more extrema than the workspace holds (one per 8 pyramid pixels and layer, above the 2 / 27 of uncorrelated noise). */
int  rcn_sift_detect_device(rcn_ctx *ctx, const float *pyr_dev, int32_t n, int32_t H, int32_t W, const rcn_sift_options *opt, int32_t K,
                            float *xy_dev /*[n][K][2]*/, int32_t *xy_int_dev /*[n][K][2]*/, float *size_dev /*[n][K]*/,
                            float *angle_dev /*[n][K]*/, float *response_dev /*[n][K]*/, int32_t *octave_dev /*[n][K]*/,
                            int32_t *counts_dev /*[n]*/);
/* 128 integer-valued floats per keypoint, rows past min(counts[i], K) zero (the local_K contract of rcn_shard_exchange) */
int  rcn_sift_describe_device(rcn_ctx *ctx, const float *pyr_dev, int32_t n, int32_t H, int32_t W, const rcn_sift_options *opt, int32_t K,
                              const float *xy_dev, const float *size_dev, const float *angle_dev, const int32_t *octave_dev,
                              const int32_t *counts_dev, float *rows_out_dev /*[n][K][128]*/);
/* The three in one call, the pyramid in the ctx's workspace: bit for bit the three calls. */
int  rcn_sift_detect_and_compute_device(rcn_ctx *ctx, const void *images_dev, int32_t input_dtype, int64_t stride_img, int64_t stride_y,
                                        int64_t stride_x, int32_t n, int32_t H, int32_t W, const rcn_sift_options *opt, int32_t K,
                                        float *xy_dev, int32_t *xy_int_dev, float *size_dev, float *angle_dev, float *response_dev,
                                        int32_t *octave_dev, int32_t *counts_dev, float *rows_out_dev);

/* ---- retrieval: the ImageMatcher stage (ImageMatcher.h:14-33) by global descriptor ------------------------------------
 * Which image pairs are matched at all.  The reference ships FakeImgMatcher (ImageMatcher.cpp:6-23: every i != j); this is the
 * retrieval its README leaves open, built from the local descriptors alone: Lloyd's k-means on the call's own rows (or a
 * codebook of the caller's), VLAD per image, dense similarities, the top k neighbours per image, and their symmetric pair list
 * in the order rcn_match_grid takes.  No model and no codebook is shipped.  Defined by tests/retr_ref.py:
 * fp64 on the fp32 inputs, products rounded before they are added, sums in ascending order; every stage equals it bit for bit.
 *
 * desc_dev is the matcher's device layout, [n][K][D] fp32 row-major (rcn_desc_upload_batch_device, rcn_shard_reserve, the
 * detectors' output); counts_dev[i] rows of image i are in use (clamped to 0..K; NULL: K each), the rest is never read.
 *
 *   training rows  row r of image i iff r % s == 0 and r < counts[i], in (image, row) order; s = train_row_stride, or when 0
 *                  the smallest s with n ceil(K / s) <= 2^18.  M of them; M < n_centroids is an error.
 *   init           centroid c = training row floor(c M / C)
 *   Lloyd step     nearest centroid by squared distance (ties: the lowest index); centroid = float(sum of its rows / their
 *                  number), the sum per image first and over the images then; an empty cluster keeps its centroid.
 *                  Exactly `iterations` steps.
 *   VLAD           V[c][d] = sum of the image's rows assigned to c - number * centroid; V' = sign(V) sqrt|V|;
 *                  G = float(V' / |V'|), zeros for an image without rows.  L = C D floats per image.
 *   similarity     sim[i][j] = sum over c of (sum over d of G_i[c][d] G_j[c][d]): blocks of D, then the blocks
 *   neighbours     of image i: the j != i by (sim descending, j ascending), the first min(k, n - 1)
 *   pairs          (min(i, j), max(i, j)) for j a neighbour of i, as ids first_img_id + slot, ascending, without duplicates.
 *                  With k >= n - 1 that is the canonical grid (every i < j).
 *
 * An image's G does not depend on the batch it is encoded in, on the padding K, or on n.
 * Limits: 1 <= D <= 256 (RCN_ERR_ARG), C D <= 65536 and n <= 8192 (RCN_ERR_UNSUPPORTED: the similarity matrix is n^2 doubles).
 * RCN_ERR_ARG: a null pointer, a negative size, a codebook of another D or another ctx, top_k / k < 1, n_centroids < 1,
 * iterations < 0, train_row_stride < 0.  n == 0 launches nothing.  Rows must be finite.  Asynchronous on the ctx stream except
 * where noted. */
typedef struct { int32_t n_centroids, iterations, train_row_stride, top_k, reserved[4]; } rcn_retr_options;
void rcn_retr_default_options(rcn_retr_options *o);                       /* 64, 10, 0 (automatic), 20 */
typedef struct rcn_retr_codebook rcn_retr_codebook;
/* opt == NULL: the defaults (top_k is not used here).  Waits once, for M. */
int  rcn_retr_codebook_train_device(rcn_ctx *ctx, const float *desc_dev, const int32_t *counts_dev, int32_t n, int32_t K, int32_t D,
                                    const rcn_retr_options *opt, rcn_retr_codebook **out);
int  rcn_retr_codebook_create(rcn_ctx *ctx, const float *centroids_host /*[C][D]*/, int32_t C, int32_t D, rcn_retr_codebook **out);
/* C and D (either may be NULL), and the centroids unless centroids_host is NULL; waits */
int  rcn_retr_codebook_read(const rcn_retr_codebook *cb, float *centroids_host, int32_t *C, int32_t *D);
void rcn_retr_codebook_destroy(rcn_retr_codebook *cb);                    /* before its ctx */
/* rows_dev: [n_rows][D of the codebook]; assign_dev[r]: the nearest centroid of row r */
int  rcn_retr_assign_device(rcn_ctx *ctx, const rcn_retr_codebook *cb, const float *rows_dev, int64_t n_rows, int32_t *assign_dev);
int  rcn_retr_encode_device(rcn_ctx *ctx, const rcn_retr_codebook *cb, const float *desc_dev, const int32_t *counts_dev, int32_t n, int32_t K,
                            int32_t D, float *global_dev /*[n][C*D]*/);
/* D: the length of a block of the two-level sum (the codebook's D; L a multiple of it) */
int  rcn_retr_similarity_device(rcn_ctx *ctx, const float *global_dev, int32_t n, int32_t L, int32_t D, double *sim_dev /*[n][n]*/);
int  rcn_retr_topk_device(rcn_ctx *ctx, const double *sim_dev, int32_t n, int32_t k, int32_t *nbr_dev /*[n][min(k,n-1)], slots*/);
/* pairs_dev holds `capacity` pairs; *n_pairs_dev receives the length of the list.  Waits for it: RCN_ERR_ARG when the list is
 * longer than capacity (as rcn_match_compact_begin; the first `capacity` pairs are stored).  An entry of nbr_dev outside
 * 0 .. n - 1, or an image's own slot, is ignored. */
int  rcn_retr_pairs_device(rcn_ctx *ctx, const int32_t *nbr_dev, int32_t n, int32_t k, int32_t first_img_id, int32_t *pairs_dev,
                           int64_t capacity, int32_t *n_pairs_dev);
/* All stages behind the codebook, the intermediate results in the ctx's workspace; waits.  pairs_host: the list rcn_match_grid
 * takes, `capacity` pairs; *n_pairs_out its length (RCN_ERR_ARG and nothing copied when capacity is smaller). */
int  rcn_retr_image_pairs(rcn_ctx *ctx, const rcn_retr_codebook *cb, const float *desc_dev, const int32_t *counts_dev, int32_t n, int32_t K,
                          int32_t D, int32_t first_img_id, int32_t top_k, int32_t *pairs_host, int64_t capacity, int32_t *n_pairs_out);

/* ---- image preparation: what detectFeatures does to a photograph before the detector sees it -------------------------
 * Utils::readImg (BGR -> RGB, reshapeImg = cv::resize to at most imgMaxSize on the longer side, the other side cut down to
 * a multiple of 8), cv::cvtColor(RGB2GRAY), the colour under every feature (SequentialReconstructor.cpp:55-110), a
 * landmark's colour (:429-433) and Utils::saveCloud (utils.cpp:205-275, :345-368).  Defined by tests/img_ref.py (DESIGN
 * section 26): cv::resize's default INTER_LINEAR for 8-bit data in its 11-bit fixed point, its 2 x 2 area branch when both
 * axes halve, a copy at equal sizes; every output byte equals the restatement.  JPEG decoding stays with the caller.
 *
 * rcn_img_reshape_size and rcn_img_resize_tables are pure host code (no device needed).  The tables of one axis: for output
 * position d, index_out[d] is the left / upper source pixel -- clamped to 0 .. src - 1 on the horizontal axis, floor(f)
 * itself (-1 .. src - 1) on the vertical one, where it is clipped together with its successor -- and weights_out[d] the two
 * 11-bit weights, which sum to 2048.  *xmax_out (may be NULL): the first d that reads a single pixel at the right border
 * (dst: none, and always on the vertical axis).  They are built in the float / double operations of resize.cpp, in a
 * translation unit compiled without contraction, and uploaded per call; the kernels do integer arithmetic only. */
#define RCN_IMG_RGB 0
#define RCN_IMG_BGR 1
int  rcn_img_reshape_size(int32_t rows, int32_t cols, int32_t max_size, int32_t *rows_out, int32_t *cols_out, double *factor_out);
int  rcn_img_resize_tables(int32_t src, int32_t dst, int32_t horizontal, int32_t *index_out /*[dst]*/, int16_t *weights_out /*[dst][2]*/,
                           int32_t *xmax_out);
typedef struct { int32_t order /*RCN_IMG_RGB | RCN_IMG_BGR*/, gray_bits /*14 | 15*/; } rcn_img_options;
void rcn_img_default_options(rcn_img_options *opt);      /* BGR (what imread delivers), 14 (OpenCV 4.2's table; 15: later releases) */
/* The tile rcn_img_prepare_device works in for this horizontal resize: tile_cols x tile_rows output pixels per workgroup, their
 * source spans staged in lds_bytes of LDS.  tile_rows shrinks as the horizontal scale grows (8, 4, 2, 1); 0: the spans of even
 * one row do not fit, and the one-row tile reads its source pixels from memory directly.  Pure host code. */
int  rcn_img_prepare_plan(int32_t src_cols, int32_t cols, int32_t channels, int32_t *tile_cols, int32_t *tile_rows, int32_t *lds_bytes);
/* n images of one source size, interleaved pixels, rows stride_row_bytes apart (padding allowed, as cv::Mat::step), images
 * stride_img_bytes apart -> rgb_out [n][rows][cols][3] in the order red, green, blue and gray_out [n][rows][cols], either of
 * which may be NULL.  channels == 1: gray_out is the resized plane (readGrayImg + reshapeImg) and rgb_out must be NULL.  One
 * kernel: swap, both resize passes and the grey conversion of the RESIZED colours.  An image's bytes do not depend on n, on
 * the strides, on its position in the batch or on the tile.  opt == NULL: the defaults.
 * RCN_ERR_ARG: a null required pointer, both outputs NULL, channels not 1 or 3, a non-positive size, n < 0, a row stride below
 * src_cols * channels, rows * cols * 3 > 2^31 - 1, an unknown option value, a destination of more than 2^24 - 1 tiles (a launch
 * holds fewer than 2^32 work-items: only a destination a few pixels wide and tens of millions of rows high reaches that; the
 * gathers below refuse n * K, and 2 L + C, beyond 2^32 - 256 for the same reason).  n == 0 launches nothing. */
int  rcn_img_prepare_device(rcn_ctx *ctx, const uint8_t *src_dev, int64_t stride_img_bytes, int64_t stride_row_bytes, int32_t channels /*1 | 3*/,
                            int32_t n, int32_t src_rows, int32_t src_cols, int32_t rows, int32_t cols, const rcn_img_options *opt,
                            uint8_t *rgb_out_dev, uint8_t *gray_out_dev);
/* rgba_out[i][k] = (r, g, b, 0) of rgb[i][y][x] at xy_int[i][k] = (x, y) for k < min(counts[i], K); zero bytes for the other
 * rows and for coordinates outside the image (the reference's unchecked at<> is undefined there). */
int  rcn_feat_colors_device(rcn_ctx *ctx, const uint8_t *rgb_dev /*[n][rows][cols][3]*/, int32_t n, int32_t rows, int32_t cols,
                            const int32_t *xy_int_dev /*[n][K][2]*/, const int32_t *counts_dev /*[n]*/, int32_t K, uint8_t *rgba_out_dev /*[n][K][4]*/);
/* rgba_out[l] = feat_rgba[first_img[l]][first_feat[l]]; zero bytes when either index is out of range */
int  rcn_landmark_colors_device(rcn_ctx *ctx, const uint8_t *feat_rgba_dev /*[n][K][4]*/, int32_t n, int32_t K, int32_t L,
                                const int32_t *first_img_dev, const int32_t *first_feat_dev, uint8_t *rgba_out_dev /*[L][4]*/);
/* Utils::saveCloud's vertices, 16-byte records (float x, y, z; uint8 r, g, b, a = 255).  inlier_dev != NULL (the flags of
 * rcn_ba_session_validity, uploaded by the caller): the L landmarks with every outlier painted (253, 0, 0), the same L landmarks
 * in their own colours, then one vertex per camera at -R^T t (fp64, each component one ascending sum of rounded products),
 * coloured (0, 250, 0), in the caller's order; NULL: the landmarks, then the cameras.  xyz_dev: what
 * rcn_ba_session_points_device returns.  *n_vertices_out (host): 2 L + C or L + C, written before the call returns. */
int  rcn_cloud_vertices_device(rcn_ctx *ctx, const double *xyz_dev /*[L][3]*/, const uint8_t *lm_rgba_dev /*[L][4]*/, const uint8_t *inlier_dev,
                               int32_t L, const double *poses34_dev /*[C][12]*/, int32_t C, void *vertices_out_dev, int64_t *n_vertices_out);
/* Host code: a PLY file of those records (property float x / y / z, uchar red / green / blue / alpha), ASCII or
 * binary_little_endian.  RCN_ERR_IO when the file cannot be written. */
int  rcn_cloud_write_ply(const char *path, const void *vertices_host, int64_t n_vertices, int32_t binary);

/* ---- ORB: FeatureClassic's second detector (the cv::ORB::create() of FeatureDetector.cpp:9, :19) ----------------------
 * Oriented FAST and rotated BRIEF with cv::ORB::create()'s defaults, restated in tests/orb_ref.py (what
 * could not be pinned against OpenCV itself is listed in section 1).  Fixed: firstLevel 0, WTA_K 2, Harris score, patch 31.
 * Integer arithmetic throughout, except the Harris response and the patch direction, which are single correctly rounded fp64
 * operations without contraction: every output equals the restatement bit for bit (angle, informative only: 1 fp32 ulp).
 * An image's result does not depend on the batch, the chunking, the strides, the input type of equal values or the run.
 *
 * Packed byte pyramid of one image: level l is level_h[l] x level_w[l] bytes at level_offset[l] (a multiple of 16),
 * bytes_per_image in all; level 0 is the image (a float image converted round-half-even, clamped), level l is level l - 1
 * through the 8-bit bilinear resize of rcn_img_prepare_device.  Score maps (rcn_orb_fast_device) have the same layout.
 * rcn_orb_layout and rcn_orb_default_pattern are pure host code (no device needed).
 *
 * Capacity: FAST corners after the strict 3 x 3 maximum are at most one per 2 x 2 pixels, and the lists hold that many, so
 * they cannot overflow.  Of those, a level keeps the ones at or above its 2 * quota-th largest FAST score; when ties make
 * that more than RCN_ORB_MAX_SURVIVORS on one level the image reports counts = -1 and no rows. */
#define RCN_ORB_MAX_LEVELS 16
#define RCN_ORB_MAX_SURVIVORS 8192
#define RCN_ORB_INPUT_F32 0              /* pixels on the 0..255 scale, finite */
#define RCN_ORB_INPUT_U8  1
typedef struct {
    int32_t nfeatures;                   /* 500, >= 1 */
    int32_t nlevels;                     /* 8, 1..RCN_ORB_MAX_LEVELS */
    int32_t edge_threshold;              /* 31, 22..4096: the rotated tests reach 22 pixels */
    int32_t fast_threshold;              /* 20, 1..254 */
    double  scale_factor;                /* 1.2, > 1 and <= 4 */
    const int8_t *pattern;               /* host: 256 tests (x0, y0, x1, y1), every |coordinate| <= 15; NULL: rcn_orb_default_pattern */
} rcn_orb_options;
typedef struct {
    int32_t n_levels, reserved;
    int32_t level_h[RCN_ORB_MAX_LEVELS], level_w[RCN_ORB_MAX_LEVELS];
    int32_t quota[RCN_ORB_MAX_LEVELS];   /* cv::ORB's geometric split of nfeatures */
    int32_t active[RCN_ORB_MAX_LEVELS];  /* 0: min(h, w) <= 2 * edge_threshold, the level yields no keypoints */
    float   scale[RCN_ORB_MAX_LEVELS];   /* float(pow(double(scale_factor), l)) */
    int64_t level_offset[RCN_ORB_MAX_LEVELS];
    int64_t bytes_per_image;
} rcn_orb_pyramid_layout;
void rcn_orb_default_options(rcn_orb_options *opt);
const int8_t *rcn_orb_default_pattern(void);   /* 1024 bytes: a BRIEF pattern of Gaussian points clipped to +-13 (tests/orb_ref.py::default_pattern) */
/* opt == NULL: the defaults.  RCN_ERR_ARG: an option out of range, H or W < 1 or > 65535 (a keypoint's level coordinates are
 * packed into 16 bits each), H W > 2^31 - 1, an empty level, a level
 * that halves the one before it on both axes (cv::resize takes another path there), a pattern coordinate beyond +-15. */
int  rcn_orb_layout(int32_t H, int32_t W, const rcn_orb_options *opt, rcn_orb_pyramid_layout *out);
/* images per pass over the ctx's workspace (<= 0: as many as fit its default cap of 1 GiB) */
int  rcn_orb_set_chunk_images(rcn_ctx *ctx, int32_t images);
/* images_dev: n grey images [H][W] addressed by ELEMENT strides (image, y, x), as the SIFT calls read them.
 * pyr_out_dev: [n][bytes_per_image].  Asynchronous on the ctx stream (the resize tables of a new size are uploaded first: waits once). */
int  rcn_orb_pyramid_device(rcn_ctx *ctx, const void *images_dev, int32_t input_dtype, int64_t stride_img, int64_t stride_y,
                            int64_t stride_x, int32_t n, int32_t H, int32_t W, const rcn_orb_options *opt, uint8_t *pyr_out_dev);
/* For inspection: the FAST-9/16 score of every pixel of every level (the largest t >= fast_threshold at which it is still a
 * corner, 0 for none and within 3 pixels of the border), before the 3 x 3 maximum.  scores_out_dev: [n][bytes_per_image]. */
int  rcn_orb_fast_device(rcn_ctx *ctx, const uint8_t *pyr_dev, int32_t n, int32_t H, int32_t W, const rcn_orb_options *opt,
                         uint8_t *scores_out_dev);
/* Keypoints in ascending order of (level, y, x); counts[i] is the uncapped number (it may exceed nfeatures: ties are kept) --
 * when it exceeds K the K largest by (response descending, canonical rank ascending) are emitted, still in canonical order.
 * xy = (x, y) * scale[level], size = 31 * scale[level], octave = level, angle in degrees in [0, 360), response the Harris
 * response rounded to fp32.  Rows past min(counts[i], K): xy and xy_int (-1, -1), the other fields 0. */
int  rcn_orb_detect_device(rcn_ctx *ctx, const uint8_t *pyr_dev, int32_t n, int32_t H, int32_t W, const rcn_orb_options *opt, int32_t K,
                           float *xy_dev /*[n][K][2]*/, int32_t *xy_int_dev /*[n][K][2]*/, float *size_dev /*[n][K]*/,
                           float *angle_dev /*[n][K]*/, float *response_dev /*[n][K]*/, int32_t *octave_dev /*[n][K]*/,
                           int32_t *counts_dev /*[n]*/);
/* 32 floats in 0..255 per keypoint (the bytes of the descriptor converted to CV_32F, FeatureDetector.cpp:24), rows past
 * min(counts[i], K) zero; bytes_out_dev (may be NULL): the same bytes packed, [n][K][32]. */
int  rcn_orb_describe_device(rcn_ctx *ctx, const uint8_t *pyr_dev, int32_t n, int32_t H, int32_t W, const rcn_orb_options *opt, int32_t K,
                             const float *xy_dev, const int32_t *octave_dev, const int32_t *counts_dev, float *rows_out_dev /*[n][K][32]*/,
                             uint8_t *bytes_out_dev);
/* The three in one call, the pyramid in the ctx's workspace: bit for bit the three calls. */
int  rcn_orb_detect_and_compute_device(rcn_ctx *ctx, const void *images_dev, int32_t input_dtype, int64_t stride_img, int64_t stride_y,
                                       int64_t stride_x, int32_t n, int32_t H, int32_t W, const rcn_orb_options *opt, int32_t K,
                                       float *xy_dev, int32_t *xy_int_dev, float *size_dev, float *angle_dev, float *response_dev,
                                       int32_t *octave_dev, int32_t *counts_dev, float *rows_out_dev, uint8_t *bytes_out_dev);

/* ---- track building (tracks.hip) -----------------------------------------------------------------------
 * The tracks that the resident match lists (rcn_match_lists_upload) tie together across all their images, as OpenMVG's
 * TracksBuilder computes them, restated in tests/tracks_ref.py; pure integer set arithmetic, every output bit for bit.
 *   nodes       one per (image, feature): every image of the resident lists, feature 0 .. K - 1 of its resident coordinates
 *   edges       every entry (f, g) of every uploaded list (a, b) joins (a, f) and (b, g); `mirror` adds nothing
 *   conflict    a connected component in which an image occurs with two or more features: RCN_TRACKS_CONFLICT_DROP_TRACK drops the
 *               component, RCN_TRACKS_CONFLICT_DROP_IMAGE every observation of such an image in it
 *   selection   n_sel > 0: observations of images outside sel_img are dropped AFTER the conflict rule (an unselected image still
 *               ties tracks together and still conflicts); sel_cam[k] is the camera row of sel_img[k]
 *   length      a track is kept when min_length <= n and (max_length == 0 or n <= max_length), n the surviving observations
 *   order       observations ascend by (image id, feature), tracks by their first surviving observation
 * Node index: the list images ascending by id, node_off[i] + feature (rcn_tracks_layout, host only: img_ids_out n_images entries,
 * node_off_out n_images + 1; either may be NULL to ask for *n_images_out alone).
 *
 * rcn_tracks_build_device: asynchronous on the ctx stream behind one small staged host-to-device copy (the slot / selection table);
 * no host synchronisation inside.  counts_dev[0 .. 1]: tracks and observations of the FULL result, also beyond the capacities.
 * Only whole tracks are written: track j iff tracks 0 .. j fit both capacities; trk_off_dev has cap_tracks + 1 entries, the ones
 * past the last written track repeat its end (rcn_new_view_tracks_device's convention: rcn_triangulate_device can run over all
 * cap_tracks rows).  obs_img_dev / obs_feat_dev [cap_obs]; obs_cam_dev [cap_obs] (may be NULL, must be NULL when n_sel == 0);
 * obs_xy_dev [cap_obs][2] (may be NULL): the resident pixels; feat_track_dev (may be NULL): one int32 per node, the WRITTEN
 * track's index or -1; stats_dev (may be NULL) int64[8]: components of at least 2 nodes, components with a conflict,
 * observations dropped by the conflict rule, components of at least 2 nodes (not dropped whole by the conflict rule) that the
 * length filter dropped, the largest component's nodes, the longest kept track, the edges read, 0.
 * rcn_tracks_build: the same with host arrays, synchronous; too small a capacity is RCN_ERR_ARG with counts_out set.
 * RCN_ERR_ARG (with a message): no resident lists, coordinates changed since the lists' upload, a repeated selected image, a negative
 * camera row, more than 2^31 - 1 nodes, bad options (min_length < 2, max_length < 0 or in 1 .. min_length - 1, an unknown policy, a
 * non-zero reserved word), a negative capacity, a null required pointer.  RCN_ERR_NOT_FOUND: a selected image that is not among
 * the list images.  opt == NULL: the defaults. */
#define RCN_TRACKS_CONFLICT_DROP_TRACK 0
#define RCN_TRACKS_CONFLICT_DROP_IMAGE 1
typedef struct {
    int32_t min_length;                  /* 2, >= 2 */
    int32_t max_length;                  /* 0: no limit */
    int32_t conflict;                    /* RCN_TRACKS_CONFLICT_DROP_TRACK */
    int32_t reserved;                    /* 0 */
} rcn_tracks_options;
void rcn_tracks_default_options(rcn_tracks_options *opt);
int  rcn_tracks_layout(rcn_ctx *ctx, int32_t *img_ids_out, int64_t *node_off_out, int32_t *n_images_out);
int  rcn_tracks_build_device(rcn_ctx *ctx, const rcn_tracks_options *opt, int32_t n_sel, const int32_t *sel_img_host,
                             const int32_t *sel_cam_host, int32_t cap_tracks, int32_t cap_obs, int32_t *counts_dev,
                             int32_t *trk_off_dev, int32_t *obs_img_dev, int32_t *obs_feat_dev, int32_t *obs_cam_dev,
                             int32_t *obs_xy_dev, int32_t *feat_track_dev, int64_t *stats_dev);
int  rcn_tracks_build(rcn_ctx *ctx, const rcn_tracks_options *opt, int32_t n_sel, const int32_t *sel_img, const int32_t *sel_cam,
                      int32_t cap_tracks, int32_t cap_obs, int32_t *counts_out, int32_t *trk_off_out, int32_t *obs_img_out,
                      int32_t *obs_feat_out, int32_t *obs_cam_out, int32_t *obs_xy_out, int32_t *feat_track_out, int64_t *stats_out);
/* Milliseconds the six phases of the last rcn_tracks_build* of this ctx took on the device (hook, flatten, conflicts, scans,
 * scatter, sort); waits for them.  RCN_ERR_ARG before the first build. */
int  rcn_tracks_last_phase_ms(rcn_ctx *ctx, double *ms_out6);

/* ---- plane-sweep depth maps, the cross-view check and the dense cloud ----------------------------------
 * The adjusted cameras and the prepared photographs -> per-view depth maps and a dense coloured cloud: the classical
 * fronto-parallel plane sweep with a ZNCC cost, a winner-takes-all depth, a consistency check against the source views' own
 * maps and a direct fusion.  Defined by tests/mvs_ref.py; every output array equals it bit for bit (integer window sums, each
 * floating-point step one separately rounded double in the order of csrc/mvs_geom.h).
 *
 * Cameras: poses34 rows of [R | t] (world -> camera) and intrinsics rows of six (fx fy cx cy k1 k2), as the BA session holds
 * them.  The sweep is pinhole; rcn_img_undistort_device removes k1, k2 beforehand: out[y][x] = the 5-bit bilinear sample of
 * the distorted plane at (fx (xn + d) + cx, fy (yn + d) + cy), xn = (x - cx) / fx, d = k1 rho + (k2 rho) rho, rho = xn^2 + yn^2,
 * rounded by (v + 512) >> 10, 0 outside; the identity when k1 = k2 = 0.  out: dense [n][rows][cols][channels].
 *
 * Planes: per reference view a list inv[D] of inverse depths (any order, repeats allowed; rcn_mvs_inv_depths: uniform in
 * inverse depth from 1 / far up to 1 / near, the middle when D == 1).  rcn_mvs_homographies (pure host code, no contraction):
 * H_out[s][k] = K_s (R_rel + t_rel e3^T inv[k]) K_r^-1 row-major, zeros for a source < 0.
 *
 * Views: views_host [V][1 + S] = (reference image, S source images, -1: none).  rcn_mvs_sweep_device: one launch for the V
 * views; a view's bits do not depend on the batch.  plane_out int16 (-1: invalid), depth_out float (0: invalid), cost_out
 * float (+inf: invalid), each dense [V][rows][cols].  rcn_mvs_consistency_device: mask_out uint8 [V][rows][cols], counts_out
 * int32 [V]; a source that is no reference view of the batch agrees with nothing.  rcn_mvs_fuse_device: the kept pixels of
 * every stride-th row and column as rcn_cloud_write_ply's 16-byte records in (view, y, x) order; only whole rows are written:
 * row j iff rows 0 .. j fit `capacity`; counts_out_dev int64[2] = (vertices written, vertices of the full result).  rgb_dev
 * [n][rows][cols][3] may be NULL (black).  All three are asynchronous on the ctx stream behind one small staged copy of the
 * view table.  opt == NULL: the defaults.
 * RCN_ERR_ARG (with a message): a null required pointer, radius outside 1 .. 5, D outside 1 .. 1024, S outside 1 .. 16, a
 * reference listed as its own source, an image index outside the batch, a non-positive size, rows * cols > 2^29 - 1, more than
 * 65535 views or 2^24 - 1 tiles / sampled rows in one launch, a bad option.  V == 0 launches nothing. */
#define RCN_MVS_MAX_PLANES 1024
#define RCN_MVS_MAX_SOURCES 16
typedef struct {
    int32_t radius;                      /* 3: the ZNCC window is (2 radius + 1)^2, 1 .. 5 */
    int32_t min_sources;                 /* 2: a plane's cost is +inf with fewer valid sources */
    int32_t min_consistent;              /* 2: sources that must agree with a pixel's depth */
    int32_t stride;                      /* 1: the fusion takes every stride-th row and column */
    double max_cost;                     /* 0.5: a pixel whose best cost exceeds it is invalid */
    double rel_tol;                      /* 0.01: |z_s - z'_s| <= rel_tol z_s */
} rcn_mvs_options;
typedef struct {
    int32_t tile, tiles_x, tiles_y;      /* the sweep's tile edge and tiles per view */
    int32_t lds_bytes;                   /* LDS of one workgroup of k_mvs_sweep */
    int64_t pixels;                      /* V rows cols: elements of plane / depth / cost / mask */
    int64_t h_doubles;                   /* V S D 9: doubles of the homography table */
    int64_t samples;                     /* pixels D S: warped samples of a full sweep */
} rcn_mvs_sizes;
void rcn_mvs_default_options(rcn_mvs_options *opt);
int  rcn_mvs_layout(int32_t rows, int32_t cols, int32_t V, int32_t D, int32_t S, int32_t radius, rcn_mvs_sizes *out);
int  rcn_mvs_inv_depths(double near_z, double far_z, int32_t D, double *inv_out);
int  rcn_mvs_homographies(const double *poses34, const double *intrinsics, int32_t ref, const int32_t *srcs, int32_t S, const double *inv, int32_t D,
                          double *H_out /*[S][D][9]*/);
int  rcn_img_undistort_device(rcn_ctx *ctx, const uint8_t *src_dev, int64_t stride_img_bytes, int64_t stride_row_bytes, int32_t channels /*1 | 3*/, int32_t n,
                              int32_t rows, int32_t cols, const double *intrinsics_dev /*[n][6]*/, uint8_t *out_dev);
int  rcn_mvs_sweep_device(rcn_ctx *ctx, const uint8_t *gray_dev, int64_t stride_img_bytes, int64_t stride_row_bytes, int32_t n_images, int32_t rows, int32_t cols,
                          const int32_t *views_host, int32_t V, int32_t S, const double *H_dev /*[V][S][D][9]*/, const double *inv_dev /*[V][D]*/, int32_t D,
                          const rcn_mvs_options *opt, int16_t *plane_out_dev, float *depth_out_dev, float *cost_out_dev);
int  rcn_mvs_consistency_device(rcn_ctx *ctx, const int32_t *views_host, int32_t V, int32_t S, const double *poses34_dev, const double *intrinsics_dev,
                                int32_t n_images, int32_t rows, int32_t cols, const int16_t *plane_dev, const float *depth_dev, const rcn_mvs_options *opt,
                                uint8_t *mask_out_dev, int32_t *counts_out_dev);
int  rcn_mvs_fuse_device(rcn_ctx *ctx, const int32_t *views_host, int32_t V, int32_t S, const double *poses34_dev, const double *intrinsics_dev, int32_t n_images,
                         const uint8_t *rgb_dev, int32_t rows, int32_t cols, const float *depth_dev, const uint8_t *mask_dev, const rcn_mvs_options *opt,
                         int64_t capacity, void *vertices_out_dev, int64_t *counts_out_dev);
/* Sources and depth ranges for every camera of a session in one call, computed on the device: sources_out [n_cams][S] = each
 * camera's S most covisible cameras (rcn_ba_session_covisible's rule: shared landmarks descending, ties to the lower index,
 * -1 where fewer share any); range_out [n_cams][2] = the smallest and largest positive camera-frame depth
 * ((P[8] X + P[9] Y) + P[10] Z) + P[11] of the landmarks it observes, (0, 0) when there is none; covisible_out (may be NULL)
 * [n_cams][n_cams]: the shared-landmark counts, the diagonal a camera's own landmarks.  poses34_host: the cameras as the
 * pipeline holds them, as rcn_ba_session_validity takes them.  Waits.  The caller widens the range by a factor of its choice. */
int  rcn_ba_session_mvs_views(rcn_ba_session *s, const double *poses34_host, int32_t S, int32_t *sources_out, double *range_out, int32_t *covisible_out);

#ifdef __cplusplus
}
#endif
#endif /* RCN_H */
