/*
 * sfmcore.h — C-ABI of the MI355X matching / geometric-verification / BA-J^TJ core.
 *
 * This is the drop-in boundary behind the reference's Python call signatures.
 * The reference has no FFI of its own: its arithmetic is OpenCV, reached by star-import
 * (code/pipeline.py:1-3).  Each entry point below names the reference interface it replaces;
 * INTEGRATION.md shows the ctypes binding (sfm-project_amd/sfmcore.py) that the reference-side
 * modules feature_matching / geometric_verification / 3d_reconstruction call through.
 *
 * Conventions
 *   - Plain pointers and sizes only.  Every array argument is a DEVICE pointer (hipMalloc'd or a
 *     torch.cuda tensor's data_ptr), C-contiguous, caller-owned.
 *   - Work is enqueued on the context's stream: a non-blocking stream the context creates, until
 *     sfm_ctx_set_stream selects another (NULL selects the legacy default stream, which is what
 *     torch's default stream is).  Entry points return after enqueueing; sfm_ctx_sync waits.
 *   - Return 0 (SFM_OK) on success, < 0 on error; sfm_last_error() gives a thread-local message.
 *     No C++ exception crosses the ABI.  No callbacks.
 *   - A context is bound to one device and must not be used from two threads at once.
 */
#ifndef SFMCORE_H
#define SFMCORE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SFM_OK 0
#define SFM_ERR_INVALID (-1)     /* bad argument (shape, null pointer, unsupported combination) */
#define SFM_ERR_HIP (-2)         /* HIP runtime error (message in sfm_last_error) */
#define SFM_ERR_NOMEM (-3)       /* device workspace allocation failed */

#define SFM_METRIC_L2 0          /* u8 x 128 (SIFT-like), squared Euclidean distance */
#define SFM_METRIC_HAMMING 1     /* u8 x 32 (ORB 256-bit), Hamming distance */

#define SFM_XC_NONE 0            /* no cross check */
#define SFM_XC_MUTUAL 1          /* strict mutual nearest neighbours, lowest index on ties */
#define SFM_XC_OPENCV 2          /* OpenCV batchDistance cross-check rule (BFMatcher crossCheck) */

typedef struct sfm_ctx sfm_ctx;

typedef struct sfm_match_params {
    int32_t metric;        /* SFM_METRIC_* */
    int32_t cross_check;   /* SFM_XC_* */
    int32_t ratio_num;     /* Lowe ratio r = num/den on (unsquared) distances; den = 0: off */
    int32_t ratio_den;
    int64_t max_dist;      /* keep distance < max_dist (d^2 for L2, bits for Hamming); < 0: off */
} sfm_match_params;

typedef struct sfm_ransac_params {
    int32_t n_hyp;         /* hypotheses per pair (multiple of 256) */
    int32_t min_inliers;   /* pair verified iff best count >= min_inliers */
    float thr;             /* Sampson-error threshold in squared pixels */
    int32_t _pad;
    uint64_t seed;         /* RANSAC seed; hypothesis h of pair (a,b) uses Philox key=seed,
                              counter=(h, 0|1, a, b): results are shard-invariant */
} sfm_ransac_params;

/* ---- context ---------------------------------------------------------------------------- */
int sfm_ctx_create(int32_t device, sfm_ctx** out);
int sfm_ctx_destroy(sfm_ctx* ctx);
int sfm_ctx_set_stream(sfm_ctx* ctx, void* hip_stream);   /* hipStream_t; NULL = default stream */
int sfm_ctx_sync(sfm_ctx* ctx);
const char* sfm_last_error(void);
int32_t sfm_version(void);

/* ---- matching -----------------------------------------------------------------------------
 * Replaces cv2.BFMatcher(normType, crossCheck).match(des1, des2) + the distance filter of
 * code/feature_matching.py:48-58 (extract_and_match, called per ordered pair from
 * code/pipeline.py:41), batched over a pair list.
 *   desc      [n_img][k_max][dim] u8  (dim = 128 for L2, 32 for Hamming)
 *   n_kp      [n_img] i32             valid descriptors per image (<= k_max)
 *   pairs     [n_pairs][2] i32        (query image a, train image b)
 *   out_count [n_pairs] i32           matches per pair
 *   out_match [n_pairs][k_max][2] i32 (queryIdx, trainIdx), ascending queryIdx
 *   out_dist  [n_pairs][k_max] i32    d^2 (L2) or Hamming distance
 * Limits: k_max <= 8192.  L2 above 4096 needs a cross-check rule (SFM_XC_MUTUAL / SFM_XC_OPENCV:
 * the column-winner kernel); the ratio-only and no-rule L2 paths stop at 4096.  Hamming above
 * 4096 runs the VALU popcount kernel.
 */
int sfm_match_batch(sfm_ctx* ctx, const uint8_t* desc, const int32_t* n_kp, int32_t n_img,
                    int32_t k_max, int32_t dim, const int32_t* pairs, int32_t n_pairs,
                    const sfm_match_params* prm, int32_t* out_count, int32_t* out_match,
                    int32_t* out_dist);
/* Both orders of every pair from one distance tile: the reference enumerates ORDERED pairs i != j
 * (code/pipeline.py:38-41) and matches each with BFMatcher(crossCheck=True)
 * (code/feature_matching.py:48-50); (a, b) and (b, a) share every distance.  pairs [n_pairs][2]
 * (a, b); outputs hold 2 * n_pairs results: slot p = sfm_match_batch on (a, b), slot n_pairs + p =
 * sfm_match_batch on (b, a), bit for bit (out_count [2 n_pairs], out_match [2 n_pairs][k_max][2],
 * out_dist [2 n_pairs][k_max]).  Any cross_check rule and max_dist; no ratio test (ratio_den
 * must be 0: the reverse direction's ratio needs its own second-best neighbour); k_max <= 4096. */
int sfm_match_batch_both(sfm_ctx* ctx, const uint8_t* desc, const int32_t* n_kp, int32_t n_img,
                         int32_t k_max, int32_t dim, const int32_t* pairs, int32_t n_pairs,
                         const sfm_match_params* prm, int32_t* out_count, int32_t* out_match,
                         int32_t* out_dist);

/* ---- geometric verification -----------------------------------------------------------------
 * Fills the empty code/geometric_verification.py (placeholder comment at code/pipeline.py:60):
 * 8-point fundamental-matrix RANSAC per pair on the tentative matches of sfm_match_batch.
 *   kps           [n_img][k_max][2] f32 pixel coordinates
 *   match_count / matches: as written by sfm_match_batch
 *   out_inl_count [n_pairs] i32  best inlier count (-1 if fewer than 8 matches)
 *   out_best_h    [n_pairs] i32  winning hypothesis id (lowest id among equal counts)
 *   out_mask      [n_pairs][k_max] u8  inlier flag per tentative match
 *   out_F         [n_pairs][9] f32  F in normalised coordinates (row-major)
 *   out_norm      [n_pairs][6] f32  (cx1, cy1, s1, cx2, cy2, s2) normalisation of each side
 */
int sfm_ransac_f_batch(sfm_ctx* ctx, const float* kps, int32_t n_img, int32_t k_max,
                       const int32_t* pairs, int32_t n_pairs, const int32_t* match_count,
                       const int32_t* matches, const sfm_ransac_params* prm,
                       int32_t* out_inl_count, int32_t* out_best_h, uint8_t* out_mask,
                       float* out_F, float* out_norm);

/* fp64 mode of sfm_ransac_f_batch (SURVEY.md §8b's f64 coordinates / F): the same spec, sampler,
 * schedule and outputs with every floating-point operation of normalisation, 8-point fit, rank-2
 * step and Sampson test in double (the oracle's *_f64 restatement is bit-identical).  kps
 * [n_img][k_max][2] f64; out_F [n_pairs][9] f64; out_norm [n_pairs][6] f64; the ordered schedule
 * only (SFM_RANSAC_MODE is ignored).
 */
int sfm_ransac_f_batch_f64(sfm_ctx* ctx, const double* kps, int32_t n_img, int32_t k_max,
                           const int32_t* pairs, int32_t n_pairs, const int32_t* match_count,
                           const int32_t* matches, const sfm_ransac_params* prm,
                           int32_t* out_inl_count, int32_t* out_best_h, uint8_t* out_mask,
                           double* out_F, double* out_norm);

/* Diagnostic companion of sfm_ransac_f_batch: the inlier count of EVERY hypothesis (no pruning),
 * out_counts [n_pairs][n_hyp] i32 (-1: degenerate sample or fewer than 8 matches), computed by the
 * score kernel of sfm_ransac_f_batch with pruning off; out_norm as above.  Optional (NULL: not
 * written): out_hyp_F [n_pairs][n_hyp][9] f32, every hypothesis's F in normalised coordinates;
 * out_hyp_mask [n_pairs][n_hyp][k_max] u8, every hypothesis's inlier decision per match.  The
 * exhaustive parity tests compare them with the oracle's and with scikit-image's estimates.
 */
int sfm_ransac_counts(sfm_ctx* ctx, const float* kps, int32_t n_img, int32_t k_max,
                      const int32_t* pairs, int32_t n_pairs, const int32_t* match_count,
                      const int32_t* matches, const sfm_ransac_params* prm, int32_t* out_counts,
                      float* out_norm, float* out_hyp_F, uint8_t* out_hyp_mask);

/* Execution statistics of sfm_ransac_f_batch (measurement, default off).  enable != 0: every later
 * batch on ctx adds its Sampson evaluations to device counters (one u32 store per score wave + a
 * small reduction kernel on the context's stream).  out != NULL: synchronises the stream, writes
 * (executed evaluations, algorithmic evaluations = n_hyp x M summed over pairs with M >= 8, number
 * of such pairs) and resets the counters.  executed / algorithmic is the share of the Sampson work
 * the exact pruning did not skip.
 */
int sfm_ransac_stats(sfm_ctx* ctx, int32_t enable, uint64_t* out);
/* Diagnostic companion of sfm_ransac_stats: the last counted sfm_ransac_f_batch{,_f64} batch's
 * per-wave counts (host out [n_pairs][n_hyp / 64] u32: matches the score wave scored past the
 * preview; entries of pairs with < 8 matches are undefined).  n_pairs / n_hyp must equal that
 * batch's; no other sfm_* call on ctx in between (the counts live in its workspace).
 * Synchronises the stream.  executed = Σ_{M>=8} n_hyp·min(128, M) + 64·Σ_w out[p][w] + M. */
int sfm_ransac_wave_stops(sfm_ctx* ctx, int32_t n_pairs, int32_t n_hyp, uint32_t* out);

/* Homography RANSAC: the second model of two-view verification (papers/schoenberger2016sfm.pdf
 * §4.1).  An F is not identifiable on a planar scene or under pure rotation; the
 * ratio of this count to sfm_ransac_f_batch's tells such pairs apart.  Inputs exactly as
 * sfm_ransac_f_batch (n_hyp a multiple of 256, <= 65536); prm->thr is the FORWARD TRANSFER ERROR
 * |H x1 - x2|^2 in squared pixels of image 2; prm->min_inliers is not read.
 *   sampler   4 distinct matches (Floyd, as the F sampler) from ONE Philox block, key = seed,
 *             counter = (h, 2, a, b): stream 2, disjoint from F's 0 and 1; shard-invariant
 *   fit       null vector of the 8x9 DLT system of the 4 Hartley-normalised correspondences
 *             (rows (x,y,1,0,0,0,-x'x,-x'y,-x') and (0,0,0,x,y,1,-y'x,-y'y,-y')), Householder QR
 *   validity  count -1 if the QR breaks down, an entry of H is not finite, or the 4 sample points
 *             do not share one strict sign of w = h31 x + h32 y + h33
 *   inlier    sign(w) equals the sample's and (u - x2 w)^2 + (v - y2 w)^2 - thr s2^2 w^2 < 0 with
 *             (u, v, w) = H (x1, y1, 1) in normalised coordinates (division-free)
 *   winner    max count, lowest h among equal counts
 *   out_inl_count [n_pairs] i32  best count (-1 if fewer than 4 matches; 0 if no valid hypothesis)
 *   out_best_h    [n_pairs] i32  winning hypothesis id (-1 if fewer than 4 matches)
 *   out_mask      [n_pairs][k_max] u8  inlier flag per tentative match; the whole row is
 *                                   written, zero from match_count on
 *   out_H         [n_pairs][9] f32  H in normalised coordinates, row-major, exactly as fitted
 *                                   (zero if fewer than 4 matches or no valid hypothesis)
 *   out_norm      [n_pairs][6] f32  as sfm_ransac_f_batch, bit-identical for >= 8 matches; the
 *                                   same rule down to 4 matches, zero below
 * Does not touch the sfm_ransac_stats counters.
 */
int sfm_ransac_h_batch(sfm_ctx* ctx, const float* kps, int32_t n_img, int32_t k_max,
                       const int32_t* pairs, int32_t n_pairs, const int32_t* match_count,
                       const int32_t* matches, const sfm_ransac_params* prm,
                       int32_t* out_inl_count, int32_t* out_best_h, uint8_t* out_mask,
                       float* out_H, float* out_norm);

/* Diagnostic companion of sfm_ransac_h_batch: the count of EVERY hypothesis (no pruning),
 * out_counts [n_pairs][n_hyp] i32 (-1: invalid hypothesis or fewer than 4 matches), by the batch's
 * kernel with pruning off; out_norm as above.  Optional (NULL: not written): out_hyp_H
 * [n_pairs][n_hyp][9] f32, every hypothesis's H in normalised coordinates (zero where the count
 * is -1).
 */
int sfm_ransac_h_counts(sfm_ctx* ctx, const float* kps, int32_t n_img, int32_t k_max,
                        const int32_t* pairs, int32_t n_pairs, const int32_t* match_count,
                        const int32_t* matches, const sfm_ransac_params* prm, int32_t* out_counts,
                        float* out_norm, float* out_hyp_H);

/* Two-view relative pose of verified pairs (papers/schoenberger2016sfm.pdf
 * §4.1-4.2): linear essential fit over the F inliers, the four (R, t) decompositions, the
 * cheirality vote and the triangulation (ray) angle.  fp64 throughout, in a fixed operation order:
 * tests/pose_ref.c states it and the results equal it bit for bit, whatever the batch.
 *   kps, n_img, k_max, pairs, n_pairs, match_count, matches   as sfm_ransac_f_batch (k_max <= 8192)
 *   mask [n_pairs][k_max] u8, inl_count [n_pairs] i32         that call's outputs
 *   intr [n_img][4] f64                                       (f, k1, cx, cy) per image
 *   coordinates  x_d = (kp - (cx, cy)) / f, undistorted by sfm_triangulate's rule (10 fixed-point
 *                steps of x = x_d / (1 + k1 |x|^2) from x = x_d), once per keypoint per call
 *   fit          N = A^T A over the masked-in matches, rows (x2x x1x, x2x x1y, x2x, x2y x1x,
 *                x2y x1y, x2y, x1x, x1y, 1), fixed-order sums; E = eigenvector of N's smallest
 *                eigenvalue (cyclic Jacobi, lowest index among equal eigenvalues), unit norm
 *   candidates   from the eigenvectors of E^T E: 0 (U W V^T, +u3), 1 (U W V^T, -u3),
 *                2 (U W^T V^T, +u3), 3 (U W^T V^T, -u3); x2 ~ R x1 + t, |t| = 1
 *   cheirality   n_front[c] = inliers with both depths > 0 under candidate c (division-free);
 *                best = the largest, lowest c on ties
 *   ray angle    per inlier in front under best, between R (x1, 1) and (x2, 1): key = sin^2 up to
 *                90 degrees, 2 - sin^2 above (monotone in the angle), rounded to f32
 *   out_E [n_pairs][9], out_R [n_pairs][9] f64 row-major, out_t [n_pairs][3] f64
 *   out_stat [n_pairs][8] i32 = {status, best, n_front[0..3], n_wide, inliers used}: n_wide = keys
 *                above prm->wide_key; status 0 ok, 1 inl_count < max(prm->min_inliers, 8),
 *                2 degenerate (a vanishing norm while building U); every other output of the pair
 *                is zero unless status is 0
 *   out_median_key [n_pairs] f32  lower median (index (n - 1) / 2 ascending) of those keys
 * On a planar scene or under pure rotation the linear fit's t is not meaningful (under pure
 * rotation R and the near-zero angle are). */
typedef struct sfm_two_view_pose_params {
    int32_t struct_size; /* sizeof(sfm_two_view_pose_params) of the caller: later fields can be
                            added without reading past an older caller's struct */
    int32_t min_inliers;
    float wide_key;      /* sin^2 of the angle a "wide" ray pair must exceed, >= 0 */
} sfm_two_view_pose_params;
int sfm_two_view_pose_batch(sfm_ctx* ctx, const float* kps, int32_t n_img, int32_t k_max,
                            const int32_t* pairs, int32_t n_pairs, const int32_t* match_count,
                            const int32_t* matches, const uint8_t* mask,
                            const int32_t* inl_count, const double* intr,
                            const sfm_two_view_pose_params* prm, double* out_E, double* out_R,
                            double* out_t, int32_t* out_stat, float* out_median_key);

/* Guided matching (COLMAP's guided_matching): re-match verified pairs with the
 * candidates restricted to the epipolar band of the pair's F.  L2 descriptors, dim == 128 only.
 * tests/guided_ref.c states the spec; the outputs equal it byte for byte, whatever the batch.
 *   desc, n_kp, n_img, k_max, dim, pairs, n_pairs   as sfm_match_batch (k_max <= 8192; any a, b in
 *                                                   range, a == b included)
 *   kps [n_img][k_max][2] f32                       pixel coordinates
 *   inl_count [n_pairs] i32, F [n_pairs][9] f32, norm [n_pairs][6] f32
 *                                                   as sfm_ransac_f_batch writes them
 *   skip        a pair gets count 0 and a zero ncand row if inl_count < max(prm->min_inliers, 8),
 *               n_kp[a] == 0, n_kp[b] == 0, s1 == 0 or s2 == 0 (norm = cx1, cy1, s1, cx2, cy2, s2)
 *   candidate   cand(i, j) = K2's Sampson test at prm->thr on keypoint i of a and j of b: with
 *               (k1, k2) = sampson_scales(s1, s2, thr), G = sampson_prep(F, k1, k2) and
 *               X1 = ((x - cx1) s1) k1, ... (f32, each operation rounded), sampson_inlier(G, X1_i,
 *               Y1_i, X2_j, Y2_j) of oracle/sfm_oracle_ransac.inc, the same FMA sequence; a NaN
 *               anywhere gives false (a NaN in F: no candidates, count 0)
 *   matching    sfm_match_batch's non-OpenCV rules on the d^2 matrix with the non-candidates
 *               removed: nn[i] = the candidate of smallest d^2 (lowest j among equals); the ratio
 *               test den^2 d1 < num^2 d2 against the second smallest value of the candidates'
 *               distance multiset (fewer than two candidates: passes); SFM_XC_MUTUAL keeps i iff
 *               the candidate query of smallest d^2 for nn[i] (lowest i among equals) is i;
 *               max_dist >= 0 keeps d1 < max_dist.  A query with a single candidate passes the
 *               ratio test, so callers should set max_dist.
 *   out_count, out_match, out_dist   sfm_match_batch's layout (ascending queryIdx; entries from
 *               count on are unspecified): they feed sfm_ransac_f_batch, sfm_graph_rows* and
 *               sfm_two_view_pose_batch unchanged
 *   out_ncand [n_pairs][k_max] i32   candidates of every query, 0 from n_kp[a] on; may be NULL */
typedef struct sfm_guided_params {
    int32_t struct_size;   /* sizeof(sfm_guided_params) of the caller, as sfm_two_view_pose_params */
    int32_t cross_check;   /* SFM_XC_NONE or SFM_XC_MUTUAL (SFM_XC_OPENCV: SFM_ERR_INVALID) */
    int32_t ratio_num, ratio_den;   /* den = 0: off */
    int32_t min_inliers;
    float   thr;           /* Sampson band in squared pixels, > 0 */
    int64_t max_dist;      /* d^2 < max_dist; < 0: off */
} sfm_guided_params;
int sfm_guided_match_batch(sfm_ctx* ctx, const uint8_t* desc, const int32_t* n_kp,
                           const float* kps, int32_t n_img, int32_t k_max, int32_t dim,
                           const int32_t* pairs, int32_t n_pairs, const int32_t* inl_count,
                           const float* F, const float* norm, const sfm_guided_params* prm,
                           int32_t* out_count, int32_t* out_match, int32_t* out_dist,
                           int32_t* out_ncand);

/* ---- verified match graph -------------------------------------------------------------------
 * Replaces the pair_matches list of code/pipeline.py:42-47 (Pair(img_inx_1, img_inx_2, matches)
 * for every non-empty pair) for a batch: rows (pair_base + pair, queryIdx, trainIdx) of the RANSAC
 * inliers of every pair whose inl_count >= min_inliers, pair-major, ascending match index.
 *   sfm_graph_offsets: out_offsets [n_pairs + 1] i64, exclusive scan of the verified counts
 *                      (out_offsets[n_pairs] = total rows); size out_rows from it.
 *   sfm_graph_rows:    out_rows [total][3] i32; match_count / matches / mask / inl_count as
 *                      written by sfm_match_batch and sfm_ransac_f_batch.
 */
int sfm_graph_offsets(sfm_ctx* ctx, int32_t n_pairs, const int32_t* inl_count,
                      int32_t min_inliers, int64_t* out_offsets);
int sfm_graph_rows(sfm_ctx* ctx, int32_t n_pairs, int32_t k_max, int32_t pair_base,
                   const int32_t* match_count, const int32_t* matches, const uint8_t* mask,
                   const int32_t* inl_count, int32_t min_inliers, const int64_t* offsets,
                   int32_t* out_rows);
/* The multi-GPU exchange form of the same graph (the graph all-gather):
 *   sfm_graph_rows_packed: out_packed [total] u32 = queryIdx << 16 | trainIdx (k_max <= 65536),
 *                          same order and offsets as sfm_graph_rows.
 *   sfm_graph_expand:      rows of n_pairs consecutive pairs back to [total][3] i32: pair p's
 *                          counts[p] packed rows start at packed[src_offsets[p]] (e.g. inside
 *                          the padded per-rank slots of an all-gather) and are written at row
 *                          dst_offsets[p] as (pair_base + p, queryIdx, trainIdx).
 */
int sfm_graph_rows_packed(sfm_ctx* ctx, int32_t n_pairs, int32_t k_max,
                          const int32_t* match_count, const int32_t* matches, const uint8_t* mask,
                          const int32_t* inl_count, int32_t min_inliers, const int64_t* offsets,
                          uint32_t* out_packed);
int sfm_graph_expand(sfm_ctx* ctx, int32_t n_pairs, int32_t pair_base, const int32_t* counts,
                     const int64_t* src_offsets, const int64_t* dst_offsets,
                     const uint32_t* packed, int32_t* out_rows);

/* ---- bundle-adjustment linearisation ---------------------------------------------------------
 * Fills the empty code/3d_reconstruction.py (import commented out at code/pipeline.py:4) with the
 * J^TJ build of papers/schoenberger2016sfm.pdf eq. (1) / §4.4.  Observations must be grouped by
 * point (pt_ptr = CSR row pointer over points, n_pt + 1 entries); cam_ptr/cam_obs is the CSR
 * index of observations by camera.
 *   cams [n_cam][8] f64 (angle-axis, t, f, k1), pp [n_cam][2] f64, pts [n_pt][3] f64
 *   uv [n_obs][2] f64, cam_idx/pt_idx [n_obs] i32
 *   out: U [n_cam][8][8], V [n_pt][3][3], W [n_obs][8][3], gc [n_cam][8], gp [n_pt][3],
 *        res [n_obs][2], cost [1] (0.5 * sum rho)
 */
int sfm_ba_jtj(sfm_ctx* ctx, int32_t n_cam, const double* cams, const double* pp, int32_t n_pt,
               const double* pts, int32_t n_obs, const int32_t* cam_idx, const int32_t* pt_idx,
               const double* uv, const int32_t* pt_ptr, const int32_t* cam_ptr,
               const int32_t* cam_obs, double loss_s, double* U, double* V, double* W,
               double* gc, double* gp, double* res, double* cost);

/* ---- bundle-adjustment step (LM with Schur complement + PCG) ----------------------------------
 * SURVEY.md §8f item 3 ("rest of incremental SfM for cfg5"): the step of paper eq. (1) that the
 * empty code/3d_reconstruction.py would take after the J^TJ build above.  Spec: DESIGN.md §4.5,
 * restated by oracle/ba_lm.py.
 *
 * sfm_ba_solve: solves the Marquardt-damped normal equations of sfm_ba_jtj's blocks,
 *     [U + λ D_U   W ; Wᵀ   V + λ D_V] [dc; dp] = -[gc; gp],  D = clamp(diag, 1e-6, 1e32),
 *   by the Schur complement on the points and block-Jacobi preconditioned CG on the cameras
 *   (S is never formed), then back-substitutes dp.  Same CSR inputs as sfm_ba_jtj
 *   (observations point-major).  Stops when |r| <= tol |b|, after max_iter iterations, or on a
 *   breakdown: p·q <= 0 (S is not positive definite along the search direction) ends the
 *   iteration with α = 0, dc and r being those of the last completed step.  A camera whose
 *   diagonal block S_cc is not positive definite (a pivot of its Cholesky factorisation is not
 *   > 0) is preconditioned by diag(1 / max(S_ii, 1e-6)) instead of S_cc⁻¹ (the fallback).
 *   out (device): dc [n_cam][8], dp [n_pt][3],
 *   info [5] f64 = {CG iterations (the one that broke down included), |r|/|b| of the recurrence
 *   residual of the last completed iteration (always: a breakdown does not read as converged),
 *   gᵀδ, δᵀ JᵀJ δ (undamped), bit set: 1 = preconditioner fallback, 2 = CG breakdown}
 *   — the LM predicted decrease is -(gᵀδ + ½ δᵀ JᵀJ δ).
 * sfm_ba_cost:   cost = 0.5 Σ ρ(|r|²) at the given parameters (no Jacobians).
 * sfm_ba_update: cams_out = cams ⊕ dc (R <- exp([δr]x) R, the tangent space of the Jacobians;
 *   t, f, k1 additive), pts_out = pts + dp.  Out-of-place.
 */
typedef struct sfm_ba_solve_params {
    double lambda;    /* Marquardt damping λ (>= 0) */
    double tol;       /* relative CG residual |r|/|b| */
    int32_t max_iter; /* CG iteration cap */
    int32_t poll;     /* convergence poll: every `poll` > 0 CG iterations the host reads the
                         device's convergence flag (one 4-byte copy + a hipStreamSynchronize) and
                         stops enqueueing once it is set; 0 (the zero-initialised struct) = every
                         SFM_BA_POLL_DEFAULT (8) iterations; < 0 = never: fully asynchronous,
                         capturable in a hip graph (all max_iter iterations are enqueued, the
                         converged ones exit at once).  Results are identical either way.
                         (sfm_version 1 read 0 as "never"; version 2 restores 0 = poll.) */
    int32_t poll_first; /* > 0: the first poll at iteration poll_first, then every `poll` (a
                         caller that expects about as many iterations as its previous solve took
                         polls once, there, instead of at every multiple of `poll`); 0 = at
                         `poll` (sfm_version 5; earlier versions had no such field) */
} sfm_ba_solve_params;
#define SFM_BA_POLL_DEFAULT 8

int sfm_ba_solve(sfm_ctx* ctx, int32_t n_cam, int32_t n_pt, int32_t n_obs,
                 const int32_t* cam_idx, const int32_t* pt_idx, const int32_t* pt_ptr,
                 const int32_t* cam_ptr, const int32_t* cam_obs, const double* U, const double* V,
                 const double* W, const double* gc, const double* gp,
                 const sfm_ba_solve_params* prm, double* dc, double* dp, double* info);
/* Multi-GPU form of sfm_ba_solve (observations sharded by point, one process per
 * GPU), as caller-driven stages so that no callback crosses the ABI: the caller all-reduces
 * (sums over all ranks, in place) the device buffer comm (>= 44 * n_cam doubles) between the
 * stage that fills it and the next one, ordered on the context's stream (e.g. an RCCL all-reduce
 * enqueued on it).  V, W, gp, dp, pt_ptr and the observation arrays are this rank's point shard
 * (indices local to it); U and gc are the GLOBAL camera blocks (sfm_ba_jtj on the shard, an
 * all-reduce of U / gc, then sfm_ba_fix_params).  Sequence (prm / arrays identical in every call;
 * no other sfm_* call on this context in between — the stages share its workspace):
 *   SETUP           -> all-reduce comm[0, 44 n_cam)  -> SETUP_FINISH
 *   for k = 0 .. max_iter-1:
 *     [every prm->poll > 0 iterations, k > 0 (from prm->poll_first when > 0): POLL -> *done
 *      (host int32); stop if 1]
 *     ITER(k)       -> all-reduce comm[0, 8 n_cam)   -> ITER_FINISH(k)
 *   BACKSUB         -> all-reduce comm[0, 2)         -> MODEL   (dc, dp, info as sfm_ba_solve)
 * After each all-reduce every camera-space value is replicated, so every rank takes the same CG
 * decisions (POLL included) and issues the same collectives; dc and info are the same on every
 * rank, dp is the shard's.  Equal to sfm_ba_solve on the whole problem up to the fp64 summation
 * order.  No counterpart in the reference (its BA module is empty). */
#define SFM_BA_STAGE_SETUP 0
#define SFM_BA_STAGE_SETUP_FINISH 1
#define SFM_BA_STAGE_ITER 2
#define SFM_BA_STAGE_ITER_FINISH 3
#define SFM_BA_STAGE_BACKSUB 4
#define SFM_BA_STAGE_MODEL 5
#define SFM_BA_STAGE_POLL 6
#define SFM_BA_STAGE_SCHUR 7   /* explicit S only (sfm_ba_set_schur): after SETUP, exports T's partials */
int sfm_ba_solve_stage(sfm_ctx* ctx, int32_t stage, int32_t k, int32_t n_cam, int32_t n_pt,
                       int32_t n_obs, const int32_t* cam_idx, const int32_t* pt_idx,
                       const int32_t* pt_ptr, const int32_t* cam_ptr, const int32_t* cam_obs,
                       const double* U, const double* V, const double* W, const double* gc,
                       const double* gp, const sfm_ba_solve_params* prm, double* comm, double* dc,
                       double* dp, double* info, int32_t* done);
/* Fixed parameters (the gauge: the reference camera's pose and one translation coordinate of a
 * second camera; known intrinsics f, k1): in place on sfm_ba_jtj's U [n_cam][8][8], W [n_obs][8][3]
 * and g_c [n_cam][8], the rows/columns of the parameters marked in fixed [n_cam][8] (u8, 1 =
 * fixed) become the identity's, their g_c entries and W rows 0 — sfm_ba_solve then returns
 * δ = 0 for them exactly.  Call after sfm_ba_jtj (and after any camera-block all-reduce). */
int sfm_ba_fix_params(sfm_ctx* ctx, int32_t n_cam, int32_t n_obs, const int32_t* cam_idx,
                      const uint8_t* fixed, double* U, double* W, double* gc);
int sfm_ba_cost(sfm_ctx* ctx, int32_t n_cam, const double* cams, const double* pp, int32_t n_pt,
                const double* pts, int32_t n_obs, const int32_t* cam_idx, const int32_t* pt_idx,
                const double* uv, double loss_s, double* cost);
int sfm_ba_update(sfm_ctx* ctx, int32_t n_cam, const double* cams, const double* dc, int32_t n_pt,
                  const double* pts, const double* dp, double* cams_out, double* pts_out);

/* Sharding-invariant sums (chunk mode, sfm_version 3).  The points of the WHOLE problem are cut
 * into n_total fixed chunks (contiguous point ranges; a rank's shard is a run of whole chunks), and
 * every sum that runs over points or observations into a camera-space or scalar value — U / g_c
 * and the cost of sfm_ba_jtj, sfm_ba_cost, the Schur diagonal blocks and b of the solve set-up,
 * the CG product Σ_o u_o, the LM model terms — is computed per chunk (an order that depends only
 * on the chunk's own observations) and the chunk partials are combined by ONE canonical pairwise
 * tree over all n_total chunks: while n > 1, a[i] = a[2i] + a[2i+1] (i < n/2), an odd last
 * element is carried, n = ceil(n/2).  Results are then bit-identical for every split of the
 * chunks over ranks, the single process included.
 *   sfm_ba_set_chunks(ctx, n_chunk, chunk_pt, chunk_obs, n_total, cam_bounds): the next BA calls
 *   on ctx work on a problem holding n_chunk of the chunks; chunk_pt / chunk_obs (host, n_chunk +
 *   1) are their LOCAL point offsets and the matching observation offsets (pt_ptr[chunk_pt[k]];
 *   chunk_pt[0] = 0, chunk_pt[n_chunk] = n_pt, non-decreasing; empty chunks allowed); cam_bounds
 *   (device, [n_cam][n_chunk + 1] i32, caller-owned) are the positions in cam_obs where each
 *   camera's observation list crosses those offsets (the list is ascending, so each chunk's part
 *   is contiguous): cam_bounds[c][0] = cam_ptr[c], cam_bounds[c][n_chunk] = cam_ptr[c + 1].
 *   n_total = 0: the problem is the whole one (n_chunk = n_total chunks), every result is final.
 *   n_total > 0: a shard (export form): sfm_ba_jtj writes U as [n_chunk][n_cam][8][8], gc as
 *   [n_chunk][n_cam][8] and cost as [n_chunk] (chunk partials, combined by the caller after
 *   gathering every rank's chunks in chunk order: sfm_ba_chunk_tree), sfm_ba_cost writes cost
 *   [n_chunk]; the sharded solve's stages write chunk partials to comm and the stages after the
 *   exchange read ALL n_total chunks' partials in chunk order: SETUP -> comm [n_chunk][n_cam][44],
 *   gathered [n_total][n_cam][44] -> SETUP_FINISH; ITER -> [n_chunk][n_cam][8], gathered ->
 *   ITER_FINISH; BACKSUB -> [n_chunk][2], gathered -> MODEL (an all-GATHER instead of the
 *   all-reduce; comm >= n_total * 44 * n_cam doubles).
 *   n_chunk = 0 switches chunk mode off (the default: the round-4 sums).  1 <= n_chunk <= 16.
 *   sfm_ba_chunk_tree(ctx, n_total, n, parts, out): out[i] = canonical tree over k of
 *   parts[k * n + i] (device arrays), i < n — the combine the library applies itself. */
#define SFM_BA_MAX_CHUNKS 16
int sfm_ba_set_chunks(sfm_ctx* ctx, int32_t n_chunk, const int32_t* chunk_pt,
                      const int32_t* chunk_obs, int32_t n_total, const int32_t* cam_bounds);
int sfm_ba_chunk_tree(sfm_ctx* ctx, int32_t n_total, int64_t n, const double* parts, double* out);

/* Explicit reduced camera system (sfm_version 4; needs chunk mode).  The solve forms the
 * off-diagonal Schur blocks T_ij = Σ_p W_pi V_d,p⁻¹ W_pjᵀ once per solve (S_ij = -T_ij, i != j) and
 * runs the CG on S directly — two launches per iteration over 64 B per camera-pair block instead of
 * streaming W (192 B per observation) every iteration.  It pays when the camera-pair products are
 * few against the CG iterations (short tracks); the caller decides (reconstruction.schur_rule).
 *   sfm_ba_set_schur(ctx, n_slot, slot_cam, n_seg, seg, n_inst, inst, row_ptr, n_ent, row_ent,
 *                    n_group, sg_ptr, sg, gk):
 *   slot_cam [n_slot][2] (ci <= cj): the camera pairs (slots) of the WHOLE problem, the same table
 *   on every rank; inst [2][n_inst] (observation a, observation b of one point, LOCAL observation
 *   indices; cam(a) = ci, cam(b) = cj of its slot; a pair within one camera appears as (a, b) and
 *   (b, a)); seg [4][n_seg] (local chunk, slot, first instance, end instance): this problem's
 *   instances grouped by (chunk, slot), each group in point order — a group's T partial is the
 *   fixed-order sum over it; row_ptr [n_cam + 1], row_ent [n_ent] = 2 slot + t: block row c of S
 *   (t = 1: the slot's transpose), in a fixed order.  The groups of the WHOLE problem (every rank's,
 *   in chunk order: a shard's n_seg groups are a contiguous run of them): n_group of them, gk
 *   [n_group] their chunk, sg_ptr [n_slot + 1] / sg [n_group] each slot's groups in chunk order.
 *   T_slot = the canonical chunk tree over the slot's group partials (missing chunks 0).  All
 *   device, caller-owned.  n_slot = 0 turns it off.  Sharded (n_total > 0): SCHUR (after SETUP)
 *   writes the shard's group partials [n_seg][64] at its comm pointer (the caller passes comm +
 *   n_total·44·n_cam + g0·64, g0 = the shard's first group); one exchange of n_total·44·n_cam +
 *   n_group·64 doubles (zero-filled: an exact all-gather); SETUP_FINISH; then ITER / ITER_FINISH
 *   need no exchange (S is replicated). */
int sfm_ba_set_schur(sfm_ctx* ctx, int32_t n_slot, const int32_t* slot_cam, int32_t n_seg,
                     const int32_t* seg, int32_t n_inst, const int32_t* inst, const int32_t* row_ptr,
                     int32_t n_ent, const int32_t* row_ent, int32_t n_group, const int32_t* sg_ptr,
                     const int32_t* sg, const int32_t* gk);

/* ---- feature tracks ----------------------------------------------------------------------------
 * the verified match graph (sfm_graph_rows) -> tracks, the input of
 * triangulation and bundle adjustment.  Nodes are (image, keypoint), node = img_base[image] +
 * keypoint (img_base [n_img + 1] i32, exclusive scan of the keypoint counts); each graph row
 * (pair, queryIdx, trainIdx) joins node(pairs[pair][0], q) and node(pairs[pair][1], t).
 * A track is a connected component with >= min_len nodes and at most one node per image;
 * tracks are ordered by their smallest node id, nodes ascending within a track (deterministic).
 *   out (device): n_tracks [1], track_ptr [n_tracks + 1] (capacity n_nodes + 1),
 *                 track_img, track_kp [track_ptr[n_tracks]] (capacity n_nodes).
 * Synchronises the stream (the component rounds are host-driven). */
int sfm_tracks(sfm_ctx* ctx, int32_t n_img, const int32_t* img_base, int32_t n_pairs,
               const int32_t* pairs, int64_t n_rows, const int32_t* rows, int32_t min_len,
               int32_t* out_n_tracks, int32_t* out_track_ptr, int32_t* out_track_img,
               int32_t* out_track_kp);

/* ---- triangulation ---------------------------------------------------------------------------
 * the points of the tracks (sfm_tracks) from posed cameras, the start of
 * bundle adjustment.  Multi-view DLT on undistorted normalised coordinates (spec in
 * csrc/triangulate.hip; restated by oracle/recon.py).  Observations point-major: pt_ptr [n_pt+1]
 * CSR, cam_idx [n_obs] i32, uv [n_obs][2] f64; cams [n_cam][8], pp [n_cam][2] as sfm_ba_jtj.
 *   out (device): pts [n_pt][3] f64; stats [n_pt][4] f64 = {mean reprojection error (px), largest
 *   ray angle (deg), smallest depth, status: 0 ok, 1 < 2 views, 2 at infinity, 3 behind a camera}.
 */
int sfm_triangulate(sfm_ctx* ctx, int32_t n_cam, const double* cams, const double* pp,
                    int32_t n_pt, const int32_t* pt_ptr, const int32_t* cam_idx, const double* uv,
                    double* out_pts, double* out_stats);

/* Robust triangulation (papers/schoenberger2016sfm.pdf §4.2): RANSAC over the view
 * pairs of every track.  A pair's midpoint (ray angle above the gate, both ray parameters
 * positive) is scored by the observations that conform to it (positive depth, reprojection error
 * under the full camera model below thr); the consensus set of the winner is refitted by
 * sfm_triangulate's DLT.  fp64 in a fixed operation order: the spec is the header of
 * csrc/triangulate_robust.hip, tests/tri_ref.c restates it and the results equal it bit for bit.
 * Inputs as sfm_triangulate, plus pt_id [n_pt] i32: hypothesis h of a track depends only on
 * (seed, pt_id, h) and the track's own observations, never on the rest of the batch.
 *   out (device): pts [n_pt][3] f64; stats [n_pt][4] f64 = sfm_triangulate's, over the consensus
 *   set {mean reprojection error, largest ray angle (deg), smallest depth, status}; mask [n_obs]
 *   u8, 1 = the observation conforms to the returned point; info [n_pt][2] i32 = {consensus
 *   size, winning hypothesis}.  Status 0 ok, 1 fewer than 2 observations, 4 no admissible
 *   hypothesis; unless it is 0 the track's point, mask, stats[0..2] and info[0] are zero and
 *   info[1] is -1. */
typedef struct sfm_triangulate_robust_params {
    int32_t struct_size; /* sizeof(sfm_triangulate_robust_params) of the caller */
    int32_t max_hyp;     /* 1 .. 1024 view pairs per track (all pairs if there are no more) */
    double thr;          /* conformity threshold, pixels, > 0 */
    double max_cos2;     /* cos^2 of the smallest admissible ray angle, in (0, 1] */
    uint64_t seed;
} sfm_triangulate_robust_params;
int sfm_triangulate_robust(sfm_ctx* ctx, int32_t n_cam, const double* cams, const double* pp,
                           int32_t n_pt, const int32_t* pt_ptr, const int32_t* cam_idx,
                           const double* uv, const int32_t* pt_id,
                           const sfm_triangulate_robust_params* prm, double* out_pts,
                           double* out_stats, uint8_t* out_mask, int32_t* out_info);

/* Recursive robust triangulation (the paper's §4.2: "run the RANSAC again on the
 * measurements outside the consensus set"): a track that a wrong match merged out of several
 * scene points gives one point per consensus set.  Inputs as sfm_triangulate_robust, plus n_obs,
 * the length of cam_idx / uv / out_label (pt_ptr's values lie in 0 .. n_obs; it sizes the
 * workspace, so that no count comes back to the host).  Per track, rounds r = 0 .. max_points-1:
 * round r is sfm_triangulate_robust applied to the sub-track of the observations in no earlier
 * round's mask, in CSR order, with the same pt_id and the seed seed + r (uint64 wrap-around);
 * enumerated against sampled pairs, the refit, the re-score and the statistics all follow the
 * sub-track.  Round 0 is taken as it comes (status 0, 1 or 4); a round r >= 1 is accepted iff
 * its status is 0 and its consensus size is >= min_views; the first round not accepted ends the
 * track.  A track's result depends on (seed, pt_id, its own observations) only.
 *   out (device), R = max_points: pts [n_pt][R][3] f64, stats [n_pt][R][4] f64, info
 *   [n_pt][R][2] i32: slot r < n_points holds round r's sfm_triangulate_robust outputs (slot 0
 *   equals that call's, byte for byte); slot n_points is zero with info {0, -1} and the status
 *   of the ending round: 1, 4, or 5 = consensus below min_views; later slots are zero, {0, -1},
 *   status 5.  n_points [n_pt] i32: the accepted rounds (round 0 counts iff its status is 0).
 *   label [n_obs] i8: the accepted round whose mask holds the observation, -1 for none
 *   (observations outside every track's CSR range are not written).
 * Every round is enqueued by the one call; nothing is read back in between. */
typedef struct sfm_triangulate_multi_params {
    int32_t struct_size; /* sizeof(sfm_triangulate_multi_params) of the caller */
    int32_t max_points;  /* R: 1 .. 8 rounds per track */
    int32_t min_views;   /* >= 2: smallest consensus of an accepted round r >= 1 */
    int32_t max_hyp;     /* as sfm_triangulate_robust_params */
    double thr;
    double max_cos2;
    uint64_t seed;
} sfm_triangulate_multi_params;
int sfm_triangulate_multi(sfm_ctx* ctx, int32_t n_cam, const double* cams, const double* pp,
                          int32_t n_pt, const int32_t* pt_ptr, int32_t n_obs,
                          const int32_t* cam_idx, const double* uv, const int32_t* pt_id,
                          const sfm_triangulate_multi_params* prm, double* out_pts,
                          double* out_stats, int32_t* out_info, int32_t* out_n_points,
                          int8_t* out_label);

/* The per-camera table both triangulation calls start from (device, out_tab [n_cam][20] f64 =
 * R (9, row-major), t (3), centre -R^T t (3), f, k1, pp (2), 0): what the fixed-order spec of
 * sfm_triangulate_robust takes as its input. */
int sfm_triangulate_cam_table(sfm_ctx* ctx, int32_t n_cam, const double* cams, const double* pp,
                              double* out_tab);

/* ---- next-view registration ---------------------------------------------------------------
 * registers a batch of images against triangulated points (P3P RANSAC +
 * Gauss-Newton refinement; spec in oracle/sfm_oracle_reg.c / csrc/register.hip).  Per image i:
 * correspondences corr_ptr[i]..corr_ptr[i+1] of xy [n][2] f64 (pixels) and X [n][3] f64 (world),
 * intrinsics intr [n_img][4] = (f, k1, cx, cy), img_id [n_img] (keys the hypothesis RNG).
 * Hypothesis h of image i depends only on (seed, img_id[i], h): batch-composition invariant.
 *   out (device): cams [n_img][8] (angle-axis, t, f, k1; zeros on failure), count [n_img]
 *   (RANSAC inliers, -1 = no pose), key [n_img] (4 h + root of the winner, -1), mask [n] u8. */
typedef struct sfm_register_params {
    int32_t n_hyp;   /* multiple of 256 */
    int32_t refine;  /* 1: Gauss-Newton on the inliers (10 steps) */
    double thr;      /* inlier threshold, pixels */
    uint64_t seed;
} sfm_register_params;

int sfm_register_batch(sfm_ctx* ctx, int32_t n_img, const int32_t* corr_ptr, const double* xy,
                       const double* X, const double* intr, const int32_t* img_id,
                       const sfm_register_params* prm, double* out_cams, int32_t* out_count,
                       int32_t* out_key, uint8_t* out_mask);

/* ---- ORB feature extraction -------------------------------------------------------------------
 * replaces cv2.ORB_create() + orb.detectAndCompute(gray, None) of
 * code/feature_matching.py:42-45 (OpenCV defaults: 500 features, scale 1.2, 8 levels, edge 31,
 * patch 31, FAST 20, Harris score), batched over images of one size.  The spec is the build's
 * integer-exact restatement of the published algorithm (oracle/sfm_oracle_orb.c header; parity
 * against OpenCV itself unpinned: no cv2 here).
 *   images    [n_img][H][W] u8 (device)
 *   out_kp    [n_img][n_features][6] f32: x, y (level-0 pixels), size, angle (deg), Harris
 *             response, octave — level order, best Harris first within a level
 *   out_desc  [n_img][n_features][32] u8 (256-bit rBRIEF, OpenCV bit order)
 *   out_count [n_img] i32 keypoints found (<= n_features)
 */
typedef struct sfm_orb_params {
    int32_t n_features;      /* 500 */
    int32_t n_levels;        /* 8 (<= 16) */
    double scale_factor;     /* 1.2 */
    int32_t fast_threshold;  /* 20 */
    int32_t _pad;
} sfm_orb_params;

int sfm_orb_batch(sfm_ctx* ctx, const uint8_t* images, int32_t n_img, int32_t H, int32_t W,
                  const sfm_orb_params* prm, float* out_kp, uint8_t* out_desc,
                  int32_t* out_count);

/* ---- image retrieval: vocabulary words, term frequencies, nearest images -------
 * Pair selection for collections where most image pairs share nothing.  Word assignment exists
 * for L2 / 128-byte descriptors (sfm_vocab_assign) and for binary / 32-byte descriptors
 * (sfm_vocab_assign_hamming, with sfm_vocab_majority to refine the vocabulary); the stages after it
 * work on word ids.  Everything is integer and exact: the outputs are a function of the inputs
 * alone.
 *
 * sfm_vocab_assign: the nearest vocabulary word of every descriptor by exact squared L2, the
 * lowest word index among equal distances (i8 MFMA, the same contraction as sfm_match_batch).
 *   desc      [n_img][k_max][128] u8 and n_kp [n_img] as for sfm_match_batch, k_max <= 8192
 *   vocab     [n_words][128] u8, 1 <= n_words <= 65536
 *   out_word  [n_img][k_max] i32: the word; -1 from n_kp[i] on
 *   out_dist  [n_img][k_max] i32 or NULL: that d^2; 0 where the word is -1
 *
 * sfm_vocab_assign_hamming: the same for 256-bit descriptors under Hamming distance (bits expanded
 * to i8 on the MFMA).  Distances take 257 values, so ties are common: the lowest word index wins
 * among equal distances, whatever the vocabulary size.
 *   desc      [n_img][k_max][32] u8, 16-byte aligned; n_kp [n_img]; k_max <= 8192
 *   vocab     [n_words][32] u8, 16-byte aligned, 1 <= n_words <= 65536
 *   out_word  [n_img][k_max] i32: the word; -1 from n_kp[i] on
 *   out_dist  [n_img][k_max] i32 or NULL: that distance in bits (0 .. 256); 0 where the word is -1
 *
 * sfm_vocab_majority: one k-majority round, out of place.  The members of word j are the rows
 * q < n_kp[i] with word[i][q] == j (entries outside [0, n_words), -1 among them, are skipped).
 * With cnt members of which ones[b] have bit b set (bit b = bit b % 8 of byte b / 8), bit b of
 * out_vocab[j] is 1 if 2 ones[b] > cnt, bit b of vocab[j] if 2 ones[b] == cnt, else 0; a word
 * without members keeps its bytes.  Integer counters in the context's workspace (n_words * 257
 * u32, at most 64.25 MB); the result does not depend on block or atomic order.  1 <= n_words <=
 * 65536, n_img * k_max < 2^32.  These two entry points are additive: sfm_version is unchanged.
 *
 * sfm_bow_hist: out_hist [n_img][n_words] u16 term frequencies of word [n_img][k_max] (entries
 * outside [0, n_words), -1 among them, and entries from n_kp[i] on are skipped).  The whole array
 * is written.  n_words <= 65536, k_max <= 65535, n_img <= 65535.
 *
 * sfm_bow_neighbours: score(a, b) = sum_w min(hist[a][w], hist[b][w]) * weight[w] in exact int64,
 * weight [n_words] i32 in [0, 65535] (the caller validates the range).  For every image a the
 * up-to-k images b != a with the largest positive score, in descending score order, lower b first
 * among equal scores: out_nbr [n_img][k] i32 padded with -1, out_score [n_img][k] i64 padded with
 * 0.  k >= 1; k >= n_img just pads.  Uses a dense [n_img][n_img] i64 score matrix in the
 * context's workspace. */
int sfm_vocab_assign(sfm_ctx* ctx, const uint8_t* desc, const int32_t* n_kp, int32_t n_img,
                     int32_t k_max, const uint8_t* vocab, int32_t n_words, int32_t* out_word,
                     int32_t* out_dist);
int sfm_vocab_assign_hamming(sfm_ctx* ctx, const uint8_t* desc, const int32_t* n_kp, int32_t n_img,
                             int32_t k_max, const uint8_t* vocab, int32_t n_words,
                             int32_t* out_word, int32_t* out_dist);
int sfm_vocab_majority(sfm_ctx* ctx, const uint8_t* desc, const int32_t* n_kp, int32_t n_img,
                       int32_t k_max, const int32_t* word, const uint8_t* vocab, int32_t n_words,
                       uint8_t* out_vocab);
int sfm_bow_hist(sfm_ctx* ctx, const int32_t* word, const int32_t* n_kp, int32_t n_img,
                 int32_t k_max, int32_t n_words, uint16_t* out_hist);
int sfm_bow_neighbours(sfm_ctx* ctx, const uint16_t* hist, int32_t n_img, int32_t n_words,
                       const int32_t* weight, int32_t k, int32_t* out_nbr, int64_t* out_score);

/* ---- measurement: the device's i8 matrix ceiling right now ------------------------------------
 * Not a reference interface: the bench line's calibration probe (bench.py "calib"), so that K1's
 * roofline fraction can be read against the ceiling of the box it ran on.  Every CU runs MFMA-only
 * waves (v_mfma_i32_32x32x32_i8, register operands, random data, 2 waves per SIMD) for about
 * target_ms (0 < target_ms <= 5000).  out[4]: wall ms of the measured launch, i8 TOP/s, median
 * in-kernel clock (GHz), fraction of the nominal dense-i8 peak.  Synchronises the stream. */
int sfm_calib_mfma_i8(sfm_ctx* ctx, float target_ms, double* out);

/* ---- measurement: the mutual certificate of the L2 ratio path -----------------------------------
 * Counters of sfm_match_batch's L2 mutual + ratio rule on the forward-scan path (DESIGN.md §4.1
 * "certificate"), default off.  enable != 0: every later such call on ctx first clears, then
 * fills three device counters (a few atomics per pair).  out != NULL: synchronises the stream and
 * writes the LAST call's (pairs the certificate decided, pairs it flagged for the reverse scan,
 * exact dot products it took).  Off: the kernels take no counter pointer at all. */
int sfm_match_cert_stats(sfm_ctx* ctx, int32_t enable, uint64_t* out);

/* The grid bound of that path's fallback (reverse scan and final kernel): their blocks stride over
 * the (query block, flagged pair) units, so a call that flags more units than this runs the stride
 * loop more than once. */
int32_t sfm_l2fr_rev_grid(void);

#ifdef __cplusplus
}
#endif
#endif /* SFMCORE_H */
