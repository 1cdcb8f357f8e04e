// Robust multi-view triangulation (papers/schoenberger2016sfm.pdf §4.2): RANSAC
// over the view pairs of a track, consensus by reprojection, refit of the consensus set by
// sfm_triangulate's DLT.  Restated on the CPU by tests/tri_ref.c, which the GPU tests match bit for
// bit (stats[1], the one acos, to 1e-9 degrees).
//
// Spec.  fp64, the operations in the order written, no FMA contraction; sums and dot products run
// left to right.  Input is the per-camera table of tri_common.h (R, t, C = -Rᵀ t, f, k1, pp): the
// spec starts there (sfm_triangulate_cam_table returns the table a call uses).  Per track with
// the n observations k = 0 .. n-1 of its CSR range, camera c_k, pixel (u_k, v_k):
//   1 views      x_k = sfm_triangulate's undistorted coordinates (10 fixed-point steps);
//                d_k[m] = R[m] x_k0 + R[3+m] x_k1 + R[6+m]  (world ray Rᵀ (x, 1)), C_k the centre.
//   2 hypotheses view pairs (i < j).  n (n-1) / 2 <= max_hyp: all of them, h counting them in
//                lexicographic order.  Otherwise h = 0 .. max_hyp-1 with
//                r = Philox4x32-10(counter (h, 3, pt_id, 0x54524931), key (seed lo, seed hi)),
//                a = mulhi32(r0, n), b = mulhi32(r1, n-1), b += 1 if b >= a, (i, j) = (min, max).
//   3 two-view   a = d_i, b = d_j, w = C_j - C_i, c = a.b, aa = a.a, bb = b.b; the pair is rejected
//                unless c > 0 and c c < max_cos2 (aa bb).  aw = a.w, bw = b.w, det = aa bb - c c,
//                s = (bb aw - c bw) / det, t = (c aw - aa bw) / det; rejected unless s > 0 and
//                t > 0.  X[m] = 0.5 ((C_i[m] + s a[m]) + (C_j[m] + t b[m])).
//   4 score      P = R X + t (rows left to right, then + t); q = (P0, P1) / P2;
//                g = 1 + k1 (q0 q0 + q1 q1); e0 = f g q0 + pp0 - u, e1 = f g q1 + pp1 - v;
//                e2 = e0 e0 + e1 e1; k conforms iff P2 > 0 and e2 < thr2 (thr2 = thr thr, formed
//                once on the host).  count = conforming observations; the winner is the largest
//                count, the lowest h among equals; a count below 2 cannot win (status 4 if none).
//   5 refit      M = Σ rowsᵀ rows over the winner's conforming observations in CSR order, rows,
//                jacobi4, smallest diagonal and the |w| > 1e-12 |xyz| test as in sfm_triangulate.
//                All n observations are scored again under the refitted point; it is kept iff
//                the |w| test passed and its count >= the winner's, else the two-view point stays.
//   6 stats      over the observations conforming to the kept point (the mask), CSR order:
//                {Σ sqrt(e2) / count, acos(clamp(min over pairs of a.b / (|a| |b|))) in degrees
//                with a = X - C (min starts at 1), min P2 (starts at 1e300), 0};
//                info = {count, winning h}.
//
// Kernels (in tri_robust_kernels.h, which triangulate_multi.hip shares).  tri_bin (thread per
// track) writes the status-1 tracks and appends every other track to one of four lists: by its hypothesis count (<= 8, <= 16, <= 32, more), and to the last one
// whenever it has more than 16 observations.  tri_robust_kernel<G, CAP, FUSED> takes one list:
// single-wave blocks, a group of G = 8 / 16 / 32 / 64 lanes per track (64 / G tracks per wave), a
// lane per hypothesis, passes of 64 hypotheses in the last list.  The group builds the track's
// view records (26 doubles) once in LDS; in every walk all lanes of a group read the same record
// (an LDS broadcast).  Observations beyond CAP are rebuilt from the camera table in global memory
// (wave-uniform rows).  Winner: group max of (count << 32) | ~h.
// Long tracks (the last list, FUSED): the wave goes on.  What is per observation (conformity, its
// error and depth under a point) is computed a lane per observation and left in the record; what
// has an order is then summed from those values by every lane in CSR order.  Refit: lane e sums
// entry e of M (the additions of the thread-per-point kernel), the 16 entries are exchanged by
// shuffles and every lane runs the same jacobi4.  Order-free reductions (the ray-angle minimum)
// are split across the wave.
// Short tracks: the group stops at the winner and tri_finish_kernel refits a thread per track,
// as sfm_triangulate does: the Jacobi chain is serial, and a group would repeat it on every one
// of its lanes (measured: 100 k x 5 views 1.72 ms fused).
#include "tri_robust_kernels.h"

using namespace tri_robust;

extern "C" int sfm_triangulate_cam_table(sfm_ctx* ctx, int32_t n_cam, const double* cams,
                                         const double* pp, double* out_tab) {
    SFM_REQUIRE(ctx != nullptr, "sfm_triangulate_cam_table: ctx is NULL");
    SFM_REQUIRE(n_cam >= 0, "sfm_triangulate_cam_table: negative size");
    if (n_cam == 0) return SFM_OK;
    SFM_REQUIRE(cams && pp && out_tab, "sfm_triangulate_cam_table: NULL array");
    SFM_HIP_CHECK(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(tri_cam_setup, dim3((n_cam + 255) / 256), dim3(256), 0, ctx->stream, n_cam,
                       cams, pp, out_tab);
    SFM_HIP_CHECK(hipGetLastError());
    return SFM_OK;
}

extern "C" int sfm_triangulate_robust(sfm_ctx* ctx, int32_t n_cam, const double* cams,
                                      const double* pp, int32_t n_pt, const int32_t* pt_ptr,
                                      const int32_t* cam_idx, const double* uv,
                                      const int32_t* pt_id,
                                      const sfm_triangulate_robust_params* prm, double* out_pts,
                                      double* out_stats, uint8_t* out_mask, int32_t* out_info) {
    SFM_REQUIRE(ctx && prm, "sfm_triangulate_robust: ctx/prm is NULL");
    SFM_REQUIRE(prm->struct_size >= (int32_t)sizeof(sfm_triangulate_robust_params),
                "sfm_triangulate_robust: prm->struct_size is smaller than the struct");
    SFM_REQUIRE(n_cam >= 0 && n_pt >= 0, "sfm_triangulate_robust: negative size");
    SFM_REQUIRE(prm->max_hyp >= 1 && prm->max_hyp <= 1024,
                "sfm_triangulate_robust: max_hyp must lie in 1 .. 1024");
    SFM_REQUIRE(prm->thr > 0.0 && prm->thr < 1e150, "sfm_triangulate_robust: thr must be > 0");
    SFM_REQUIRE(prm->max_cos2 > 0.0 && prm->max_cos2 <= 1.0,
                "sfm_triangulate_robust: max_cos2 must lie in (0, 1]");
    if (n_pt == 0) return SFM_OK;
    SFM_REQUIRE(cams && pp && pt_ptr && cam_idx && uv && pt_id && out_pts && out_stats &&
                    out_mask && out_info,
                "sfm_triangulate_robust: NULL array");
    SFM_REQUIRE(n_cam > 0, "sfm_triangulate_robust: no cameras");
    SFM_HIP_CHECK(hipSetDevice(ctx->device));
    // workspace: camera table | bin counts | bin lists
    const size_t tab_bytes = sfm::align_up(sizeof(double) * CAMW * (size_t)n_cam, 256);
    const size_t cnt_bytes = 256;
    const size_t list_bytes = sizeof(int32_t) * N_BIN * (size_t)n_pt;
    char* ws = (char*)sfm::workspace(ctx, tab_bytes + cnt_bytes + list_bytes);
    if (!ws) return SFM_ERR_NOMEM;
    double* tab = (double*)ws;
    int32_t* counts = (int32_t*)(ws + tab_bytes);
    int32_t* lists = (int32_t*)(ws + tab_bytes + cnt_bytes);
    hipStream_t st = ctx->stream;
    SFM_HIP_CHECK(hipMemsetAsync(counts, 0, cnt_bytes, st));
    hipLaunchKernelGGL(tri_cam_setup, dim3((n_cam + 255) / 256), dim3(256), 0, st, n_cam, cams, pp,
                       tab);
    enqueue(ctx, n_pt, nullptr, counts, lists, pt_ptr, cam_idx, uv, pt_id, tab,
            prm->thr * prm->thr, prm->max_cos2, prm->max_hyp, (uint64_t)prm->seed, out_pts,
            out_stats, out_mask, out_info);
    SFM_HIP_CHECK(hipGetLastError());
    return SFM_OK;
}
