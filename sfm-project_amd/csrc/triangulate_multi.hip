// Recursive robust triangulation (papers/schoenberger2016sfm.pdf §4.2: "run the
// RANSAC again on the measurements outside the consensus set"): a track that a wrong match merged
// out of several scene points gives one point per consensus set.
//
// Spec.  Per track, rounds r = 0 .. R-1 (R = max_points).  Round r is sfm_triangulate_robust
// (the header of triangulate_robust.hip) applied to the sub-track of the observations that are in
// no earlier round's mask, in CSR order, with the track's pt_id and the seed seed + r (uint64
// wrap-around); whether the pairs are enumerated or sampled follows from the sub-track's own
// length.  Round 0 is taken as it comes (status 0, 1 or 4); a round r >= 1 is accepted iff its
// status is 0 and its consensus size is >= min_views; the first round that is not accepted ends
// the track.  n_points counts the accepted rounds (round 0 iff its status is 0).  Slot r <
// n_points holds round r's outputs; slot n_points is zero with info {0, -1} and the status of the
// ending round (1, 4, or 5 for a consensus below min_views); later slots are zero, {0, -1},
// status 5.  label[o] is the accepted round whose mask holds observation o, -1 for none.
//
// Kernels.  One call enqueues every round; nothing comes back to the host in between.  A round
// is the kernels of tri_robust_kernels.h on a sub-problem (CSR, cam_idx, uv, pt_id of its own)
// into contiguous per-sub-track results, then tri_multi_scatter, a thread per sub-track:
//   - writes slot r, the labels (through the sub-problem's map back to the caller's observation
//     index) and n_points; round 0 also fills the slots after it with their defaults;
//   - decides whether the track goes on: accepted, r + 1 < R and >= 2 observations left (with
//     fewer the next round is status 1, written here);
//   - builds the next round's sub-problem from the tracks that go on: the block scans (tracks,
//     observations left) as one packed 64-bit pair, takes its range of both with one atomic on
//     the packed device counter (so track slots and observation offsets stay in step: the end of
//     a sub-track is the start of the next), and each thread gathers its track's remaining
//     cam_idx / uv / map.
// Round 0 runs on the caller's arrays.  Rounds >= 1 run grids sized for n_pt whose blocks read the
// device-side track count and return: on a clean problem they are near-empty launches, and their
// work follows the tracks that reach them.  The order of the sub-tracks depends on the atomics;
// no result does (a track's result depends on seed, pt_id and its own observations only).
#include "tri_robust_kernels.h"

using namespace tri_robust;

namespace {

struct SubProblem {
    int32_t* ptr;     // [n + 1]
    int32_t* cam;     // [n_obs]
    double* uv;       // [n_obs][2]
    int32_t* id;      // [n] pt_id of the track
    int32_t* track;   // [n] the caller's track
    int32_t* map;     // [n_obs] the caller's observation
};

template <bool FIRST>
__global__ __launch_bounds__(256) void tri_multi_scatter(
    int n_pt, const int32_t* __restrict__ n_live, int r, int R, int min_views,
    const int32_t* __restrict__ ptr, const int32_t* __restrict__ cam,
    const double* __restrict__ uv, const int32_t* __restrict__ id,
    const int32_t* __restrict__ track, const int32_t* __restrict__ map,
    const double* __restrict__ s_pts, const double* __restrict__ s_stats,
    const uint8_t* __restrict__ s_mask, const int32_t* __restrict__ s_info,
    unsigned long long* __restrict__ next_ctr, SubProblem nx, double* __restrict__ out_pts,
    double* __restrict__ out_stats, int32_t* __restrict__ out_info,
    int32_t* __restrict__ out_n_points, int8_t* __restrict__ out_label) {
    __shared__ unsigned long long wave_tot[4], base;   // (tracks << 32) | observations
    const int n_sub = FIRST ? n_pt : *n_live;
    if ((int)(blockIdx.x * blockDim.x) >= n_sub) return;   // the whole block
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int p = 0, o0 = 0, n = 0, cnt = 0;
    bool go = false;
    if (s < n_sub) {
        p = FIRST ? s : track[s];
        o0 = ptr[s];
        n = ptr[s + 1] - o0;
        const int status = (int)s_stats[4 * (size_t)s + 3];
        cnt = s_info[2 * (size_t)s];
        const bool acc = status == 0 && (FIRST || cnt >= min_views);
        const size_t slot = (size_t)p * R + r;
        if (FIRST || acc) {
#pragma unroll
            for (int m = 0; m < 3; ++m) out_pts[3 * slot + m] = s_pts[3 * (size_t)s + m];
#pragma unroll
            for (int m = 0; m < 4; ++m) out_stats[4 * slot + m] = s_stats[4 * (size_t)s + m];
            out_info[2 * slot] = cnt;
            out_info[2 * slot + 1] = s_info[2 * (size_t)s + 1];
        } else {
            out_stats[4 * slot + 3] = status != 0 ? (double)status : 5.0;
        }
        if (FIRST) {
            for (int q = 1; q < R; ++q) {
                const size_t sq = slot + q;
                out_pts[3 * sq] = 0.0; out_pts[3 * sq + 1] = 0.0; out_pts[3 * sq + 2] = 0.0;
                out_stats[4 * sq] = 0.0; out_stats[4 * sq + 1] = 0.0; out_stats[4 * sq + 2] = 0.0;
                out_stats[4 * sq + 3] = 5.0;
                out_info[2 * sq] = 0;
                out_info[2 * sq + 1] = -1;
            }
            out_n_points[p] = acc ? 1 : 0;
            for (int k = 0; k < n; ++k) out_label[(size_t)o0 + k] = s_mask[(size_t)o0 + k] ? 0 : -1;
        } else if (acc) {
            out_n_points[p] = r + 1;
            for (int k = 0; k < n; ++k)
                if (s_mask[(size_t)o0 + k]) out_label[map[(size_t)o0 + k]] = (int8_t)r;
        }
        if (acc && r + 1 < R) {
            if (n - cnt >= 2) go = true;
            else out_stats[4 * (slot + 1) + 3] = 1.0;
        }
    }
    if (next_ctr == nullptr) return;   // the last round: nothing follows

    // ---- the next round's sub-problem: block scan of (1, observations left), one atomic
    const unsigned long long v = go ? ((1ull << 32) | (unsigned long long)(uint32_t)(n - cnt)) : 0ull;
    unsigned long long inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long t = __shfl_up(inc, off, 64);
        if (lane >= off) inc += t;
    }
    if (lane == 63) wave_tot[wave] = inc;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long tot = wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3];
        base = tot ? atomicAdd(next_ctr, tot) : 0ull;
        if (blockIdx.x == 0) nx.ptr[0] = 0;
    }
    __syncthreads();
    if (!go) return;
    unsigned long long e = base + (inc - v);
    for (int w = 0; w < wave; ++w) e += wave_tot[w];
    const int sn = (int)(e >> 32);
    int w = (int)(uint32_t)e;
    nx.track[sn] = p;
    nx.id[sn] = id[s];
    const int w_end = w + (n - cnt);
    nx.ptr[sn + 1] = w_end;
    for (int k = 0; k < n && w < w_end; ++k) {
        const size_t o = (size_t)o0 + k;
        if (s_mask[o]) continue;
        nx.cam[w] = cam[o];
        nx.uv[2 * (size_t)w] = uv[2 * o];
        nx.uv[2 * (size_t)w + 1] = uv[2 * o + 1];
        nx.map[w] = FIRST ? (int32_t)o : map[o];
        ++w;
    }
}

}  // namespace

extern "C" int sfm_triangulate_multi(sfm_ctx* ctx, int32_t n_cam, const double* cams,
                                     const double* pp, int32_t n_pt, const int32_t* pt_ptr,
                                     int32_t n_obs, const int32_t* cam_idx, const double* uv,
                                     const int32_t* pt_id, const sfm_triangulate_multi_params* prm,
                                     double* out_pts, double* out_stats, int32_t* out_info,
                                     int32_t* out_n_points, int8_t* out_label) {
    SFM_REQUIRE(ctx && prm, "sfm_triangulate_multi: ctx/prm is NULL");
    SFM_REQUIRE(prm->struct_size >= (int32_t)sizeof(sfm_triangulate_multi_params),
                "sfm_triangulate_multi: prm->struct_size is smaller than the struct");
    SFM_REQUIRE(n_cam >= 0 && n_pt >= 0 && n_obs >= 0, "sfm_triangulate_multi: negative size");
    SFM_REQUIRE(prm->max_points >= 1 && prm->max_points <= 8,
                "sfm_triangulate_multi: max_points must lie in 1 .. 8");
    SFM_REQUIRE(prm->min_views >= 2, "sfm_triangulate_multi: min_views must be >= 2");
    SFM_REQUIRE(prm->max_hyp >= 1 && prm->max_hyp <= 1024,
                "sfm_triangulate_multi: max_hyp must lie in 1 .. 1024");
    SFM_REQUIRE(prm->thr > 0.0 && prm->thr < 1e150, "sfm_triangulate_multi: thr must be > 0");
    SFM_REQUIRE(prm->max_cos2 > 0.0 && prm->max_cos2 <= 1.0,
                "sfm_triangulate_multi: max_cos2 must lie in (0, 1]");
    if (n_pt == 0) return SFM_OK;
    SFM_REQUIRE(cams && pp && pt_ptr && pt_id && out_pts && out_stats && out_info &&
                    out_n_points && (n_obs == 0 || (cam_idx && uv && out_label)),
                "sfm_triangulate_multi: NULL array");
    SFM_REQUIRE(n_cam > 0, "sfm_triangulate_multi: no cameras");
    SFM_HIP_CHECK(hipSetDevice(ctx->device));
    const int R = prm->max_points;
    // workspace: camera table | bin counts and sub-problem counters of every round (zeroed) |
    // bin lists | a round's results | two sub-problems (a round reads one and fills the other)
    const size_t A = 256;
    const size_t tab_bytes = sfm::align_up(sizeof(double) * CAMW * (size_t)n_cam, A);
    const size_t ctl_bytes = A * (size_t)(R + 1);
    const size_t list_bytes = sfm::align_up(sizeof(int32_t) * N_BIN * (size_t)n_pt, A);
    const size_t rp_bytes = sfm::align_up(sizeof(double) * 3 * (size_t)n_pt, A);
    const size_t rs_bytes = sfm::align_up(sizeof(double) * 4 * (size_t)n_pt, A);
    const size_t ri_bytes = sfm::align_up(sizeof(int32_t) * 2 * (size_t)n_pt, A);
    const size_t rm_bytes = sfm::align_up((size_t)n_obs + 1, A);
    const size_t t_bytes = sfm::align_up(sizeof(int32_t) * ((size_t)n_pt + 1), A);
    const size_t o_bytes = sfm::align_up(sizeof(int32_t) * ((size_t)n_obs + 1), A);
    const size_t sub_bytes = R > 1 ? 3 * t_bytes + 2 * o_bytes + 4 * o_bytes : 0;
    char* ws = (char*)sfm::workspace(ctx, tab_bytes + ctl_bytes + list_bytes + rp_bytes + rs_bytes +
                                              ri_bytes + rm_bytes + 2 * sub_bytes);
    if (!ws) return SFM_ERR_NOMEM;
    char* q = ws;
    auto take = [&](size_t bytes) { char* at = q; q += bytes; return at; };
    double* tab = (double*)take(tab_bytes);
    char* ctl = take(ctl_bytes);
    int32_t* lists = (int32_t*)take(list_bytes);
    double* s_pts = (double*)take(rp_bytes);
    double* s_stats = (double*)take(rs_bytes);
    int32_t* s_info = (int32_t*)take(ri_bytes);
    uint8_t* s_mask = (uint8_t*)take(rm_bytes);
    SubProblem sub[2] = {};
    for (int b = 0; b < 2 && R > 1; ++b) {
        sub[b].uv = (double*)take(4 * o_bytes);
        sub[b].ptr = (int32_t*)take(t_bytes);
        sub[b].id = (int32_t*)take(t_bytes);
        sub[b].track = (int32_t*)take(t_bytes);
        sub[b].cam = (int32_t*)take(o_bytes);
        sub[b].map = (int32_t*)take(o_bytes);
    }
    unsigned long long* ctr = (unsigned long long*)(ctl + A * (size_t)R);   // [R], entry 0 unused
    hipStream_t st = ctx->stream;
    SFM_HIP_CHECK(hipMemsetAsync(ctl, 0, ctl_bytes, st));
    hipLaunchKernelGGL(tri_cam_setup, dim3((n_cam + 255) / 256), dim3(256), 0, st, n_cam, cams, pp,
                       tab);
    const double thr2 = prm->thr * prm->thr;
    const dim3 grid((n_pt + 255) / 256), block(256);
    for (int r = 0; r < R; ++r) {
        const SubProblem& c = sub[r & 1];
        const int32_t* c_ptr = r ? c.ptr : pt_ptr;
        const int32_t* c_cam = r ? c.cam : cam_idx;
        const double* c_uv = r ? c.uv : uv;
        const int32_t* c_id = r ? c.id : pt_id;
        // the tracks of round r: the high word of its packed counter
        const int32_t* n_live = r ? (const int32_t*)(ctr + r) + 1 : nullptr;
        enqueue(ctx, n_pt, n_live, (int32_t*)(ctl + A * (size_t)r), lists, c_ptr, c_cam, c_uv, c_id,
                tab, thr2, prm->max_cos2, prm->max_hyp, (uint64_t)prm->seed + (uint64_t)r, s_pts,
                s_stats, s_mask, s_info);
        unsigned long long* next_ctr = r + 1 < R ? ctr + r + 1 : nullptr;
        const SubProblem nx = r + 1 < R ? sub[(r + 1) & 1] : SubProblem{};
        if (r == 0)
            hipLaunchKernelGGL(tri_multi_scatter<true>, grid, block, 0, st, n_pt, n_live, r, R,
                               prm->min_views, c_ptr, c_cam, c_uv, c_id, nullptr, nullptr, s_pts,
                               s_stats, s_mask, s_info, next_ctr, nx, out_pts, out_stats, out_info,
                               out_n_points, out_label);
        else
            hipLaunchKernelGGL(tri_multi_scatter<false>, grid, block, 0, st, n_pt, n_live, r, R,
                               prm->min_views, c_ptr, c_cam, c_uv, c_id, c.track, c.map, s_pts,
                               s_stats, s_mask, s_info, next_ctr, nx, out_pts, out_stats, out_info,
                               out_n_points, out_label);
    }
    SFM_HIP_CHECK(hipGetLastError());
    return SFM_OK;
}
