// btba_api_corres.hip -- host side of libbtba.so: correspondence RANSAC, descriptor matching, window assembly, map points and findCorres.
#include "btba_host_common.hpp"
#include "btba_ransac.hpp"
#include "btba_xorwow.hpp"
#include "btba_match.hpp"
#include "btba_mappoints.hpp"
#include "btba_window.hpp"

extern "C" {

// ---- correspondence RANSAC ---------------------------------------------------------
// the reference's per-trial cuRAND streams = one table of uniforms for all pairs; rebuilt only when the seed changes or
// more trials are asked for than the table holds (a longer table for the same seed starts with the shorter one)
static int ransac_uniform_table(btba_workspace *ws, uint64_t seed, int n_trials)
{
    if (ws->ransac_u_host.size() >= 3 * (size_t)n_trials && ws->ransac_u_seed == seed) return BTBA_OK;
    HIP_TRY(hipStreamSynchronize(ws->stream));      // an earlier call's kernels / upload may still be using the old table
    ws->ransac_u_host.assign(3 * (size_t)n_trials, 0.0f);
    xorwow::ransac_uniform_table(seed, n_trials, ws->ransac_u_host.data());
    ws->ransac_u_seed = seed;
    int rc;
    if ((rc = ws->ransac_u.ensure(12 * (size_t)n_trials))) return rc;
    HIP_TRY(hipMemcpyAsync(ws->ransac_u.p, ws->ransac_u_host.data(), 12 * (size_t)n_trials, hipMemcpyHostToDevice, ws->stream));
    return BTBA_OK;
}

// vote + extraction for D.n_pairs pairs whose point counts are on the DEVICE (offsets[p] .. offsets[p + 1]); `best` zeroed by the caller.
// Asynchronous on the workspace stream: btba_ransac_pairs_ex and btba_corres_chain (one pair per call, its count written by an earlier kernel).
static int ransac_enqueue(btba_workspace *ws, const RansacDims &D, const float4 *dA, const float4 *dB, const int *d_offsets, const int *dS, float *d_pose,
                          int *d_cnt, unsigned long long *d_best, int *d_ids, int *d_nin, int *d_bt, float *d_bp)
{
    k_ransac_vote<<<dim3((D.n_trials + 255) / 256, D.n_pairs), 256, 0, ws->stream>>>(D, dA, dB, d_offsets, dS, ws->ransac_u.as<float>(), d_pose, d_cnt, d_best);
    k_ransac_extract<<<D.n_pairs, 256, 0, ws->stream>>>(D, dA, dB, d_offsets, d_pose, d_best, d_ids, d_nin, d_bt, d_bp);
    HIP_TRY(hipGetLastError());
    return BTBA_OK;
}

int btba_ransac_pairs_ex(btba_workspace *ws, int hypothesis, int device_resident, int n_pairs, const float *ptsA, const float *ptsB, const int32_t *n_pts,
                         int n_trials, float dist_thres, const int32_t *samples, uint64_t seed,
                         int32_t *inlier_ids_out, int32_t *n_inliers_out, int32_t *best_trial_out, float *best_pose_out,
                         int32_t *trial_counts_out, float *trial_poses_out)
{
    DeviceGuard device_guard(ws);
    if (!ws || n_pairs < 1 || !n_pts || n_trials < 1 || !(dist_thres >= 0.0f) || !inlier_ids_out || !n_inliers_out) return BTBA_EINVAL;
    const bool draw_hash = (hypothesis & BTBA_RANSAC_DRAW_HASH) != 0;
    hypothesis &= ~BTBA_RANSAC_DRAW_HASH;
    if (hypothesis != BTBA_RANSAC_REFERENCE_SVD && hypothesis != BTBA_RANSAC_HORN) return BTBA_EINVAL;
    std::vector<int32_t> offsets(n_pairs + 1, 0);
    for (int p = 0; p < n_pairs; p++) {
        if (n_pts[p] < 0) return BTBA_EINVAL;
        offsets[p + 1] = offsets[p] + n_pts[p];
    }
    const size_t T = (size_t)offsets[n_pairs], NT = (size_t)n_pairs * n_trials;
    if (T && (!ptsA || !ptsB)) return BTBA_EINVAL;
    const bool dev = device_resident != 0;
    Scratch S;
    const auto s_a = S.add<float4>(T ? T : 1, !dev), s_b = S.add<float4>(T ? T : 1, !dev);
    const auto s_off = S.add<int>((size_t)n_pairs + 1);
    const auto s_smp = S.add<int>((samples && !dev) ? 3 * NT : 1);      // (absent: one word)
    const auto s_pose = S.add<float>(12 * NT);
    const auto s_cnt = S.add<int>(NT);
    const auto s_best = S.add<unsigned long long>((size_t)n_pairs);
    const auto s_ids = S.add<int>(T ? T : 1, !dev);
    const auto s_nin = S.add<int>((size_t)n_pairs), s_bt = S.add<int>((size_t)n_pairs);
    const auto s_bp = S.add<float>(16 * (size_t)n_pairs);
    int rc;
    if ((rc = S.bind(ws->ransac, 256))) return rc;
    if (T && !dev) {
        HIP_TRY(hipMemcpyAsync(s_a, ptsA, 16 * T, hipMemcpyHostToDevice, ws->stream));
        HIP_TRY(hipMemcpyAsync(s_b, ptsB, 16 * T, hipMemcpyHostToDevice, ws->stream));
    }
    HIP_TRY(hipMemcpyAsync(s_off, offsets.data(), 4 * (size_t)(n_pairs + 1), hipMemcpyHostToDevice, ws->stream));
    HIP_TRY(hipStreamSynchronize(ws->stream));          // `offsets` is a local (16 B per pair: the only host wait of the device-resident form)
    if (samples && !dev) HIP_TRY(hipMemcpyAsync(s_smp, samples, 12 * NT, hipMemcpyHostToDevice, ws->stream));
    HIP_TRY(hipMemsetAsync(s_best, 0, 8 * (size_t)n_pairs, ws->stream));
    if (!samples && !draw_hash && (rc = ransac_uniform_table(ws, seed, n_trials))) return rc;
    RansacDims D{};
    D.n_pairs = n_pairs; D.n_trials = n_trials; D.dist_thres = dist_thres; D.seed = seed; D.hypothesis = hypothesis;
    D.draw = samples ? 1 : (draw_hash ? 0 : 2);
    const float4 *dA = dev ? reinterpret_cast<const float4 *>(ptsA) : s_a;
    const float4 *dB = dev ? reinterpret_cast<const float4 *>(ptsB) : s_b;
    const int *dS = (samples && dev) ? samples : s_smp;
    // device-resident: results go straight to the caller's device buffers (the optional per-trial tables too)
    int *d_ids = dev ? inlier_ids_out : s_ids;
    int *d_nin = dev ? n_inliers_out : s_nin;
    int *d_bt = (dev && best_trial_out) ? best_trial_out : s_bt;
    float *d_bp = (dev && best_pose_out) ? best_pose_out : s_bp;
    int *d_cnt = (dev && trial_counts_out) ? trial_counts_out : s_cnt;
    float *d_pose = (dev && trial_poses_out) ? trial_poses_out : s_pose;
    if ((rc = ransac_enqueue(ws, D, dA, dB, s_off, dS, d_pose, d_cnt, s_best, d_ids, d_nin, d_bt, d_bp))) return rc;
    if (dev) return BTBA_OK;                          // asynchronous on the workspace stream
    // the inlier lists are written only up to each pair's count: fetch counts first, ids after
    HIP_TRY(hipMemcpyAsync(n_inliers_out, d_nin, 4 * (size_t)n_pairs, hipMemcpyDeviceToHost, ws->stream));
    if (T) HIP_TRY(hipMemcpyAsync(inlier_ids_out, d_ids, 4 * T, hipMemcpyDeviceToHost, ws->stream));
    if (best_trial_out) HIP_TRY(hipMemcpyAsync(best_trial_out, d_bt, 4 * (size_t)n_pairs, hipMemcpyDeviceToHost, ws->stream));
    if (best_pose_out) HIP_TRY(hipMemcpyAsync(best_pose_out, d_bp, 64 * (size_t)n_pairs, hipMemcpyDeviceToHost, ws->stream));
    if (trial_counts_out) HIP_TRY(hipMemcpyAsync(trial_counts_out, d_cnt, 4 * NT, hipMemcpyDeviceToHost, ws->stream));
    if (trial_poses_out) HIP_TRY(hipMemcpyAsync(trial_poses_out, d_pose, 48 * NT, hipMemcpyDeviceToHost, ws->stream));
    HIP_TRY(hipStreamSynchronize(ws->stream));
    return BTBA_OK;
}

int btba_ransac_pairs(btba_workspace *ws, int n_pairs, const float *ptsA_host, const float *ptsB_host, const int32_t *n_pts,
                      int n_trials, float dist_thres, const int32_t *samples_host, uint64_t seed,
                      int32_t *inlier_ids_out, int32_t *n_inliers_out, int32_t *best_trial_out, float *best_pose_out,
                      int32_t *trial_counts_out, float *trial_poses_out)
{
    DeviceGuard device_guard(ws);
    return btba_ransac_pairs_ex(ws, BTBA_RANSAC_REFERENCE_SVD, 0, n_pairs, ptsA_host, ptsB_host, n_pts, n_trials, dist_thres, samples_host, seed,
                                inlier_ids_out, n_inliers_out, best_trial_out, best_pose_out, trial_counts_out, trial_poses_out);
}

int btba_ransac_reference_uniforms(uint64_t seed, int n_trials, float *u_out)
{
    if (n_trials < 0 || (n_trials && !u_out)) return BTBA_EINVAL;
    xorwow::ransac_uniform_table(seed, n_trials, u_out);
    return BTBA_OK;
}

void btba_match_params_default(btba_match_params *p)
{
    if (!p) return;
    p->k = 5;                                                         // FeatureManager.cpp:262 (k_near)
    p->mutual = 1;                                                    // config_ycbineoat.yml:47
    p->max_dist_neighbor = 0.03f;
    p->cos_max_normal_neighbor = (float)std::cos(45.0f / 180.0 * M_PI);
    p->max_dist_no_neighbor = 0.02f;
    p->cos_max_normal_no_neighbor = (float)std::cos(45.0f / 180.0 * M_PI);
    p->min_z = 0.1f;                                                  // FeatureManager.cpp:319
}

int btba_match_capacity(const btba_match_params *prm, int n_frames, int H, int W, int D, const int32_t *n_kpts,
                        int n_pairs, const int32_t *pairs, int64_t *capacity_out)
{
    if (!prm || prm->k < 1 || prm->k > kMatchKMax || n_frames < 1 || H < 1 || W < 1 || D < 4 || D > kMatchMaxD || D % 4 || !n_kpts || n_pairs < 0 ||
        (n_pairs && !pairs) || !capacity_out)
        return BTBA_EINVAL;
    for (int f = 0; f < n_frames; f++)
        if (n_kpts[f] < 0 || n_kpts[f] > kMatchMaxKpts) return BTBA_EINVAL;
    int64_t cap = 0;
    for (int p = 0; p < n_pairs; p++) {
        const int a = pairs[2 * p], b = pairs[2 * p + 1];
        if (a < 0 || a >= n_frames || b < 0 || b >= n_frames || a == b) return BTBA_EINVAL;
        cap += n_kpts[a] + (prm->mutual ? n_kpts[b] : 0);
    }
    if (cap > INT_MAX) return BTBA_EINVAL;                            // query and output positions are int32 on the device
    *capacity_out = cap;
    return BTBA_OK;
}

// every pointer argument btba_match_pairs / btba_corres_chain read before their first HIP call
static int match_check_frames(const btba_match_params *prm, int n_frames, int H, int W, int D, const int32_t *n_kpts, int n_pairs, const int32_t *pairs,
                              const float *K, const float *const *desc_dev, const float *const *kpts_dev, const float *const *depth_dev,
                              const float *const *normal_dev, const float *poses, const int32_t *frame_ids, int64_t *cap)
{
    int rc = btba_match_capacity(prm, n_frames, H, W, D, n_kpts, n_pairs, pairs, cap);
    if (rc) return rc;
    if (!K || !desc_dev || !kpts_dev || !depth_dev || !normal_dev || !poses || !frame_ids) return BTBA_EINVAL;
    std::vector<char> used(n_frames, 0);
    for (int p = 0; p < n_pairs; p++) used[pairs[2 * p]] = used[pairs[2 * p + 1]] = 1;
    for (int f = 0; f < n_frames; f++)
        if (used[f] && n_kpts[f] > 0 &&
            (!desc_dev[f] || !kpts_dev[f] || !depth_dev[f] || !normal_dev[f] || misaligned(desc_dev[f], 16) || misaligned(kpts_dev[f], 8) || misaligned(normal_dev[f], 16)))
            return BTBA_EINVAL;
    return BTBA_OK;
}

// The matcher's launches for validated arguments, asynchronous on the workspace stream.  The host tables stay in E until the
// caller has synchronised; E.d_cnt / E.d_off are the per-pair counts and offsets (device, in ws->match).
struct MatchEnqueue {
    std::vector<MatchFrame> fr;
    std::vector<MatchPair> pt;
    int *d_cnt = nullptr, *d_off = nullptr;
    btba_match *d_out = nullptr;
    float4 *d_pa = nullptr, *d_pb = nullptr;
};

static int match_enqueue(btba_workspace *ws, const btba_match_params *prm, bool dev, int n_frames, int H, int W, const float *K,
                         const float *const *desc_dev, int D, const float *const *kpts_dev, const int32_t *n_kpts, const float *const *depth_dev,
                         const float *const *normal_dev, const float *poses, const int32_t *frame_ids, int n_pairs, const int32_t *pairs,
                         btba_match *matches_out, float *ptsA_model_out, float *ptsB_model_out, MatchEnqueue &E)
{
    std::vector<char> used(n_frames, 0);
    for (int p = 0; p < n_pairs; p++) used[pairs[2 * p]] = used[pairs[2 * p + 1]] = 1;
    // host tables: frames, pairs (thresholds chosen by frame ids, FeatureManager.cpp:259)
    std::vector<MatchFrame> &fr = E.fr;
    fr.assign(n_frames, MatchFrame{});
    int n_norms = 0, max_n = 0;
    for (int f = 0; f < n_frames; f++) {
        MatchFrame &m = fr[f];
        m = MatchFrame{};
        m.n = used[f] ? n_kpts[f] : 0;
        m.desc = desc_dev[f]; m.kpts = reinterpret_cast<const float2 *>(kpts_dev[f]);
        m.depth = depth_dev[f]; m.normal = reinterpret_cast<const float4 *>(normal_dev[f]);
        m.norm_off = n_norms;
        n_norms += m.n;
        max_n = std::max(max_n, m.n);
        for (int k = 0; k < 12; k++) m.pose[k] = poses[16 * f + k];
    }
    std::vector<MatchPair> &pt = E.pt;
    pt.assign(n_pairs, MatchPair{});
    int qbase = 0, max_q = 0;
    for (int p = 0; p < n_pairs; p++) {
        const int a = pairs[2 * p], b = pairs[2 * p + 1];
        const bool neighbor = std::abs((long long)frame_ids[a] - (long long)frame_ids[b]) == 1;
        pt[p] = MatchPair{ a, b, qbase, 0, neighbor ? prm->max_dist_neighbor : prm->max_dist_no_neighbor,
                           neighbor ? prm->cos_max_normal_neighbor : prm->cos_max_normal_no_neighbor, 0.0f, 0.0f };
        const int nq = fr[a].n + (prm->mutual ? fr[b].n : 0);
        qbase += nq;
        max_q = std::max(max_q, nq);
    }
    const size_t Q = (size_t)qbase;
    const size_t Q1 = Q ? Q : 1;
    Scratch S;
    const auto dF = S.add<MatchFrame>(n_frames);
    const auto dP = S.add<MatchPair>(n_pairs);
    const auto d_nrm = S.add<float>(n_norms ? n_norms : 1);
    const auto d_cand = S.add<MatchCand>(prm->k * Q1);
    const auto d_sel = S.add<int>(Q1), d_pos = S.add<int>(Q1);
    const auto s_cnt = S.add<int>(n_pairs), s_off = S.add<int>(n_pairs);
    const auto s_out = S.add<btba_match>(Q1, !dev);
    const auto s_pa = S.add<float4>(Q1, !dev && ptsA_model_out), s_pb = S.add<float4>(Q1, !dev && ptsB_model_out);
    int rc;
    if ((rc = S.bind(ws->match))) return rc;
    HIP_TRY(hipMemcpyAsync(dF, fr.data(), sizeof(MatchFrame) * n_frames, hipMemcpyHostToDevice, ws->stream));
    HIP_TRY(hipMemcpyAsync(dP, pt.data(), sizeof(MatchPair) * n_pairs, hipMemcpyHostToDevice, ws->stream));

    MatchDims M{};
    M.W = W; M.H = H; M.D = D; M.k = prm->k; M.mutual = prm->mutual ? 1 : 0; M.min_z = prm->min_z;
    float intr[4];
    scaled_intrinsics(H, W, H, W, K, intr, &M.Kinv);                 // btba_depth_to_normals' inverse: the same camera-space points
    int *d_cnt = s_cnt, *d_off = s_off;
    btba_match *d_out = dev ? matches_out : s_out;
    float4 *d_pa = dev ? reinterpret_cast<float4 *>(ptsA_model_out) : s_pa;      // (nullptr when the caller wants no points)
    float4 *d_pb = dev ? reinterpret_cast<float4 *>(ptsB_model_out) : s_pb;
    if (max_n > 0) {
        k_match_norms<<<dim3((max_n + 255) / 256, n_frames), 256, 0, ws->stream>>>(dF, D, d_nrm);
        k_match_topk<<<dim3(n_pairs, (max_n + kMatchRows - 1) / kMatchRows, 1 + M.mutual), 256, 0, ws->stream>>>(M, dF, dP, d_nrm, d_cand);
    }
    k_match_select<<<n_pairs, 256, 0, ws->stream>>>(M, dF, dP, d_cand, d_sel, d_pos, d_cnt);
    k_match_offsets<<<1, 256, 0, ws->stream>>>(n_pairs, d_cnt, d_off);
    if (max_q > 0)
        k_match_pack<<<dim3(n_pairs, (max_q + 255) / 256), 256, 0, ws->stream>>>(M, dF, dP, d_cand, d_sel, d_pos, d_off, d_out, d_pa, d_pb);
    HIP_TRY(hipGetLastError());
    E.d_cnt = d_cnt; E.d_off = d_off; E.d_out = d_out; E.d_pa = d_pa; E.d_pb = d_pb;
    return BTBA_OK;
}

int btba_match_pairs(btba_workspace *ws, const btba_match_params *prm, int device_resident, int n_frames, int H, int W,
                     const float *K, const float *const *desc_dev, int D, const float *const *kpts_dev,
                     const int32_t *n_kpts, const float *const *depth_dev, const float *const *normal_dev, const float *poses,
                     const int32_t *frame_ids, int n_pairs, const int32_t *pairs,
                     btba_match *matches_out, float *ptsA_model_out, float *ptsB_model_out, int32_t *n_out)
{
    // every argument is checked before the first HIP call
    int64_t cap = 0;
    int rc = match_check_frames(prm, n_frames, H, W, D, n_kpts, n_pairs, pairs, K, desc_dev, kpts_dev, depth_dev, normal_dev, poses, frame_ids, &cap);
    if (rc) return rc;
    if (!ws || (n_pairs && !n_out) || (cap && !matches_out)) return BTBA_EINVAL;
    if (n_pairs == 0) return BTBA_OK;
    DeviceGuard device_guard(ws);
    const bool dev = device_resident != 0;
    MatchEnqueue E;
    if ((rc = match_enqueue(ws, prm, dev, n_frames, H, W, K, desc_dev, D, kpts_dev, n_kpts, depth_dev, normal_dev, poses, frame_ids, n_pairs, pairs,
                            matches_out, ptsA_model_out, ptsB_model_out, E)))
        return rc;
    HIP_TRY(hipMemcpyAsync(n_out, E.d_cnt, sizeof(int32_t) * n_pairs, hipMemcpyDeviceToHost, ws->stream));
    HIP_TRY(hipStreamSynchronize(ws->stream));                       // n_out valid; the host tables in E may go
    if (!dev) {
        size_t total = 0;
        for (int p = 0; p < n_pairs; p++) total += (size_t)n_out[p];
        if (total) {
            HIP_TRY(hipMemcpyAsync(matches_out, E.d_out, sizeof(btba_match) * total, hipMemcpyDeviceToHost, ws->stream));
            if (E.d_pa) HIP_TRY(hipMemcpyAsync(ptsA_model_out, E.d_pa, 16 * total, hipMemcpyDeviceToHost, ws->stream));
            if (E.d_pb) HIP_TRY(hipMemcpyAsync(ptsB_model_out, E.d_pb, 16 * total, hipMemcpyDeviceToHost, ws->stream));
            HIP_TRY(hipStreamSynchronize(ws->stream));
        }
    }
    return BTBA_OK;
}

int btba_window_layout(int n_windows, int n_frames, const int32_t *seg_counts, const int32_t *newframe_index, int32_t min_fm_edges_newframe,
                       int64_t *corr_stride_out, uint32_t *max_corr_per_pair_out, uint32_t *pair_offsets_out,
                       int64_t *n_edges_newframe_out, int32_t *run_ba_out)
{
    if (n_windows < 1 || n_frames < 2 || n_frames > BTBA_MAX_FRAMES || !seg_counts || !newframe_index) return BTBA_EINVAL;
    const int P = n_frames * (n_frames - 1) / 2;
    int64_t stride = 0;
    int32_t longest = 0;
    for (int w = 0; w < n_windows; w++) {                             // validate everything before the first output is written
        if (newframe_index[w] < 0 || newframe_index[w] >= n_frames) return BTBA_EINVAL;
        int64_t total = 0;
        for (int p = 0; p < P; p++) {
            const int32_t c = seg_counts[(size_t)w * P + p];
            if (c < 0) return BTBA_EINVAL;
            total += c;
            longest = std::max(longest, c);
        }
        if (total > (int64_t)UINT32_MAX) return BTBA_EINVAL;
        stride = std::max(stride, total);
    }
    for (int w = 0; w < n_windows; w++) {
        const int32_t *cnt = seg_counts + (size_t)w * P;
        const int nf = newframe_index[w];
        int64_t edges = 0;
        uint32_t at = 0;
        int p = 0;
        for (int i = 0; i < n_frames; i++)
            for (int j = i + 1; j < n_frames; j++, p++) {
                if (pair_offsets_out) pair_offsets_out[(size_t)w * (P + 1) + p] = at;
                at += (uint32_t)cnt[p];
                if (i == nf || j == nf) edges += cnt[p];
            }
        if (pair_offsets_out) pair_offsets_out[(size_t)w * (P + 1) + P] = at;
        if (n_edges_newframe_out) n_edges_newframe_out[w] = edges;
        if (run_ba_out) run_ba_out[w] = edges > (int64_t)min_fm_edges_newframe ? 1 : 0;
    }
    if (corr_stride_out) *corr_stride_out = stride;
    if (max_corr_per_pair_out) *max_corr_per_pair_out = (uint32_t)longest;
    return BTBA_OK;
}

int btba_marshal_windows(btba_workspace *ws, int n_windows, int n_frames, const btba_match *matches_dev, int64_t n_records,
                         const uint32_t *segments_dev, uint32_t max_corr_per_pair, int64_t corr_stride,
                         btba_entryj *corr_dev, uint32_t *pair_offsets_dev, float *corr24_dev)
{
    if (!ws || n_windows < 1 || n_windows > 65535 || n_frames < 2 || n_frames > BTBA_MAX_FRAMES || n_records < 0 || n_records > (int64_t)UINT32_MAX ||
        (!matches_dev && n_records) || !segments_dev || !corr_dev || !pair_offsets_dev || corr_stride < 1)
        return BTBA_EINVAL;
    if (misaligned(matches_dev, 16) || misaligned(segments_dev, 8) || misaligned(corr_dev, 16) ||
        misaligned(pair_offsets_dev, 4) || misaligned(corr24_dev, 8))
        return BTBA_EINVAL;
    DeviceGuard device_guard(ws);
    const int P = n_frames * (n_frames - 1) / 2;
    const unsigned tiles = std::max(1u, (max_corr_per_pair + (unsigned)kWinThreads - 1u) / (unsigned)kWinThreads);      // tile 0 also writes the offsets
    k_window_marshal<<<dim3(tiles, (unsigned)P, (unsigned)n_windows), kWinThreads, 0, ws->stream>>>(
        n_frames, P, segments_dev, reinterpret_cast<const unsigned char *>(matches_dev), (unsigned long long)n_records, (unsigned long long)corr_stride,
        reinterpret_cast<uint4 *>(corr_dev), pair_offsets_dev, reinterpret_cast<float2 *>(corr24_dev));
    HIP_TRY(hipGetLastError());
    return BTBA_OK;
}

int btba_procrustes_pairs(btba_workspace *ws, int device_resident, int n_pairs, const btba_match *matches_dev, int64_t n_records,
                          const int32_t *segments, const float *posesA, const float *posesB, float *pose_out, float *err_out, double *moments_out)
{
    // every argument is checked before the first HIP call
    if (!ws || n_pairs < 0 || n_records < 0 || n_records > (int64_t)UINT32_MAX) return BTBA_EINVAL;
    if (n_pairs == 0) return BTBA_OK;
    if (!segments || !posesA || !posesB || !pose_out || !err_out || (!matches_dev && n_records) || misaligned(matches_dev, 8))
        return BTBA_EINVAL;
    std::vector<KabschRec> rec(n_pairs);
    for (int e = 0; e < n_pairs; e++) {
        const int64_t off = segments[2 * e], n = segments[2 * e + 1];
        if (off < 0 || n < 0 || off + n > n_records) return BTBA_EINVAL;
        rec[e] = KabschRec{ (uint32_t)off, (int32_t)n };
    }
    DeviceGuard device_guard(ws);
    const bool dev = device_resident != 0;
    const size_t np = (size_t)n_pairs;
    Scratch S;
    const auto s_rec = S.add<KabschRec>(np);
    const auto s_mom = S.add<double>(16 * np, !(moments_out && dev));
    const auto s_pa = S.add<float>(16 * np, !dev), s_pb = S.add<float>(16 * np, !dev), s_out = S.add<float>(16 * np, !dev);
    const auto s_err = S.add<float>(np, !dev);
    int rc = S.bind(ws->window);
    if (rc) return rc;
    KabschRec *d_rec = s_rec;
    double *d_mom = moments_out && dev ? moments_out : s_mom;
    const float *pa = posesA, *pb = posesB;
    float *po = pose_out, *pe = err_out;
    HIP_TRY(hipMemcpyAsync(d_rec, rec.data(), sizeof(KabschRec) * np, hipMemcpyHostToDevice, ws->stream));
    if (!dev) {
        HIP_TRY(hipMemcpyAsync(s_pa, posesA, sizeof(float) * 16 * np, hipMemcpyHostToDevice, ws->stream));
        HIP_TRY(hipMemcpyAsync(s_pb, posesB, sizeof(float) * 16 * np, hipMemcpyHostToDevice, ws->stream));
        pa = s_pa;
        pb = s_pb;
        po = s_out;
        pe = s_err;
    }
    const unsigned char *recs = reinterpret_cast<const unsigned char *>(matches_dev);
    k_kabsch_moments<<<n_pairs, kKabschThreads, 0, ws->stream>>>(d_rec, recs, pa, pb, d_mom);
    k_kabsch_solve<<<n_pairs, kKabschThreads, 0, ws->stream>>>(d_rec, recs, pa, pb, d_mom, po, pe);
    HIP_TRY(hipGetLastError());
    if (!dev) {
        HIP_TRY(hipMemcpyAsync(pose_out, po, sizeof(float) * 16 * np, hipMemcpyDeviceToHost, ws->stream));
        HIP_TRY(hipMemcpyAsync(err_out, pe, sizeof(float) * np, hipMemcpyDeviceToHost, ws->stream));
        if (moments_out) HIP_TRY(hipMemcpyAsync(moments_out, d_mom, sizeof(double) * 16 * np, hipMemcpyDeviceToHost, ws->stream));
    }
    HIP_TRY(hipStreamSynchronize(ws->stream));                       // the host table above may go
    return BTBA_OK;
}

}  // extern "C"

// ---- map-point memory and the tracker's findCorres (btba_mappoints.hpp) ------------------------------------------------------
struct btba_mappoints {
    btba_workspace *ws = nullptr;
    int device = 0;                        // the workspace's device: destroy does not touch the workspace (it may be gone already)
    struct Slot { bool live = false; int n = 0; DevBuf data; };     // data: kpts float2[n] | canon int[n] | order int[n] | map int[n]
    std::vector<Slot> slots;
    int slot_cap = 0, mp_cap = 0;
    DevBuf table;                          // MpSlot[slot_cap]
    DevBuf img;                            // int [mp_cap][slot_cap]
    DevBuf stamp, stack;                   // int [mp_cap] each
    DevBuf hdr;                            // kMpNext, kMpTop, kMpErr
    int64_t live_known = 0;                // live map points at the last host synchronisation of forget
    int64_t bound = 0;                     // upper bound of live map points: live_known + keypoints of every slot that may still create some
    bool broken = false;                   // the device allocator's guard fired (unreachable while capacity >= bound): the memory is unusable
};

namespace {
constexpr int kMpMaxSlots = 1024;
constexpr int64_t kMpMaxImgInts = (int64_t)1 << 28;     // 1 GiB of img rows

size_t mp_slot_bytes(int n) { return (size_t)n * 8 + 3 * (size_t)n * 4 + 64; }
MpSlot mp_slot_view(btba_mappoints::Slot &s)
{
    MpSlot v{};
    unsigned char *b = s.data.as<unsigned char>();
    v.kpts = reinterpret_cast<const float2 *>(b);
    v.canon = reinterpret_cast<const int *>(b + (size_t)s.n * 8);
    v.order = reinterpret_cast<const int *>(b + (size_t)s.n * 12);
    v.map = reinterpret_cast<int *>(b + (size_t)s.n * 16);
    v.n = s.n;
    return v;
}

// grow img / stamp / stack / the slot table to (slots, points); contents kept, new entries -1.  Synchronous.
int mp_grow(btba_mappoints *M, int slots, int points)
{
    if (slots <= M->slot_cap && points <= M->mp_cap) return BTBA_OK;
    hipStream_t st = M->ws->stream;
    const int ns = std::max(slots, M->slot_cap), np = std::max(points, M->mp_cap);
    if ((int64_t)ns * np > kMpMaxImgInts || ns > kMpMaxSlots) return BTBA_ENOMEM;
    DevBuf img, stamp, stack, table;
    int rc;
    if ((rc = img.ensure((size_t)ns * np * 4)) || (rc = stamp.ensure((size_t)np * 4)) || (rc = stack.ensure((size_t)np * 4)) ||
        (rc = table.ensure(sizeof(MpSlot) * ns)))
        return rc;
    HIP_TRY(hipMemsetAsync(img.p, 0xFF, (size_t)ns * np * 4, st));
    HIP_TRY(hipMemsetAsync(stamp.p, 0xFF, (size_t)np * 4, st));
    HIP_TRY(hipMemsetAsync(table.p, 0, sizeof(MpSlot) * ns, st));
    if (M->mp_cap && M->slot_cap) {
        HIP_TRY(hipMemcpy2DAsync(img.p, (size_t)ns * 4, M->img.p, (size_t)M->slot_cap * 4, (size_t)M->slot_cap * 4, M->mp_cap, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(stack.p, M->stack.p, (size_t)M->mp_cap * 4, hipMemcpyDeviceToDevice, st));
    }
    if (M->slot_cap) HIP_TRY(hipMemcpyAsync(table.p, M->table.p, sizeof(MpSlot) * M->slot_cap, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    M->img = std::move(img); M->stamp = std::move(stamp); M->stack = std::move(stack); M->table = std::move(table);
    M->slot_cap = ns; M->mp_cap = np;
    return BTBA_OK;
}
}  // namespace

int btba_mappoints_create(btba_workspace *ws, btba_mappoints **out)
{
    if (!ws || !out) return BTBA_EINVAL;
    *out = nullptr;
    DeviceGuard device_guard(ws);
    btba_mappoints *M = new (std::nothrow) btba_mappoints;
    if (!M) return BTBA_ENOMEM;
    M->ws = ws;
    M->device = ws->device;
    int rc;
    if ((rc = M->hdr.ensure(16))) { delete M; return rc; }
    hipError_t e = hipMemsetAsync(M->hdr.p, 0, 16, ws->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ws->stream);
    if (e != hipSuccess) { g_last_hip_error = (int)e; delete M; return BTBA_EHIP; }
    *out = M;
    return BTBA_OK;
}

void btba_mappoints_destroy(btba_mappoints *M) { destroy_on_device(M); }

int btba_mappoints_register_frame(btba_mappoints *M, int n_kpts, const float *kpts_dev, int32_t *slot_out)
{
    if (!M || !slot_out || n_kpts < 0 || n_kpts > kMatchMaxKpts || (n_kpts && !kpts_dev) || misaligned(kpts_dev, 8)) return BTBA_EINVAL;
    if (M->broken) return BTBA_ENOMEM;
    DeviceGuard device_guard(M->ws);
    hipStream_t st = M->ws->stream;
    int slot = 0;
    while (slot < (int)M->slots.size() && M->slots[slot].live) slot++;
    int rc;
    // capacity first: a failure here leaves the memory as it was
    if ((rc = mp_grow(M, slot + 1 > M->slot_cap ? std::max(2 * M->slot_cap, std::max(slot + 1, 16)) : M->slot_cap,
                      M->bound + n_kpts > M->mp_cap ? (int)std::min<int64_t>(std::max<int64_t>(2 * (int64_t)M->mp_cap, M->bound + n_kpts + 1024), INT_MAX) : M->mp_cap)))
        return rc;
    btba_mappoints::Slot fresh;
    if ((rc = fresh.data.ensure(mp_slot_bytes(n_kpts)))) return rc;
    fresh.n = n_kpts;
    MpSlot v = mp_slot_view(fresh);
    int *bad = reinterpret_cast<int *>(fresh.data.as<unsigned char>() + (size_t)n_kpts * 20);
    HIP_TRY(hipMemsetAsync(bad, 0, 4, st));
    if (n_kpts) {
        HIP_TRY(hipMemcpyAsync(const_cast<float2 *>(v.kpts), kpts_dev, (size_t)n_kpts * 8, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemsetAsync(const_cast<int *>(v.order), 0xFF, (size_t)n_kpts * 4, st));
        const int g = (n_kpts + 255) / 256;
        k_mp_canon<<<g, 256, 0, st>>>(v.kpts, n_kpts, const_cast<int *>(v.canon), bad);
        k_mp_order<<<g, 256, 0, st>>>(v.kpts, n_kpts, v.canon, const_cast<int *>(v.order), v.map);
        HIP_TRY(hipGetLastError());
    }
    int bad_h = 0;
    HIP_TRY(hipMemcpyAsync(&bad_h, bad, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (bad_h) return BTBA_EINVAL;                                   // a non-finite keypoint
    HIP_TRY(hipMemcpy(M->table.as<MpSlot>() + slot, &v, sizeof(MpSlot), hipMemcpyHostToDevice));
    if (slot == (int)M->slots.size()) M->slots.emplace_back();
    fresh.live = true;
    M->slots[slot] = std::move(fresh);
    M->bound += n_kpts;
    *slot_out = slot;
    return BTBA_OK;
}

int btba_mappoints_forget_frame(btba_mappoints *M, int32_t slot)
{
    if (!M || slot < 0 || slot >= (int)M->slots.size() || !M->slots[slot].live) return BTBA_EINVAL;
    if (M->broken) return BTBA_ENOMEM;
    DeviceGuard device_guard(M->ws);
    hipStream_t st = M->ws->stream;
    if (M->mp_cap) {
        k_mp_forget<<<1, 256, 0, st>>>(slot, M->slot_cap, M->img.as<int>(), M->hdr.as<int>(), M->stack.as<int>());
        HIP_TRY(hipGetLastError());
    }
    int h[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(h, M->hdr.p, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    M->slots[slot] = btba_mappoints::Slot{};
    MpSlot dead{};
    HIP_TRY(hipMemcpy(M->table.as<MpSlot>() + slot, &dead, sizeof(MpSlot), hipMemcpyHostToDevice));
    M->live_known = h[kMpNext] - h[kMpTop];
    M->bound = M->live_known;
    for (auto &s : M->slots)
        if (s.live) M->bound += s.n;
    return BTBA_OK;
}

int btba_mappoints_export(btba_mappoints *M, int32_t *dims_out, int32_t *slot_n_out, int32_t *canon_out, int32_t *map_out, int32_t *img_out)
{
    if (!M || !dims_out) return BTBA_EINVAL;
    DeviceGuard device_guard(M->ws);
    hipStream_t st = M->ws->stream;
    int h[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(h, M->hdr.p, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const int S = (int)M->slots.size();
    int64_t total = 0;
    for (auto &s : M->slots) total += s.live ? s.n : 0;
    dims_out[0] = S; dims_out[1] = h[kMpNext]; dims_out[2] = (int32_t)total; dims_out[3] = h[kMpErr];
    if (slot_n_out)
        for (int k = 0; k < S; k++) slot_n_out[k] = M->slots[k].live ? M->slots[k].n : -1;
    int64_t off = 0;
    for (int k = 0; k < S; k++) {
        btba_mappoints::Slot &s = M->slots[k];
        if (!s.live || !s.n) continue;
        MpSlot v = mp_slot_view(s);
        if (canon_out) HIP_TRY(hipMemcpyAsync(canon_out + off, v.canon, (size_t)s.n * 4, hipMemcpyDeviceToHost, st));
        if (map_out) HIP_TRY(hipMemcpyAsync(map_out + off, v.map, (size_t)s.n * 4, hipMemcpyDeviceToHost, st));
        off += s.n;
    }
    if (img_out && h[kMpNext] && S)
        HIP_TRY(hipMemcpy2DAsync(img_out, (size_t)S * 4, M->img.p, (size_t)M->slot_cap * 4, (size_t)S * 4, h[kMpNext], hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return BTBA_OK;
}

void btba_corres_params_default(btba_corres_params *p)
{
    if (!p) return;
    p->n_trials = 2000;                                               // ransac.max_iter (btba::Config::ransac_max_iter)
    p->dist_thres = 0.01f;                                            // ransac.inlier_dist
    p->hypothesis = BTBA_RANSAC_REFERENCE_SVD;
    p->pad = 0;
    p->seed = 0;                                                      // the reference's literal curand_init seed
}

int btba_corres_chain_capacity(const btba_match_params *prm, int n_frames, int H, int W, int D, const int32_t *n_kpts,
                               int n_pairs, const int32_t *pairs, int64_t *capacity_out)
{
    int64_t nn = 0;
    int rc = btba_match_capacity(prm, n_frames, H, W, D, n_kpts, n_pairs, pairs, &nn);
    if (rc) return rc;
    std::vector<std::pair<int, int>> seen;
    seen.reserve(n_pairs);
    int64_t cap = nn;
    for (int p = 0; p < n_pairs; p++) {
        const int a = pairs[2 * p], b = pairs[2 * p + 1];
        seen.emplace_back(std::min(a, b), std::max(a, b));
        cap += n_kpts[a];                                             // propagated matches: at most one per key of A
    }
    std::sort(seen.begin(), seen.end());
    if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) return BTBA_EINVAL;     // a frame pair twice
    if (cap > INT_MAX) return BTBA_EINVAL;
    *capacity_out = cap;
    return BTBA_OK;
}

int btba_corres_chain(btba_workspace *ws, btba_mappoints *M, const btba_match_params *prm, const btba_corres_params *rprm, int device_resident,
                      int n_frames, int H, int W, const float *K, const float *const *desc_dev, int D, const float *const *kpts_dev,
                      const int32_t *n_kpts, const float *const *depth_dev, const float *const *normal_dev, const float *poses,
                      const int32_t *frame_ids, const int32_t *slots, int32_t *status, int n_pairs, const int32_t *pairs,
                      btba_match *matches_out, int32_t *n_out, int32_t *stage_counts_out)
{
    // every argument is checked before the first HIP call
    int64_t cap = 0, cap_nn = 0;
    int rc = btba_corres_chain_capacity(prm, n_frames, H, W, D, n_kpts, n_pairs, pairs, &cap);
    if (rc) return rc;
    if ((rc = match_check_frames(prm, n_frames, H, W, D, n_kpts, n_pairs, pairs, K, desc_dev, kpts_dev, depth_dev, normal_dev, poses, frame_ids, &cap_nn)))
        return rc;
    if (!ws || !M || M->ws != ws || !rprm || !slots || !status || (n_pairs && !n_out) || (cap && !matches_out)) return BTBA_EINVAL;
    if (M->broken || M->bound > M->mp_cap) return BTBA_ENOMEM;         // before any launch: nothing changes
    const int hyp = rprm->hypothesis & ~BTBA_RANSAC_DRAW_HASH;
    if (rprm->n_trials < 1 || !(rprm->dist_thres >= 0.0f) || (hyp != BTBA_RANSAC_REFERENCE_SVD && hyp != BTBA_RANSAC_HORN)) return BTBA_EINVAL;
    std::vector<int> slot_user(M->slots.size(), -1);
    for (int p = 0; p < n_pairs; p++)
        for (int s = 0; s < 2; s++) {
            const int f = pairs[2 * p + s], sl = slots[f];
            if (sl < 0 || sl >= (int)M->slots.size() || !M->slots[sl].live || M->slots[sl].n != n_kpts[f]) return BTBA_EINVAL;
            if (slot_user[sl] >= 0 && slot_user[sl] != f) return BTBA_EINVAL;    // two frames of the call on one slot
            slot_user[sl] = f;
        }
    for (int p = 0; p < n_pairs; p++)
        if (frame_ids[pairs[2 * p]] <= frame_ids[pairs[2 * p + 1]]) return BTBA_EINVAL;   // A is the newer frame
    if (n_pairs == 0) return BTBA_OK;
    DeviceGuard device_guard(ws);
    hipStream_t st = ws->stream;

    // host tables (alive until the final synchronisation)
    std::vector<CorresFrame> cf(n_frames);
    for (int f = 0; f < n_frames; f++) {
        cf[f] = CorresFrame{};
        cf[f].depth = depth_dev[f];
        for (int k = 0; k < 12; k++) cf[f].pose[k] = poses[16 * f + k];
        cf[f].slot = slots[f];
    }
    std::vector<CorresPair> cp(n_pairs);
    int64_t base = 0;
    for (int p = 0; p < n_pairs; p++) {
        const int a = pairs[2 * p], b = pairs[2 * p + 1];
        cp[p] = CorresPair{ a, b, std::abs((long long)frame_ids[a] - (long long)frame_ids[b]) == 1 ? 1 : 0, (int)base };
        base += n_kpts[a] + (prm->mutual ? n_kpts[b] : 0) + n_kpts[a];
    }
    const size_t L = (size_t)std::max<int64_t>(base, 1), Nn = (size_t)std::max<int64_t>(cap_nn, 1), NT = (size_t)rprm->n_trials;
    const bool dev = device_resident != 0;
    const size_t np = (size_t)n_pairs, n_res = (size_t)n_frames + 1 + 2 * np + 4 * np;      // status | out_off | n_out | stage
    Scratch S;
    const auto dF = S.add<CorresFrame>(n_frames);
    const auto dP = S.add<CorresPair>(np);
    const auto d_nn = S.add<btba_match>(Nn);
    const auto s_npa = S.add<float4>(Nn), s_npb = S.add<float4>(Nn);
    const auto s_list = S.add<btba_match>(L);
    const auto s_la = S.add<float4>(L), s_lb = S.add<float4>(L);
    const auto s_ids = S.add<int>(L), d_ump = S.add<int>(L), d_ua = S.add<int>(L);
    const auto s_out = S.add<btba_match>((size_t)std::max<int64_t>(cap, 1), !dev);
    const auto s_meta = S.add<int>(2 * np), s_roff = S.add<int>(2 * np);
    const auto s_best = S.add<unsigned long long>(np);
    const auto s_nin = S.add<int>(np), s_bt = S.add<int>(np);
    const auto s_bp = S.add<float>(16 * np), s_tp = S.add<float>(12 * NT);
    const auto s_tc = S.add<int>(NT);
    const auto s_res = S.add<int>(n_res + 4);                          // ... | hdr copy
    if ((rc = S.bind(ws->corres))) return rc;
    if (!(rprm->hypothesis & BTBA_RANSAC_DRAW_HASH) && (rc = ransac_uniform_table(ws, rprm->seed, rprm->n_trials))) return rc;
    int *d_status = s_res, *d_outoff = d_status + n_frames, *d_nout = d_outoff + n_pairs + 1, *d_stage = d_nout + n_pairs;
    HIP_TRY(hipMemcpyAsync(dF, cf.data(), sizeof(CorresFrame) * n_frames, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dP, cp.data(), sizeof(CorresPair) * n_pairs, hipMemcpyHostToDevice, st));
    std::vector<int32_t> st_in(status, status + n_frames);
    HIP_TRY(hipMemcpyAsync(d_status, st_in.data(), 4 * (size_t)n_frames, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(d_outoff, 0, 4, st));

    // NN for every pair at once (it reads no map state)
    float4 *d_npa = s_npa, *d_npb = s_npb;
    MatchEnqueue E;
    if ((rc = match_enqueue(ws, prm, true, n_frames, H, W, K, desc_dev, D, kpts_dev, n_kpts, depth_dev, normal_dev, poses, frame_ids, n_pairs, pairs,
                            d_nn, reinterpret_cast<float *>(d_npa), reinterpret_cast<float *>(d_npb), E)))
        return rc;

    CorresDims Cd{};
    Cd.W = W; Cd.H = H; Cd.slot_cap = M->slot_cap; Cd.mp_cap = M->mp_cap;
    float intr[4];
    scaled_intrinsics(H, W, H, W, K, intr, &Cd.Kinv);
    RansacDims Rd{};
    Rd.n_pairs = 1; Rd.n_trials = rprm->n_trials; Rd.dist_thres = rprm->dist_thres; Rd.seed = rprm->seed; Rd.hypothesis = hyp;
    Rd.draw = (rprm->hypothesis & BTBA_RANSAC_DRAW_HASH) ? 0 : 2;
    btba_match *d_list = s_list, *d_out = dev ? matches_out : s_out;
    float4 *d_la = s_la, *d_lb = s_lb;
    int *d_ids = s_ids, *d_meta = s_meta, *d_roff = s_roff, *d_nin = s_nin, *d_bt = s_bt, *d_tc = s_tc;
    unsigned long long *d_best = s_best;
    float *d_bp = s_bp, *d_tp = s_tp;
    const MpSlot *dS = M->table.as<MpSlot>();
    // per pair, in order: propagation, RANSAC (vote + inlier list), update + gates.  No host synchronisation in between.
    for (int p = 0; p < n_pairs; p++) {
        const int bs = cp[p].base;
        k_corres_prop<<<1, 256, 0, st>>>(Cd, p, dF, dP, dS, M->img.as<int>(), d_nn, d_npa, d_npb, E.d_cnt, E.d_off,
                                         d_status, d_list, d_la, d_lb, d_meta, d_roff, d_best, d_stage);
        if ((rc = ransac_enqueue(ws, Rd, d_la + bs, d_lb + bs, d_roff + 2 * p, nullptr, d_tp, d_tc, d_best + p, d_ids + bs, d_nin + p, d_bt + p, d_bp + 16 * p)))
            return rc;
        k_corres_update<<<1, 256, 0, st>>>(Cd, p, dF, dP, dS, M->img.as<int>(), M->stamp.as<int>(), M->hdr.as<int>(), M->stack.as<int>(), d_status,
                                           d_list, d_meta, d_ids, d_nin, d_ump, d_ua, d_out, d_outoff, d_nout, d_stage);
    }
    HIP_TRY(hipGetLastError());
    std::vector<int32_t> res(n_res);
    int hdr[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(res.data(), d_status, 4 * res.size(), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(hdr, M->hdr.p, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));                              // the chain's one host synchronisation
    if (hdr[kMpErr]) { M->broken = true; return BTBA_ENOMEM; }     // unreachable (capacity >= bound, checked above); should it fire, the memory is unusable
    std::memcpy(status, res.data(), 4 * (size_t)n_frames);
    const int32_t *r_off = res.data() + n_frames, *r_nout = r_off + n_pairs + 1, *r_stage = r_nout + n_pairs;
    std::memcpy(n_out, r_nout, 4 * (size_t)n_pairs);
    if (stage_counts_out) std::memcpy(stage_counts_out, r_stage, 16 * (size_t)n_pairs);
    if (!dev && r_off[n_pairs]) {
        HIP_TRY(hipMemcpyAsync(matches_out, d_out, sizeof(btba_match) * (size_t)r_off[n_pairs], hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return BTBA_OK;
}
