// btba_api_marginals.hip -- how well a window constrains its poses: the solver's system at the caller's poses
// (btba_linearize_batch_zn_aux) and the batched fp64 inverse of its matrix (btba_pose_covariances).  Kernels: btba_marginals.hpp.
#include "btba_host_common.hpp"
#include "btba_marginals.hpp"

static_assert(kMarginalsMaxFrames == BTBA_MAX_FRAMES_LDS, "the covariance kernel serves the windows whose matrix the solve keeps in LDS");
static_assert(marginals_unknowns(kMarginalsMaxFrames) <= kMarginalsBlock, "one lane per unknown");
static_assert(marginals_lds_bytes(kMarginalsMaxFrames) <= kMarginalsLdsLimit, "the largest window's packed triangle and vectors fit one compute unit's LDS");

extern "C" {

int btba_linearize_batch_zn_aux(btba_workspace *ws, const btba_params *params, int n_instances, int n_frames, int H, int W, const float *K,
                                const float *zn_dev, const btba_zn_aux *aux, const btba_entryj *corr_dev, int64_t corr_stride,
                                const uint32_t *pair_offsets_dev, uint32_t max_corr_per_pair, const int32_t *dense_pairs, int n_dense_pairs,
                                const float *poses_dev, float *info_dev, float *rhs_dev)
{
    // (argument checks first: none of them touches the device)
    if (!ws || !params || !poses_dev || !info_dev || n_instances < 1 || n_frames < 2 || n_frames > BTBA_MAX_FRAMES) return BTBA_EINVAL;
    if (params->weights_sparse_per_iter || params->weights_dense_per_iter) return BTBA_EINVAL;      // the system of WHICH iterate?  the scalar weights say
    DeviceGuard device_guard(ws);
    const int B = n_instances, N = n_frames, na = 6 * (N - 1);
    // One traced iterate of the solve itself, on a copy of the poses: whichever kernel the dispatch picks for this window assembles the system
    // exactly as it does inside a solve, and its trace record holds it.  The iterate's update lands in the copy and is dropped.
    btba_params prm = *params;
    prm.n_gn_iters = 1;
    prm.n_pcg_iters = 1;                                        // (the system is recorded before the PCG starts)
    prm.n_weights_per_iter = 0;
    prm.flags = (prm.flags | BTBA_FLAG_TRACE) & ~(BTBA_FLAG_TIME_KERNELS | BTBA_FLAG_TIME_SAMPLED);
    int Pd = 0;                                                 // dense pairs in the record: as solve_enqueue counts them
    if (prm.weight_dense_depth > 0.0f) Pd = dense_pairs ? n_dense_pairs : N * (N - 1) / 2;
    if (Pd < 0) return BTBA_EINVAL;
    btba_trace_layout L;
    btba_trace_layout_get(N, Pd, prm.n_pcg_iters, &L);
    Scratch scratch;
    auto poses = scratch.add<float>(16 * (size_t)B * N);
    auto trace = scratch.add<float>((size_t)B * (size_t)L.record_floats);
    if (int rc = scratch.bind(ws->marginals)) return rc;
    HIP_TRY(hipMemcpyAsync(poses, poses_dev, sizeof(float) * 16 * (size_t)B * N, hipMemcpyDeviceToDevice, ws->stream));
    const btba_stats stats = ws->stats;                         // a linearisation is not a solve: the workspace's figures stay those of the last one
    const int rc = btba_solve_batch_zn_aux(ws, &prm, B, N, H, W, K, zn_dev, aux, corr_dev, corr_stride, pair_offsets_dev, max_corr_per_pair,
                                           dense_pairs, n_dense_pairs, poses, trace);
    ws->stats = stats;
    if (rc != BTBA_OK) return rc;
    k_gather_system<<<dim3((unsigned)((na * na + 255) / 256), (unsigned)B), 256, 0, ws->stream>>>(N, trace, L.record_floats, L.off_A, L.off_rhs, info_dev, rhs_dev);
    HIP_TRY(hipGetLastError());
    return BTBA_OK;
}

int btba_pose_covariances(btba_workspace *ws, int n_instances, int n_frames, const float *info_dev, int64_t info_stride,
                          double *cov_blocks_dev, double *cov_full_dev, double *pivot_ratio_dev, int32_t *status_dev)
{
    if (!ws || n_instances < 1 || n_frames < 2 || n_frames > BTBA_MAX_FRAMES_LDS || !info_dev || !cov_blocks_dev || !status_dev) return BTBA_EINVAL;
    const int64_t na = marginals_unknowns(n_frames);
    if (info_stride < na * na) return BTBA_EINVAL;
    if (misaligned(info_dev, 4) || misaligned(cov_blocks_dev, 8) || misaligned(cov_full_dev, 8) || misaligned(pivot_ratio_dev, 8) || misaligned(status_dev, 4)) return BTBA_EINVAL;
    DeviceGuard device_guard(ws);
    const MarginalsLayout lay(n_frames);
    if (lay.total > kMarginalsLdsLimit) return BTBA_EINVAL;
    if (!ws->marginals_attr_set) {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_pose_covariances), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMarginalsLdsLimit));
        ws->marginals_attr_set = true;
    }
    MarginalsArgs A{};
    A.n_frames = n_frames; A.info_stride = info_stride; A.info = info_dev;
    A.cov_blocks = cov_blocks_dev; A.cov_full = cov_full_dev; A.pivot_ratio = pivot_ratio_dev; A.status = status_dev;
    k_pose_covariances<<<(unsigned)n_instances, kMarginalsBlock, lay.total, ws->stream>>>(A);
    HIP_TRY(hipGetLastError());
    return BTBA_OK;
}

}  // extern "C"
