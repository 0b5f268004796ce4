// objective_driver.cpp -- ctypes entry into the C++ host layer's btba::objectiveBatchZn (tests/test_gpu_objective_cpp.py).
// Every array is a device pointer; K is row-major on the host.  Also returns btba::residualVariance of a total given on the host.
#include <utility>
#include <vector>

#include "../../bundletrack_amd/cpp/btba_host.hpp"

extern "C" __attribute__((visibility("default"))) int objective_driver(void *ws, int n_instances, int n_frames, int H, int W, const float *K_rowmajor,
                                                                        const float *zn_dev, const void *corr_dev, int64_t corr_stride,
                                                                        const uint32_t *pair_offsets_dev, uint32_t max_corr_per_pair,
                                                                        const int32_t *dense_pairs, int n_dense_pairs, const float *poses_dev,
                                                                        void *total_dev, void *sparse_dev, void *dense_dev)
{
    try {
        btba_params prm;
        btba_params_default(&prm);
        btba::Matrix3f K;
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) K(r, c) = K_rowmajor[3 * r + c];
        std::vector<std::pair<int32_t, int32_t>> dp;
        for (int q = 0; q < n_dense_pairs; q++) dp.emplace_back(dense_pairs[2 * q], dense_pairs[2 * q + 1]);
        btba::objectiveBatchZn(static_cast<btba_workspace *>(ws), prm, n_instances, n_frames, H, W, K, zn_dev, nullptr, static_cast<const btba_entryj *>(corr_dev),
                               corr_stride, pair_offsets_dev, max_corr_per_pair, dp, poses_dev, static_cast<btba_objective_total *>(total_dev),
                               static_cast<btba_objective_pair *>(sparse_dev), static_cast<btba_objective_pair *>(dense_dev));
        return 0;
    } catch (const btba::Error &e) {
        return e.status;
    }
}

extern "C" __attribute__((visibility("default"))) double objective_driver_variance(const void *total_host, int n_frames)
{
    return btba::residualVariance(*static_cast<const btba_objective_total *>(total_host), n_frames);
}
