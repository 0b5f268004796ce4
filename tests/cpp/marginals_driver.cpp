// marginals_driver.cpp -- ctypes entry into the C++ host layer's btba::linearizeBatchZn and btba::poseCovariances
// (tests/test_gpu_marginals_cpp.py).  Every array is a device pointer; K is row-major on the host.
#include <vector>

#include "../../bundletrack_amd/cpp/btba_host.hpp"

extern "C" __attribute__((visibility("default"))) int marginals_driver(void *ws, int n_gn_iters, int n_instances, int n_frames, int H, int W,
                                                                        const float *K_rowmajor, const float *zn_dev, const void *corr_dev,
                                                                        int64_t corr_stride, const uint32_t *pair_offsets_dev,
                                                                        uint32_t max_corr_per_pair, const float *poses_dev, float *info_dev,
                                                                        float *rhs_dev, double *cov_blocks_dev, double *cov_full_dev,
                                                                        double *pivot_ratio_dev, int32_t *status_dev)
{
    try {
        btba_params prm;
        btba_params_default(&prm);
        prm.n_gn_iters = n_gn_iters;
        btba::Matrix3f K;
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) K(r, c) = K_rowmajor[3 * r + c];
        btba_workspace *w = static_cast<btba_workspace *>(ws);
        btba::linearizeBatchZn(w, prm, n_instances, n_frames, H, W, K, zn_dev, nullptr, static_cast<const btba_entryj *>(corr_dev), corr_stride,
                               pair_offsets_dev, max_corr_per_pair, {}, poses_dev, info_dev, rhs_dev);
        btba::poseCovariances(w, n_instances, n_frames, info_dev, cov_blocks_dev, status_dev, cov_full_dev, pivot_ratio_dev);
        return 0;
    } catch (const btba::Error &e) {
        return e.status;
    }
}
