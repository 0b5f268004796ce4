// eval_driver.cpp -- ctypes entry into the C++ host layer's btba::poseErrors and btba::vocapAuc (tests/test_gpu_eval.py,
// tests/test_eval_ref.py).  Poses are flat row-major host arrays; models are device pointers.
#include <vector>

#include "../../bundletrack_amd/cpp/btba_host.hpp"

namespace {
btba::Matrix4f from_rowmajor(const float *p)
{
    btba::Matrix4f M;
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) M(r, c) = p[4 * r + c];
    return M;
}
}  // namespace

extern "C" __attribute__((visibility("default"))) int pose_errors_driver(void *ws, int n_models, void *const *models_dev, const int32_t *n_pts,
                                                                          int n_evals, const int32_t *model_index, const float *poses_pred,
                                                                          const float *poses_gt, float *add_out, float *adds_out)
{
    try {
        std::vector<const float *> models(n_models);
        for (int m = 0; m < n_models; m++) models[m] = static_cast<const float *>(models_dev[m]);
        std::vector<btba::Matrix4f> pp, pg;
        for (int e = 0; e < n_evals; e++) {
            pp.push_back(from_rowmajor(poses_pred + 16 * e));
            pg.push_back(from_rowmajor(poses_gt + 16 * e));
        }
        std::vector<float> add, adds;
        btba::poseErrors(static_cast<btba_workspace *>(ws), models, std::vector<int32_t>(n_pts, n_pts + n_models),
                         std::vector<int32_t>(model_index, model_index + n_evals), pp, pg, add, adds);
        for (int e = 0; e < n_evals; e++) { add_out[e] = add[e]; adds_out[e] = adds[e]; }
        return 0;
    } catch (const btba::Error &e) {
        return e.status;
    }
}

extern "C" __attribute__((visibility("default"))) double vocap_driver(const double *errors, int n, double max_threshold)
{
    return btba::vocapAuc(std::vector<double>(errors, errors + n), max_threshold);
}
