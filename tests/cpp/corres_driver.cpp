// corres_driver.cpp -- ctypes entry into a C++ tracking session on btba::GpuFeatureManager (tests/test_gpu_corres.py): btba::Bundler with
// its own OptimizerGpu processes frames 0 .. n-1 (device data given per frame, the first pose given); the pose and status after every
// frame and the feature manager's final match records come back for the comparison with the Python session.
#include <cstring>
#include <memory>
#include <vector>

#include "../../bundletrack_amd/cpp/btba_host.hpp"

extern "C" __attribute__((visibility("default"))) int corres_session(void *ws, int n_frames, int H, int W, const float *K_rowmajor, int D,
                                                                      void *const *desc_dev, void *const *kpts_dev, const int32_t *n_kpts,
                                                                      void *const *depth_dev, void *const *normal_dev, const float *pose0_rowmajor,
                                                                      int window_size, int max_ba, float *poses_out, int32_t *status_out,
                                                                      int32_t *n_keys_out, int32_t *keys_out, int32_t *counts_out, int cap_keys,
                                                                      btba_match *records_out, int64_t cap_records)
{
    try {
        auto yml = std::make_shared<btba::Config>();
        yml->window_size = window_size;
        yml->max_BA_frames = max_ba;
        auto fm = std::make_shared<btba::GpuFeatureManager>(static_cast<btba_workspace *>(ws), yml);
        btba::Matrix3f K;
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) K(r, c) = K_rowmajor[3 * r + c];
        btba::Bundler bundler(yml, fm, K, H, W);
        for (int f = 0; f < n_frames; f++) {
            auto fr = std::make_shared<btba::Frame>();
            fr->_H = H; fr->_W = W; fr->_K = K;
            if (f == 0)
                for (int r = 0; r < 4; r++)
                    for (int c = 0; c < 4; c++) fr->_pose_in_model(r, c) = pose0_rowmajor[4 * r + c];
            fr->_n_keypts = n_kpts[f];
            fr->_feat_dim = D;
            fr->_feat_des_gpu = static_cast<float *>(desc_dev[f]);
            fr->_kpts_gpu = static_cast<float2 *>(kpts_dev[f]);
            fr->_depth_gpu = static_cast<float *>(depth_dev[f]);
            fr->_normal_gpu = static_cast<float4 *>(normal_dev[f]);
            bundler.processNewFrame(fr);
            for (int r = 0; r < 4; r++)
                for (int c = 0; c < 4; c++) poses_out[16 * f + 4 * r + c] = fr->_pose_in_model(r, c);
            status_out[f] = fr->_status == btba::Frame::FAIL ? 1 : 0;
        }
        int k = 0;
        int64_t o = 0;
        for (const auto &kv : fm->_records) {
            if (k >= cap_keys || o + (int64_t)kv.second.size() > cap_records) return 1;
            keys_out[2 * k] = kv.first.first; keys_out[2 * k + 1] = kv.first.second;
            counts_out[k] = (int32_t)kv.second.size();
            if (!kv.second.empty()) std::memcpy(records_out + o, kv.second.data(), sizeof(btba_match) * kv.second.size());
            o += (int64_t)kv.second.size();
            k++;
        }
        *n_keys_out = k;
        return 0;
    } catch (const btba::Error &e) {
        return e.status ? e.status : 1;
    } catch (...) {
        return 1;
    }
}
