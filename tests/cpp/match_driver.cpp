// match_driver.cpp -- ctypes entry into the C++ host layer's FeatureManager::findCorresbyNNMultiPair (tests/test_gpu_matching.py).
// Frames are described by flat host arrays (device pointers for the per-frame data); the matches of every pair come back
// concatenated, pair after pair, with their counts.
#include <cstring>
#include <memory>
#include <vector>

#include "../../bundletrack_amd/cpp/btba_host.hpp"

namespace {
struct NoFeatures : btba::FeatureManager {
    void findCorres(const std::shared_ptr<btba::Frame> &, const std::shared_ptr<btba::Frame> &) override {}
};
}  // namespace

extern "C" __attribute__((visibility("default"))) int match_driver(void *ws, int n_frames, int H, int W, const float *K_rowmajor, int D,
                                                                    void *const *desc_dev, void *const *kpts_dev, const int32_t *n_kpts,
                                                                    void *const *depth_dev, void *const *normal_dev, const float *poses_rowmajor,
                                                                    const int32_t *frame_ids, int n_pairs, const int32_t *pairs,
                                                                    float *ptA_out, float *ptB_out, int32_t *n_out)
{
    try {
        std::vector<std::shared_ptr<btba::Frame>> frames(n_frames);
        for (int f = 0; f < n_frames; f++) {
            auto fr = std::make_shared<btba::Frame>();
            fr->_id = frame_ids[f];
            fr->_H = H; fr->_W = W;
            for (int r = 0; r < 3; r++)
                for (int c = 0; c < 3; c++) fr->_K(r, c) = K_rowmajor[3 * r + c];
            for (int r = 0; r < 4; r++)
                for (int c = 0; c < 4; c++) fr->_pose_in_model(r, c) = poses_rowmajor[16 * f + 4 * r + c];
            fr->_n_keypts = n_kpts[f];
            fr->_feat_dim = D;
            fr->_feat_des_gpu = static_cast<float *>(desc_dev[f]);
            fr->_kpts_gpu = static_cast<float2 *>(kpts_dev[f]);
            fr->_depth_gpu = static_cast<float *>(depth_dev[f]);
            fr->_normal_gpu = static_cast<float4 *>(normal_dev[f]);
            frames[f] = fr;
        }
        std::vector<std::pair<std::shared_ptr<btba::Frame>, std::shared_ptr<btba::Frame>>> pr;
        for (int p = 0; p < n_pairs; p++) pr.emplace_back(frames[pairs[2 * p]], frames[pairs[2 * p + 1]]);
        NoFeatures fm;
        fm.findCorresbyNNMultiPair(static_cast<btba_workspace *>(ws), pr);
        size_t o = 0;
        for (int p = 0; p < n_pairs; p++) {
            const auto &m = fm._matches[{ pr[p].first->_id, pr[p].second->_id }];
            n_out[p] = (int32_t)(m.ptA_cam.size() / 3);
            std::memcpy(ptA_out + o, m.ptA_cam.data(), sizeof(float) * m.ptA_cam.size());
            std::memcpy(ptB_out + o, m.ptB_cam.data(), sizeof(float) * m.ptB_cam.size());
            o += m.ptA_cam.size();
        }
        return 0;
    } catch (const btba::Error &e) {
        return e.status;
    }
}
