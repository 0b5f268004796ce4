// detector_driver.cpp -- ctypes entry into the C++ host layer's DetectorFeatureManager (tests/test_gpu_detector.py), directly or
// through Bundler::processNewFrame.  Frames are described by flat arrays of device pointers; the stand-in detector hands back the
// caller's keypoint buffers (detector pixels), which detectFeature maps back in place.
#include <memory>
#include <vector>

#include "../../bundletrack_amd/cpp/btba_host.hpp"

namespace {
struct DetectorOnly : btba::DetectorFeatureManager {
    using btba::DetectorFeatureManager::DetectorFeatureManager;
    void findCorres(const std::shared_ptr<btba::Frame> &, const std::shared_ptr<btba::Frame> &) override {}
};
}  // namespace

// via_bundler = 0: detectFeature on each frame; 1: each frame through a fresh Bundler's processNewFrame (a first frame: no BA).
// Frame f writes its detector input to bgr_out + f S S 3 and gray_out + f S S.  n_calls_out: how often the detector ran;
// n_keypts_out[f], status_out[f] (0 FAIL, 1 NO_BA, 2 OTHER) per frame.
extern "C" __attribute__((visibility("default"))) int detector_driver(void *ws, int via_bundler, int n_frames, int H, int W, int S,
                                                                       void *const *color_dev, const float *roi, void *const *kpts_dev,
                                                                       const int32_t *n_kpts, void *const *desc_dev, int D, uint8_t *bgr_out,
                                                                       float *gray_out, int32_t *n_calls_out, int32_t *n_keypts_out, int32_t *status_out)
{
    try {
        int calls = 0;
        for (int f = 0; f < n_frames; f++) {
            auto fr = std::make_shared<btba::Frame>();
            fr->_H = H; fr->_W = W;
            fr->_color_gpu = static_cast<uchar4 *>(color_dev[f]);
            for (int q = 0; q < 4; q++) fr->_roi[q] = roi[4 * f + q];
            auto detect = [&, f](const uint8_t *, const float *, int) {
                calls++;
                btba::DetectedFeatures d;
                d.kpts_dev = static_cast<float2 *>(kpts_dev[f]);
                d.desc_dev = static_cast<float *>(desc_dev[f]);
                d.n = n_kpts[f];
                d.dim = D;
                return d;
            };
            auto fm = std::make_shared<DetectorOnly>(static_cast<btba_workspace *>(ws), detect, bgr_out ? bgr_out + (size_t)f * S * S * 3 : nullptr,
                                                     gray_out ? gray_out + (size_t)f * S * S : nullptr, S);
            if (!via_bundler) {
                fm->detectFeature(fr);
            } else {
                btba::Matrix3f K{};
                K(0, 0) = K(1, 1) = 500.0f; K(0, 2) = W / 2.0f; K(1, 2) = H / 2.0f; K(2, 2) = 1.0f;
                btba::Bundler b(std::make_shared<btba::Config>(), fm, K, H, W,
                                [](const std::vector<btba::EntryJ> &, const std::vector<int> &, int, int, int, const std::vector<float *> &,
                                   const std::vector<uchar4 *> &, const std::vector<float4 *> &, std::vector<btba::Matrix4f> &, const btba::Matrix3f &) {});
                b.processNewFrame(fr);
            }
            n_keypts_out[f] = fr->_n_keypts;
            status_out[f] = (int32_t)fr->_status;
        }
        *n_calls_out = calls;
        return 0;
    } catch (const btba::Error &e) {
        return e.status;
    }
}
