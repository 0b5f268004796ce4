// vos_driver.cpp -- ctypes entry into the C++ host layer's MaskPropagator (tests/test_gpu_vos.py): one video's session on
// caller-owned device buffers, directly or through Bundler::processNewFrame's hook.  The "backbone" is a device copy of the frame's
// prepared features into the slot the propagator names.
#include <hip/hip_runtime_api.h>

#include <memory>
#include <vector>

#include "../../bundletrack_amd/cpp/btba_host.hpp"

namespace {
struct NoFeatures : btba::FeatureManager {
    void findCorres(const std::shared_ptr<btba::Frame> &, const std::shared_ptr<btba::Frame> &) override {}
};
}  // namespace

// feats_in_dev [n_frames][C][Hd*Wd]; label_dev uint8 [H*W] (classes 0 .. d-1) of frame 0; ring buffers as btba::MaskPropagator takes
// them; masks_out_dev [n_frames - 1][H*W] receives the class map of every later frame.  Returns 0, a btba status, or -1 for a HIP error.
extern "C" __attribute__((visibility("default"))) int vos_session_driver(void *ws, int d, int H, int W, int C, int range, int n_frames,
                                                                          const float *feats_in_dev, const uint8_t *label_dev, float *ring_feats,
                                                                          float *ring_labels, float *pred, uint8_t *mask, uint8_t *masks_out_dev)
{
    try {
        btba_vos_params p = btba::vosParams();
        p.range = range;
        btba::MaskPropagator mp(static_cast<btba_workspace *>(ws), d, H, W, C, p, ring_feats, ring_labels, pred, mask);
        const size_t fl = (size_t)C * mp.Hd * mp.Wd;
        for (int f = 0; f < n_frames; f++) {
            if (hipMemcpy(mp.nextFeatures(), feats_in_dev + f * fl, sizeof(float) * fl, hipMemcpyDeviceToDevice) != hipSuccess) return -1;
            if (f == 0) { mp.start(label_dev); continue; }
            const uint8_t *m = mp.step();
            if (hipMemcpy(masks_out_dev + (size_t)(f - 1) * H * W, m, (size_t)H * W, hipMemcpyDeviceToDevice) != hipSuccess) return -1;
        }
        return 0;
    } catch (const btba::Error &e) {
        return e.status;
    }
}

// The same session through Bundler::processNewFrame: every frame brings bgr_dev[f] (uint8 [H*W*3]) and shared depth / normal maps,
// frame 0 also label_dev as its mask; each frame goes through a fresh Bundler (a first frame: no BA) that shares the propagator.
// rgb_dev float [3][H][W] receives the normalised image of the last frame.
extern "C" __attribute__((visibility("default"))) int vos_bundler_driver(void *ws, int d, int H, int W, int C, int range, int n_frames,
                                                                          const float *feats_in_dev, uint8_t *label_dev, float *ring_feats,
                                                                          float *ring_labels, float *pred, uint8_t *mask, uint8_t *masks_out_dev,
                                                                          void *const *bgr_dev, float *depth_dev, float *normal_dev, float *rgb_dev)
{
    try {
        btba_vos_params p = btba::vosParams();
        p.range = range;
        auto mp = std::make_shared<btba::MaskPropagator>(static_cast<btba_workspace *>(ws), d, H, W, C, p, ring_feats, ring_labels, pred, mask);
        const size_t fl = (size_t)C * mp->Hd * mp->Wd;
        auto cfg = std::make_shared<btba::Config>();
        btba::Matrix3f K{};
        K(0, 0) = K(1, 1) = 500.0f; K(0, 2) = 0.5f * W; K(1, 2) = 0.5f * H; K(2, 2) = 1.0f;
        bool copy_failed = false;
        for (int f = 0; f < n_frames; f++) {
            btba::Bundler b(cfg, std::make_shared<NoFeatures>(), K, H, W,
                            [](const std::vector<btba::EntryJ> &, const std::vector<int> &, int, int, int, const std::vector<float *> &,
                               const std::vector<uchar4 *> &, const std::vector<float4 *> &, std::vector<btba::Matrix4f> &, const btba::Matrix3f &) {});
            b.mask_ws = static_cast<btba_workspace *>(ws);
            b.mask_propagator = mp;
            b.rgb_dev = rgb_dev;
            b.segmenter = [&](const float *, float *out) {
                if (hipMemcpy(out, feats_in_dev + f * fl, sizeof(float) * fl, hipMemcpyDeviceToDevice) != hipSuccess) copy_failed = true;
            };
            auto fr = std::make_shared<btba::Frame>();
            fr->_H = H; fr->_W = W;
            fr->_bgr_gpu = static_cast<const uint8_t *>(bgr_dev[f]);
            fr->_depth_gpu = depth_dev;
            fr->_normal_gpu = reinterpret_cast<float4 *>(normal_dev);
            if (f == 0) fr->_mask_gpu = label_dev;
            b.processNewFrame(fr);
            if (copy_failed || !fr->_mask_gpu) return -1;
            if (f > 0 && hipMemcpy(masks_out_dev + (size_t)(f - 1) * H * W, fr->_mask_gpu, (size_t)H * W, hipMemcpyDeviceToDevice) != hipSuccess) return -1;
        }
        return mp->n_frames == n_frames ? 0 : -2;
    } catch (const btba::Error &e) {
        return e.status;
    }
}
