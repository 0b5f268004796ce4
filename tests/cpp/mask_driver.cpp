// mask_driver.cpp -- ctypes entry into the C++ host layer's segmentationByMaskMultiFrame (tests/test_gpu_mask.py) and into
// Bundler::processNewFrame's segmentation step.  Frames are described by flat arrays of device pointers; the ROIs and the
// statuses come back in host arrays.
#include <memory>
#include <vector>

#include "../../bundletrack_amd/cpp/btba_host.hpp"

namespace {
struct NoFeatures : btba::FeatureManager {
    void findCorres(const std::shared_ptr<btba::Frame> &, const std::shared_ptr<btba::Frame> &) override {}
};
}  // namespace

// via_bundler = 0: segmentationByMaskMultiFrame on all frames at once; 1: each frame through a fresh Bundler's processNewFrame
// (config mask_largest_component_hull / mask_dilate, workspace mask_ws), status_out[f] = 0 FAIL, 1 NO_BA, 2 OTHER.
extern "C" __attribute__((visibility("default"))) int mask_driver(void *ws, int via_bundler, int n_frames, int H, int W, int hull, int dilate,
                                                                   void *const *mask_dev, void *const *depth_dev, void *const *normal_dev,
                                                                   void *const *color_dev, void *const *fg_out_dev, float *roi_out, int32_t *status_out)
{
    try {
        std::vector<std::shared_ptr<btba::Frame>> frames(n_frames);
        for (int f = 0; f < n_frames; f++) {
            auto fr = std::make_shared<btba::Frame>();
            fr->_H = H; fr->_W = W;
            fr->_mask_gpu = static_cast<uint8_t *>(mask_dev[f]);
            fr->_depth_gpu = static_cast<float *>(depth_dev[f]);
            fr->_normal_gpu = static_cast<float4 *>(normal_dev[f]);
            fr->_color_gpu = color_dev ? static_cast<uchar4 *>(color_dev[f]) : nullptr;
            fr->_fg_mask_gpu = fg_out_dev ? static_cast<uint8_t *>(fg_out_dev[f]) : nullptr;
            frames[f] = fr;
        }
        if (!via_bundler) {
            btba::segmentationByMaskMultiFrame(static_cast<btba_workspace *>(ws), frames, hull != 0, dilate);
        } else {
            auto cfg = std::make_shared<btba::Config>();
            cfg->mask_largest_component_hull = hull != 0;
            cfg->mask_dilate = dilate;
            btba::Matrix3f K{};
            K(0, 0) = K(1, 1) = 500.0f; K(0, 2) = W / 2.0f; K(1, 2) = H / 2.0f; K(2, 2) = 1.0f;
            for (int f = 0; f < n_frames; f++) {                     // a fresh Bundler per frame: each frame is a first frame (no BA)
                btba::Bundler b(cfg, std::make_shared<NoFeatures>(), K, H, W,
                                [](const std::vector<btba::EntryJ> &, const std::vector<int> &, int, int, int, const std::vector<float *> &,
                                   const std::vector<uchar4 *> &, const std::vector<float4 *> &, std::vector<btba::Matrix4f> &, const btba::Matrix3f &) {});
                b.mask_ws = static_cast<btba_workspace *>(ws);
                b.processNewFrame(frames[f]);
            }
        }
        for (int f = 0; f < n_frames; f++) {
            for (int q = 0; q < 4; q++) roi_out[4 * f + q] = frames[f]->_roi[q];
            status_out[f] = (int32_t)frames[f]->_status;
        }
        return 0;
    } catch (const btba::Error &e) {
        return e.status;
    }
}
