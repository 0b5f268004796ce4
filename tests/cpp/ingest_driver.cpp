// ingest_driver.cpp -- ctypes entry into the C++ host layer's ingestFrames (tests/test_gpu_ingest.py) and into
// Bundler::processNewFrame's ingest step.  Frames are described by flat arrays of device pointers.
#include <memory>
#include <vector>

#include "../../bundletrack_amd/cpp/btba_host.hpp"

namespace {
struct NoFeatures : btba::FeatureManager {
    void findCorres(const std::shared_ptr<btba::Frame> &, const std::shared_ptr<btba::Frame> &) override {}
};
}  // namespace

// via_bundler = 0: ingestFrames on all frames at once with K in every frame; 1: each frame through a fresh Bundler's processNewFrame
// (the Bundler's K, workspace mask_ws).  ingested_out[f] = Frame::_ingested afterwards.  bgr_dev / color_dev / raw_dev / xyz_dev may be
// null, and so may their entries.
extern "C" __attribute__((visibility("default"))) int ingest_driver(void *ws, int via_bundler, int n_frames, int H, int W, const float *K_rowmajor,
                                                                     void *const *code_dev, void *const *bgr_dev, void *const *depth_dev,
                                                                     void *const *normal_dev, void *const *color_dev, void *const *raw_dev,
                                                                     void *const *xyz_dev, int32_t *ingested_out)
{
    try {
        btba::Matrix3f K{};
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) K(r, c) = K_rowmajor[3 * r + c];
        std::vector<std::shared_ptr<btba::Frame>> frames(n_frames);
        for (int f = 0; f < n_frames; f++) {
            auto fr = std::make_shared<btba::Frame>();
            fr->_H = H; fr->_W = W;
            if (!via_bundler) fr->_K = K;
            fr->_depth_code_gpu = static_cast<const uint16_t *>(code_dev[f]);
            fr->_bgr_gpu = bgr_dev ? static_cast<const uint8_t *>(bgr_dev[f]) : nullptr;
            fr->_depth_gpu = static_cast<float *>(depth_dev[f]);
            fr->_normal_gpu = static_cast<float4 *>(normal_dev[f]);
            fr->_color_gpu = color_dev ? static_cast<uchar4 *>(color_dev[f]) : nullptr;
            fr->_depth_raw_gpu = raw_dev ? static_cast<float *>(raw_dev[f]) : nullptr;
            fr->_xyz_gpu = xyz_dev ? static_cast<float4 *>(xyz_dev[f]) : nullptr;
            frames[f] = fr;
        }
        if (!via_bundler) {
            btba::ingestFrames(static_cast<btba_workspace *>(ws), frames, btba::ingestParams());
        } else {
            auto cfg = std::make_shared<btba::Config>();
            for (int f = 0; f < n_frames; f++) {                     // a fresh Bundler per frame: each frame is a first frame (no BA)
                btba::Bundler b(cfg, std::make_shared<NoFeatures>(), K, H, W,
                                [](const std::vector<btba::EntryJ> &, const std::vector<int> &, int, int, int, const std::vector<float *> &,
                                   const std::vector<uchar4 *> &, const std::vector<float4 *> &, std::vector<btba::Matrix4f> &, const btba::Matrix3f &) {});
                b.mask_ws = static_cast<btba_workspace *>(ws);
                b.processNewFrame(frames[f]);
            }
        }
        for (int f = 0; f < n_frames; f++) ingested_out[f] = frames[f]->_ingested ? 1 : 0;
        return 0;
    } catch (const btba::Error &e) {
        return e.status;
    }
}
