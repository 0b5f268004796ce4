// vos_net_driver.cpp -- ctypes entry into the C++ host layer's segmentation backbone (tests/test_gpu_vos_net.py): a btba::VosBackbone
// made from the caller's host records, run on caller-owned device buffers either through features() or, frame by frame, as the
// Bundler::SegmentFn that asSegmenter() hands out.
#include <hip/hip_runtime_api.h>

#include <vector>

#include "../../bundletrack_amd/cpp/btba_host.hpp"

// via_segmenter: 0 = features(n_frames, H, W, ...);  1 = asSegmenter(H, W) called once per frame.  Returns 0 or a btba status.
extern "C" __attribute__((visibility("default"))) int vos_net_driver(void *ws, const btba_vos_net_config *config, const btba_vos_net_layer *layers,
                                                                      int n_layers, int n_frames, int H, int W, const float *rgb_dev,
                                                                      float *features_out_dev, int via_segmenter)
{
    try {
        const btba::VosBackbone net(static_cast<btba_workspace *>(ws), *config, std::vector<btba_vos_net_layer>(layers, layers + (n_layers > 0 ? n_layers : 0)));
        if (via_segmenter) {
            int32_t Hd = 0, Wd = 0;
            if (btba_vos_net_out_size(H, W, &Hd, &Wd) != BTBA_OK) return BTBA_EINVAL;
            const btba::Bundler::SegmentFn fn = net.asSegmenter(H, W);
            for (int f = 0; f < n_frames; f++) fn(rgb_dev + (size_t)f * 3 * H * W, features_out_dev + (size_t)f * 256 * Hd * Wd);
        } else {
            net.features(n_frames, H, W, rgb_dev, features_out_dev);
        }
        // the model is destroyed on return: its destructor waits for the device
        return 0;
    } catch (const btba::Error &e) {
        return e.status;
    }
}
