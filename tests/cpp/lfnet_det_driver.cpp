// lfnet_det_driver.cpp -- ctypes entry into the C++ host layer's detector net (tests/test_gpu_lfnet_det.py): a btba::LfnetScoreNet
// made from the caller's host arrays, run on caller-owned device buffers either through scores() or as the LfnetDetector::ScoreFn
// that asScoreNet() hands out, inside a btba::LfnetDetector whose descriptor net is a stand-in that describes nothing.
#include <hip/hip_runtime_api.h>

#include <vector>

#include "../../bundletrack_amd/cpp/btba_host.hpp"

// via_score_net: 0 = scores(n_frames, H, W, ...);  1 = LfnetDetector(asScoreNet(...), ...) on frame 0 (H == W), which also runs the
// keypoint head into `head` (params->pad_size is replaced by the model's) and writes the keypoint count to *n_kpts_out.
// Returns 0, a btba status, or -1 when the ScoreFn's map set is not the model's.
extern "C" __attribute__((visibility("default"))) int lfnet_det_driver(void *ws, const btba_lfnet_det_config *config,
                                                                        const btba_lfnet_det_weights *weights, int n_frames, int H, int W,
                                                                        const float *photo_dev, float *const *score_dev, float *ori_dev,
                                                                        int via_score_net, const btba_lfnet_params *params,
                                                                        const btba::LfnetBuffers *head, int *n_kpts_out)
{
    try {
        const btba::LfnetScoreNet net(static_cast<btba_workspace *>(ws), *config, *weights);
        const std::vector<float *> maps(score_dev, score_dev + config->num_scales);
        if (via_score_net) {
            if (H != W || !params || !head || !n_kpts_out) return BTBA_EINVAL;
            btba_lfnet_params p = *params;
            p.pad_size = net.padSize();
            int asked = 0;
            const btba::LfnetDetector det(static_cast<btba_workspace *>(ws), net.asScoreNet(maps, ori_dev),
                                          [&](const float *patches_dev, int m, int &dim) { asked = m; dim = 0; return (float *)nullptr; }, p, *head);
            const btba::DetectedFeatures f = det(nullptr, photo_dev, H);
            if (f.n != asked || (const float *)f.kpts_dev != head->kpts) return -1;
            *n_kpts_out = f.n;
        } else {
            net.scores(n_frames, H, W, photo_dev, maps, ori_dev);
        }
        // the model is destroyed on return: its destructor waits for the device
        return 0;
    } catch (const btba::Error &e) {
        return e.status;
    }
}
