// lfnet_driver.cpp -- ctypes entry into the C++ host layer's keypoint head (tests/test_gpu_lfnet.py): btba::lfnetKeypoints on
// caller-owned device buffers, directly or as btba::LfnetDetector called the way DetectorFeatureManager calls its detector.  The
// "score net" hands back prepared score maps and ori_maps; the "descriptor net" hands back the patches themselves (dim = P * P).
#include <hip/hip_runtime_api.h>

#include <vector>

#include "../../bundletrack_amd/cpp/btba_host.hpp"

namespace {
btba::LfnetMapSet map_set(int S, const float *const *score_dev, const int32_t *map_h, const int32_t *map_w, const float *scale_factors)
{
    btba::LfnetMapSet m;
    m.score_dev.assign(score_dev, score_dev + S);
    m.map_h.assign(map_h, map_h + S);
    m.map_w.assign(map_w, map_w + S);
    m.scale_factors.assign(scale_factors, scale_factors + S);
    return m;
}
}  // namespace

// out: max_heatmaps, max_scales, kpts_xy, n_kpts, kpts, kpts_scale, kpts_ori, patches (device); counts_out: host int32 [n_frames].
// Returns 0 or a btba status.
extern "C" __attribute__((visibility("default"))) int lfnet_keypoints_driver(void *ws, int n_frames, int H, int W, int S, int top_k, int pad_size,
                                                                              int crop_radius, const float *const *score_dev, const int32_t *map_h,
                                                                              const int32_t *map_w, const float *scale_factors,
                                                                              const float *photo_dev, const float *ori_dev, void *const *out,
                                                                              int32_t *counts_out)
{
    try {
        btba_lfnet_params p = btba::lfnetParams();
        p.top_k = top_k; p.pad_size = pad_size; p.crop_radius = crop_radius;
        btba::LfnetBuffers b;
        b.max_heatmaps = static_cast<float *>(out[0]); b.max_scales = static_cast<float *>(out[1]);
        b.kpts_xy = static_cast<int32_t *>(out[2]); b.n_kpts = static_cast<int32_t *>(out[3]);
        b.kpts = static_cast<float *>(out[4]); b.kpts_scale = static_cast<float *>(out[5]);
        b.kpts_ori = static_cast<float *>(out[6]); b.patches = static_cast<float *>(out[7]);
        const std::vector<int> counts = btba::lfnetKeypoints(static_cast<btba_workspace *>(ws), p, n_frames, H, W,
                                                             map_set(S, score_dev, map_h, map_w, scale_factors), photo_dev, ori_dev, b);
        for (int f = 0; f < n_frames; f++) counts_out[f] = counts[f];
        return 0;
    } catch (const btba::Error &e) {
        return e.status;
    }
}

// One square frame through btba::LfnetDetector as a DetectorFeatureManager::DetectFn.  Returns the keypoint count, or -(status).
// desc_out: where the functor's descriptor pointer is copied ([m][P * P] floats = the patches).
extern "C" __attribute__((visibility("default"))) int lfnet_detector_driver(void *ws, int size, int S, int top_k, int pad_size, int crop_radius,
                                                                             const float *const *score_dev, const int32_t *map_h,
                                                                             const int32_t *map_w, const float *scale_factors, const float *gray_dev,
                                                                             const float *ori_dev, void *const *out, float *desc_out, int *dim_out)
{
    try {
        btba_lfnet_params p = btba::lfnetParams();
        p.top_k = top_k; p.pad_size = pad_size; p.crop_radius = crop_radius;
        btba::LfnetBuffers b;
        b.max_heatmaps = static_cast<float *>(out[0]); b.max_scales = static_cast<float *>(out[1]);
        b.kpts_xy = static_cast<int32_t *>(out[2]); b.n_kpts = static_cast<int32_t *>(out[3]);
        b.kpts = static_cast<float *>(out[4]); b.kpts_scale = static_cast<float *>(out[5]);
        b.kpts_ori = static_cast<float *>(out[6]); b.patches = static_cast<float *>(out[7]);
        const btba::LfnetMapSet maps = map_set(S, score_dev, map_h, map_w, scale_factors);
        const int P = p.patch_size;
        btba::DetectorFeatureManager::DetectFn detect = btba::LfnetDetector(
            static_cast<btba_workspace *>(ws),
            [&](const float *, int, const float *&ori) { ori = ori_dev; return maps; },
            [&](const float *patches, int, int &dim) { dim = P * P; return const_cast<float *>(patches); }, p, b);
        const btba::DetectedFeatures f = detect(nullptr, gray_dev, size);
        *dim_out = f.dim;
        if (f.n > 0 && hipMemcpy(desc_out, f.desc_dev, sizeof(float) * (size_t)f.n * f.dim, hipMemcpyDeviceToDevice) != hipSuccess) return -1000;
        return f.kpts_dev == reinterpret_cast<float2 *>(b.kpts) ? f.n : -1001;
    } catch (const btba::Error &e) {
        return -e.status;
    }
}
