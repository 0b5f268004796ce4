// fusion_driver.cpp -- ctypes entry into the C++ host layer's btba::fuseBounds, btba::fuseFrames and btba::voxelDownsample
// (tests/test_gpu_fusion_cpp.py).  Every map and output is a device pointer; K, the poses and the box are on the host.
#include <vector>

#include "../../bundletrack_amd/cpp/btba_host.hpp"

static btba::ObjectCloudBuffers buffers(int capacity, void *xyz, void *normal, void *colour, void *count, void *lin, void *n_out, void *n_outside, void *status)
{
    btba::ObjectCloudBuffers o;
    o.capacity = capacity;
    o.xyz = static_cast<float4 *>(xyz);
    o.normal = static_cast<float4 *>(normal);
    o.colour = static_cast<uchar4 *>(colour);
    o.count = static_cast<uint32_t *>(count);
    o.lin = static_cast<int32_t *>(lin);
    o.n_out = static_cast<int32_t *>(n_out);
    o.n_outside = static_cast<int32_t *>(n_outside);
    o.status = static_cast<int32_t *>(status);
    return o;
}

// n_frames frames of one instance: mode 0 = fuseBounds into box_dev, mode 1 = fuseFrames with the host box
extern "C" __attribute__((visibility("default"))) int fusion_driver_frames(void *ws, int mode, float leaf, int n_frames, int H, int W, const float *K_rowmajor,
                                                                            const float *poses_rowmajor, const void *const *depth, const void *const *normal,
                                                                            const void *const *colour, int32_t *box_dev, const int32_t *box_host, int capacity,
                                                                            void *xyz, void *nrm, void *col, void *count, void *lin, void *n_out, void *n_outside,
                                                                            void *status)
{
    try {
        btba_fuse_params prm;
        btba_fuse_params_default(&prm);
        prm.leaf = leaf;
        btba::Matrix3f K;
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) K(r, c) = K_rowmajor[3 * r + c];
        std::vector<btba_fuse_segment> segs;
        for (int f = 0; f < n_frames; f++) {
            btba::Matrix4f T;
            for (int r = 0; r < 4; r++)
                for (int c = 0; c < 4; c++) T(r, c) = poses_rowmajor[16 * f + 4 * r + c];
            segs.push_back(btba::frameSegment(0, T, static_cast<const float *>(depth[f]), static_cast<const float4 *>(normal[f]),
                                              colour ? static_cast<const uchar4 *>(colour[f]) : nullptr));
        }
        if (mode == 0) btba::fuseBounds(static_cast<btba_workspace *>(ws), prm, 1, segs, H, W, K, box_dev);
        else btba::fuseFrames(static_cast<btba_workspace *>(ws), prm, 1, segs, H, W, K, std::vector<int32_t>(box_host, box_host + 6),
                              buffers(capacity, xyz, nrm, col, count, lin, n_out, n_outside, status));
        return 0;
    } catch (const btba::Error &e) {
        return e.status;
    }
}

extern "C" __attribute__((visibility("default"))) int fusion_driver_downsample(void *ws, float leaf, const void *xyz_in, int64_t n, const int32_t *box_host,
                                                                                int capacity, void *xyz, void *count, void *lin, void *n_out, void *n_outside,
                                                                                void *status)
{
    try {
        btba_fuse_params prm;
        btba_fuse_params_default(&prm);
        prm.leaf = leaf;
        btba::voxelDownsample(static_cast<btba_workspace *>(ws), prm, { static_cast<const float4 *>(xyz_in) }, { n }, std::vector<int32_t>(box_host, box_host + 6),
                              buffers(capacity, xyz, nullptr, nullptr, count, lin, n_out, n_outside, status));
        return 0;
    } catch (const btba::Error &e) {
        return e.status;
    }
}
