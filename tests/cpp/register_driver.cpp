// register_driver.cpp -- ctypes entry into the C++ host layer's btba::registerIndex and btba::registerFrames (tests/test_gpu_register_cpp.py).
// Every map, the model and every output are device pointers; K, the poses and the box are on the host.
#include <vector>

#include "../../bundletrack_amd/cpp/btba_host.hpp"

static btba::ObjectCloudBuffers model(int capacity, void *xyz, void *normal, void *lin, void *n_out)
{
    btba::ObjectCloudBuffers o;
    o.capacity = capacity;
    o.xyz = static_cast<float4 *>(xyz);
    o.normal = static_cast<float4 *>(normal);
    o.lin = static_cast<int32_t *>(lin);
    o.n_out = static_cast<int32_t *>(n_out);
    return o;
}

// one instance: the index of its cloud into cell_index
extern "C" __attribute__((visibility("default"))) int register_driver_index(void *ws, const int32_t *box_host, int capacity, void *lin, void *n_out, void *cell_index)
{
    try {
        btba::registerIndex(static_cast<btba_workspace *>(ws), 1, std::vector<int32_t>(box_host, box_host + 6), model(capacity, nullptr, nullptr, lin, n_out),
                            static_cast<int32_t *>(cell_index));
        return 0;
    } catch (const btba::Error &e) {
        return e.status;
    }
}

// n_frames frames and, with n_points > 0, one point list behind them, all against instance 0
extern "C" __attribute__((visibility("default"))) int register_driver_frames(void *ws, float leaf, int n_iters, int n_frames, int H, int W, const float *K_rowmajor,
                                                                              const float *poses_rowmajor, const void *const *depth, const void *const *normal,
                                                                              const void *points, int64_t n_points, const int32_t *box_host, int capacity, void *xyz,
                                                                              void *nrm, void *cell_index, void *pose_out, void *result, void *trace)
{
    try {
        btba_register_params prm;
        btba_register_params_default(&prm);
        prm.leaf = leaf;
        prm.n_iters = n_iters;
        btba::Matrix3f K;
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) K(r, c) = K_rowmajor[3 * r + c];
        auto pose = [&](int f) {
            btba::Matrix4f T;
            for (int r = 0; r < 4; r++)
                for (int c = 0; c < 4; c++) T(r, c) = poses_rowmajor[16 * f + 4 * r + c];
            return T;
        };
        std::vector<btba_fuse_segment> items;
        for (int f = 0; f < n_frames; f++)
            items.push_back(btba::frameSegment(0, pose(f), static_cast<const float *>(depth[f]), static_cast<const float4 *>(normal[f]), nullptr));
        if (n_points > 0) items.push_back(btba::pointSegment(0, pose(n_frames), static_cast<const float4 *>(points), n_points));
        btba::registerFrames(static_cast<btba_workspace *>(ws), prm, 1, items, H, W, K, std::vector<int32_t>(box_host, box_host + 6),
                             model(capacity, xyz, nrm, nullptr, nullptr), static_cast<const int32_t *>(cell_index), static_cast<float *>(pose_out),
                             static_cast<btba_register_result *>(result), static_cast<btba_register_iter *>(trace));
        return 0;
    } catch (const btba::Error &e) {
        return e.status;
    }
}
