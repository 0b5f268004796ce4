// keyframes_driver.cpp -- ctypes entry into the C++ host layer's btba::DeviceKeyframeMemory (tests/test_gpu_keyframes_cpp.py).  Every per-session
// array and every output is a device pointer.  One memory lives between the calls: create, then add / select / writeback / export, then destroy.
#include <cstring>
#include <memory>

#include "../../bundletrack_amd/cpp/btba_host.hpp"

static std::unique_ptr<btba::DeviceKeyframeMemory> g_mem;

#define DRIVER_API extern "C" __attribute__((visibility("default")))

DRIVER_API int keyframes_driver_create(void *ws, int n_sessions, int capacity, int max_BA, float min_rot_deg, int min_feat_num)
{
    try {
        g_mem.reset();
        g_mem = std::make_unique<btba::DeviceKeyframeMemory>(static_cast<btba_workspace *>(ws), n_sessions, capacity, max_BA, min_rot_deg, min_feat_num);
        return 0;
    } catch (const btba::Error &e) {
        return e.status;
    }
}

DRIVER_API void keyframes_driver_destroy() { g_mem.reset(); }

DRIVER_API int keyframes_driver_add(const void *active, const void *pose, const void *frame_id, const void *frame_key, const void *status_other, const void *n_keypts,
                                    void *added_out)
{
    try {
        g_mem->checkAndAddKeyframes(static_cast<const float *>(pose), static_cast<const int32_t *>(frame_id), static_cast<const uint64_t *>(frame_key),
                                    static_cast<const int32_t *>(status_other), static_cast<const int32_t *>(n_keypts), static_cast<int32_t *>(added_out),
                                    static_cast<const int32_t *>(active));
        return 0;
    } catch (const btba::Error &e) {
        return e.status;
    }
}

DRIVER_API int keyframes_driver_select(const void *newpose, const void *new_id, const void *new_key, void *n_window, void *slot, void *frame_id, void *frame_key,
                                       void *pose, void *newframe_index)
{
    try {
        btba::KeyframeWindows w;
        w.n_window = static_cast<int32_t *>(n_window);
        w.slot = static_cast<int32_t *>(slot);
        w.frame_id = static_cast<int32_t *>(frame_id);
        w.frame_key = static_cast<uint64_t *>(frame_key);
        w.pose = static_cast<float *>(pose);
        w.newframe_index = static_cast<int32_t *>(newframe_index);
        g_mem->selectKeyFramesForBA(static_cast<const float *>(newpose), static_cast<const int32_t *>(new_id), static_cast<const uint64_t *>(new_key), w);
        return 0;
    } catch (const btba::Error &e) {
        return e.status;
    }
}

DRIVER_API int keyframes_driver_writeback(const void *n_window, const void *slot, const void *pose)
{
    try {
        g_mem->writeback(static_cast<const int32_t *>(n_window), static_cast<const int32_t *>(slot), static_cast<const float *>(pose));
        return 0;
    } catch (const btba::Error &e) {
        return e.status;
    }
}

// host outputs: count, overflow [S]; frame_id [S][C]; frame_key [S][C]; poses [S][C][16]
DRIVER_API int keyframes_driver_export(int32_t *count, int32_t *overflow, int32_t *frame_id, uint64_t *frame_key, float *poses)
{
    try {
        const btba::KeyframePools p = g_mem->exportPools();
        std::memcpy(count, p.count.data(), sizeof(int32_t) * p.count.size());
        std::memcpy(overflow, p.overflow.data(), sizeof(int32_t) * p.overflow.size());
        std::memcpy(frame_id, p.frame_id.data(), sizeof(int32_t) * p.frame_id.size());
        std::memcpy(frame_key, p.frame_key.data(), sizeof(uint64_t) * p.frame_key.size());
        std::memcpy(poses, p.poses.data(), sizeof(float) * p.poses.size());
        return 0;
    } catch (const btba::Error &e) {
        return e.status;
    }
}

DRIVER_API int keyframes_driver_distances(void *ws, int n, const void *A, const void *B, void *out)
{
    try {
        btba::rotationDistances(static_cast<btba_workspace *>(ws), n, static_cast<const float *>(A), static_cast<const float *>(B), static_cast<float *>(out));
        return 0;
    } catch (const btba::Error &e) {
        return e.status;
    }
}

// The host memory btba::KeyframeMemory on the same poses, timed (scripts/keyframes_timing.py): a pool of n_pool keyframes (poses [n_pool + 1][16]
// row-major, the last one the new frame), `reps` calls each of selectKeyFramesForBA and of a checkAndAddKeyframe that scans the whole pool and
// joins (taken out again); ms_out[2 * reps]: the selects' times, then the adds'.  CPU only.
#include <chrono>

DRIVER_API int keyframes_driver_host_loop(const float *poses, int n_pool, int max_BA, int reps, double *ms_out)
{
    using clock = std::chrono::steady_clock;
    auto yml = std::make_shared<btba::Config>();
    yml->max_BA_frames = max_BA;
    yml->keyframe_min_rot = 0.0f;
    btba::KeyframeMemory mem(yml);
    auto frame = [&](int k) {
        auto fr = std::make_shared<btba::Frame>();
        fr->_id = k;
        fr->_n_keypts = 100;
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) fr->_pose_in_model(r, c) = poses[16 * (size_t)k + 4 * r + c];
        return fr;
    };
    for (int k = 0; k < n_pool; k++)
        if (!mem.checkAndAddKeyframe(frame(k))) return 1;
    const auto fresh = frame(n_pool);
    for (int r = 0; r < reps; r++) {
        const auto t0 = clock::now();
        const auto chosen = mem.selectKeyFramesForBA(fresh);
        ms_out[r] = std::chrono::duration<double, std::milli>(clock::now() - t0).count();
        if (chosen.empty()) return 2;
    }
    for (int r = 0; r < reps; r++) {
        const auto t0 = clock::now();
        const bool added = mem.checkAndAddKeyframe(fresh);
        ms_out[reps + r] = std::chrono::duration<double, std::milli>(clock::now() - t0).count();
        if (!added) return 3;
        mem._keyframes.pop_back();
    }
    return 0;
}
