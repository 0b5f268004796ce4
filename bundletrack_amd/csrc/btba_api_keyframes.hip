// btba_api_keyframes.hip -- host side of libbtba.so: the device keyframe memory (btba_keyframes.hpp) and btba_rotation_distances.
#include "btba_host_common.hpp"
#include "btba_keyframes.hpp"

struct btba_keyframes {
    btba_workspace *ws = nullptr;
    int device = 0;                        // the workspace's device: destroy does not touch the workspace (it may be gone already)
    int n_sessions = 0, capacity = 0, max_BA = 0;
    KeyframesPool L;
    KeyframesLds lds;
    DevBuf pool;
};

namespace {

KfPool kf_view(const btba_keyframes *kf)
{
    unsigned char *base = kf->pool.as<unsigned char>();
    KfPool P{};
    P.poses = reinterpret_cast<float *>(base + kf->L.poses);
    P.frame_id = reinterpret_cast<int32_t *>(base + kf->L.frame_id);
    P.frame_key = reinterpret_cast<uint64_t *>(base + kf->L.frame_key);
    P.count = reinterpret_cast<int32_t *>(base + kf->L.count);
    P.overflow = reinterpret_cast<int32_t *>(base + kf->L.overflow);
    P.capacity = kf->capacity;
    P.n_sessions = kf->n_sessions;
    return P;
}

}  // namespace

extern "C" {

int btba_keyframes_create(btba_workspace *ws, int n_sessions, int capacity, int max_BA_frames, btba_keyframes **out)
{
    if (!out) return BTBA_EINVAL;
    *out = nullptr;
    KeyframesPool L;
    KeyframesLds lds;
    // every size is checked before the first HIP call: a (capacity, max_BA_frames) outside the limits is refused, never truncated
    if (!ws || !keyframes_pool_layout(n_sessions, capacity, &L) || !keyframes_lds_layout(capacity, max_BA_frames, &lds)) return BTBA_EINVAL;
    DeviceGuard device_guard(ws);
    btba_keyframes *kf = new (std::nothrow) btba_keyframes;
    if (!kf) return BTBA_ENOMEM;
    kf->ws = ws;
    kf->device = ws->device;
    kf->n_sessions = n_sessions;
    kf->capacity = capacity;
    kf->max_BA = max_BA_frames;
    kf->L = L;
    kf->lds = lds;
    if (int rc = kf->pool.ensure(L.total)) { delete kf; return rc; }
    hipError_t e = hipMemsetAsync(kf->pool.p, 0, L.total, ws->stream);
    if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_keyframes_select), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kKfLdsLimit);
    if (e != hipSuccess) { g_last_hip_error = (int)e; (void)hipStreamSynchronize(ws->stream); delete kf; return BTBA_EHIP; }
    *out = kf;
    return BTBA_OK;
}

void btba_keyframes_destroy(btba_keyframes *kf) { destroy_on_device(kf); }

int btba_keyframes_reset(btba_keyframes *kf, int session)
{
    if (!kf || session < -1 || session >= kf->n_sessions) return BTBA_EINVAL;
    DeviceGuard device_guard(kf->ws);
    const KfPool P = kf_view(kf);
    const size_t first = session < 0 ? 0 : (size_t)session, n = session < 0 ? (size_t)kf->n_sessions : 1;
    HIP_TRY(hipMemsetAsync(P.count + first, 0, sizeof(int32_t) * n, kf->ws->stream));
    HIP_TRY(hipMemsetAsync(P.overflow + first, 0, sizeof(int32_t) * n, kf->ws->stream));
    return BTBA_OK;
}

int btba_keyframes_check_add(btba_keyframes *kf, float min_rot_deg, int min_feat_num, const int32_t *active_dev, const float *pose_dev,
                             const int32_t *frame_id_dev, const uint64_t *frame_key_dev, const int32_t *status_other_dev, const int32_t *n_keypts_dev,
                             int32_t *added_out_dev)
{
    if (!kf || !pose_dev || !frame_id_dev || !status_other_dev || !n_keypts_dev || !added_out_dev || min_rot_deg != min_rot_deg) return BTBA_EINVAL;
    if (misaligned(active_dev, 4) || misaligned(pose_dev, 4) || misaligned(frame_id_dev, 4) || misaligned(frame_key_dev, 8) || misaligned(status_other_dev, 4) ||
        misaligned(n_keypts_dev, 4) || misaligned(added_out_dev, 4))
        return BTBA_EINVAL;
    DeviceGuard device_guard(kf->ws);
    k_keyframes_check_add<<<kf->n_sessions, 64, 0, kf->ws->stream>>>(kf_view(kf), min_rot_deg, min_feat_num, active_dev, pose_dev, frame_id_dev, frame_key_dev,
                                                                     status_other_dev, n_keypts_dev, added_out_dev);
    HIP_TRY(hipGetLastError());
    return BTBA_OK;
}

int btba_keyframes_select(btba_keyframes *kf, const int32_t *active_dev, const float *newpose_dev, const int32_t *new_frame_id_dev,
                          const uint64_t *new_frame_key_dev, int32_t *n_window_out, int32_t *window_slot_out, int32_t *window_frame_id_out,
                          uint64_t *window_frame_key_out, float *window_pose_out, int32_t *newframe_index_out)
{
    if (!kf || !newpose_dev || !new_frame_id_dev || !n_window_out || !window_slot_out || !window_frame_id_out || !window_frame_key_out || !window_pose_out ||
        !newframe_index_out)
        return BTBA_EINVAL;
    if (misaligned(active_dev, 4) || misaligned(newpose_dev, 4) || misaligned(new_frame_id_dev, 4) || misaligned(new_frame_key_dev, 8) || misaligned(n_window_out, 4) ||
        misaligned(window_slot_out, 4) || misaligned(window_frame_id_out, 4) || misaligned(window_frame_key_out, 8) || misaligned(window_pose_out, 4) ||
        misaligned(newframe_index_out, 4))
        return BTBA_EINVAL;
    DeviceGuard device_guard(kf->ws);
    const KfSelectOut O{ n_window_out, window_slot_out, window_frame_id_out, window_frame_key_out, window_pose_out, newframe_index_out };
    k_keyframes_select<<<kf->n_sessions, kKfSelectThreads, kf->lds.total, kf->ws->stream>>>(kf_view(kf), kf->max_BA, kf->lds, active_dev, newpose_dev,
                                                                                          new_frame_id_dev, new_frame_key_dev, O);
    HIP_TRY(hipGetLastError());
    return BTBA_OK;
}

int btba_keyframes_writeback(btba_keyframes *kf, const int32_t *active_dev, const int32_t *n_window_dev, const int32_t *window_slot_dev, const float *pose_dev)
{
    if (!kf || !n_window_dev || !window_slot_dev || !pose_dev || misaligned(active_dev, 4) || misaligned(n_window_dev, 4) || misaligned(window_slot_dev, 4) ||
        misaligned(pose_dev, 4))
        return BTBA_EINVAL;
    DeviceGuard device_guard(kf->ws);
    k_keyframes_writeback<<<kf->n_sessions, 256, 0, kf->ws->stream>>>(kf_view(kf), kf->max_BA, active_dev, n_window_dev, window_slot_dev, pose_dev);
    HIP_TRY(hipGetLastError());
    return BTBA_OK;
}

int btba_keyframes_export(btba_keyframes *kf, int32_t *count_out, int32_t *overflow_out, int32_t *frame_id_out, uint64_t *frame_key_out, float *pose_out)
{
    if (!kf) return BTBA_EINVAL;
    DeviceGuard device_guard(kf->ws);
    const KfPool P = kf_view(kf);
    hipStream_t st = kf->ws->stream;
    const size_t S = (size_t)kf->n_sessions, SC = S * (size_t)kf->capacity;
    if (count_out) HIP_TRY(hipMemcpyAsync(count_out, P.count, sizeof(int32_t) * S, hipMemcpyDeviceToHost, st));
    if (overflow_out) HIP_TRY(hipMemcpyAsync(overflow_out, P.overflow, sizeof(int32_t) * S, hipMemcpyDeviceToHost, st));
    if (frame_id_out) HIP_TRY(hipMemcpyAsync(frame_id_out, P.frame_id, sizeof(int32_t) * SC, hipMemcpyDeviceToHost, st));
    if (frame_key_out) HIP_TRY(hipMemcpyAsync(frame_key_out, P.frame_key, sizeof(uint64_t) * SC, hipMemcpyDeviceToHost, st));
    if (pose_out) HIP_TRY(hipMemcpyAsync(pose_out, P.poses, sizeof(float) * 16 * SC, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return BTBA_OK;
}

int btba_rotation_distances(btba_workspace *ws, int n, const float *A_dev, const float *B_dev, float *dist_out_dev)
{
    if (!ws || n < 0 || n > (1 << 27) || (n > 0 && (!A_dev || !B_dev || !dist_out_dev)) || misaligned(A_dev, 4) || misaligned(B_dev, 4) || misaligned(dist_out_dev, 4))
        return BTBA_EINVAL;
    if (n == 0) return BTBA_OK;
    DeviceGuard device_guard(ws);
    k_rotation_distances<<<(n + 255) / 256, 256, 0, ws->stream>>>(n, A_dev, B_dev, dist_out_dev);
    HIP_TRY(hipGetLastError());
    return BTBA_OK;
}

}  // extern "C"
