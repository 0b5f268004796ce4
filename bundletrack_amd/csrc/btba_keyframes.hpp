// btba_keyframes.hpp -- kernels of the device keyframe memory (btba_keyframes_*, include/btba.h): Bundler::checkAndAddKeyframe and
// Bundler::selectKeyFramesForBA (Bundler.cpp:185-274) for many tracking sessions at once.  The distance is btba_keyframes_point.hpp's, the
// pool and the LDS are btba_keyframes_layout.hpp's.  No atomics: a session's state is written by one wave (check_add) or read by one
// workgroup (select), so the bytes of a session depend on that session alone.
#pragma once
#include <hip/hip_runtime.h>
#include <cfloat>
#include <climits>
#include <cstdint>
#include "btba_keyframes_layout.hpp"
#include "btba_keyframes_point.hpp"

namespace btba {

struct KfPool {
    float *poses;
    int32_t *frame_id;
    uint64_t *frame_key;
    int32_t *count, *overflow;
    int capacity, n_sessions;
};

struct KfSelectOut {
    int32_t *n_window, *window_slot, *window_frame_id;
    uint64_t *window_frame_key;
    float *window_pose;
    int32_t *newframe_index;
};

__device__ __forceinline__ bool kf_active(const int32_t *active, int s) { return !active || active[s] != 0; }
__device__ __forceinline__ int kf_count(const KfPool &P, int s) { return min(max(P.count[s], 0), P.capacity); }

__global__ void k_rotation_distances(int n, const float *A, const float *B, float *out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = keyframes_distance(A + 16 * i, B + 16 * i);
}

// checkAndAddKeyframe (Bundler.cpp:185-219), one frame per session: one wave per session, lanes over the pool, one ballot.
__global__ __launch_bounds__(64) void k_keyframes_check_add(KfPool P, float min_rot_deg, int min_feat_num, const int32_t *active, const float *pose,
                                                            const int32_t *frame_id, const uint64_t *frame_key, const int32_t *status_other,
                                                            const int32_t *n_keypts, int32_t *added_out)
{
    const int s = blockIdx.x, lane = threadIdx.x;
    if (s >= P.n_sessions || !kf_active(active, s)) return;
    const int C = P.capacity, count = kf_count(P, s);
    float *pool = P.poses + 16 * ((size_t)s * C);
    float T[12];
    for (int k = 0; k < 12; k++) T[k] = pose[16 * (size_t)s + k];
    bool join = frame_id[s] == 0;                                                          // :187-191
    if (!join && status_other[s] != 0 && n_keypts[s] >= min_feat_num) {                    // :192, :199-202
        bool near = false;
        for (int c = lane; c < count; c += 64)                                             // :204-215
            near |= keyframes_degrees(keyframes_distance(T, pool + 16 * (size_t)c)) < min_rot_deg;
        join = __ballot(near) == 0ull;
    }
    int added = 0;
    if (join && count >= C) {
        added = -1;
        if (lane == 0) P.overflow[s] += 1;
    } else if (join) {
        added = 1;
        if (lane < 16) pool[16 * (size_t)count + lane] = pose[16 * (size_t)s + lane];
        if (lane == 0) {
            P.frame_id[(size_t)s * C + count] = frame_id[s];
            P.frame_key[(size_t)s * C + count] = frame_key ? frame_key[s] : 0ull;
            P.count[s] = count + 1;
        }
    }
    if (lane == 0) added_out[s] = added;
}

// (cum, slot) lexicographic minimum: strict `<` on cum, the lowest pool slot on ties (Bundler.cpp:257 walks the pool in order)
__device__ __forceinline__ void kf_take_less(float &cum, int &slot, float ocum, int oslot)
{
    if (ocum < cum || (ocum == cum && oslot < slot)) { cum = ocum; slot = oslot; }
}

// selectKeyFramesForBA (Bundler.cpp:222-274, "greedy_rot") and optimizeGPU's sort by id and pose gather (:286, :334-341): one workgroup per
// session.  A member's distances to every pool slot are computed once, when it joins (one column of the table); a round re-sums each
// candidate's row in the current summation order -- members' slots ascending, the new frame last -- and reduces (cum, slot) across lanes
// and waves.  Rows of the window at and past n_window keep their bytes.
__global__ __launch_bounds__(kKfSelectThreads) void k_keyframes_select(KfPool P, int max_BA, KeyframesLds L, const int32_t *active, const float *newpose,
                                                                       const int32_t *new_frame_id, const uint64_t *new_frame_key, KfSelectOut O)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char kf_lds[];
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (s >= P.n_sessions || !kf_active(active, s)) return;                                // uniform over the workgroup
    float *table = reinterpret_cast<float *>(kf_lds + L.table);                            // column j at table + j * C
    int32_t *member = reinterpret_cast<int32_t *>(kf_lds + L.member);
    int32_t *order = reinterpret_cast<int32_t *>(kf_lds + L.order);
    float *red_cum = reinterpret_cast<float *>(kf_lds + L.red_cum);
    int32_t *red_slot = reinterpret_cast<int32_t *>(kf_lds + L.red_slot);
    int32_t *pick = reinterpret_cast<int32_t *>(kf_lds + L.pick);
    const int C = P.capacity, count = kf_count(P, s);
    const float *pool = P.poses + 16 * ((size_t)s * C);
    const float *fresh = newpose + 16 * (size_t)s;
    int n;
    if (count + 1 <= max_BA) {                                                             // :227-235: the pool fits
        n = count + 1;
        for (int j = tid; j < n; j += kKfSelectThreads) member[j] = j < count ? j : -1;
    } else {
        if (tid == 0) { member[0] = -1; member[1] = 0; order[0] = 1; order[1] = 0; }       // the new frame (:224), keyframe 0 (:237)
        for (int c = tid; c < count; c += kKfSelectThreads) {
            table[c] = keyframes_distance(pool + 16 * (size_t)c, fresh);
            table[C + c] = keyframes_distance(pool + 16 * (size_t)c, pool);
        }
        n = 2;
        __syncthreads();
        while (n < max_BA) {                                                               // :243
            float best = FLT_MAX;
            int best_slot = INT_MAX;
            for (int c = tid; c < count; c += kKfSelectThreads) {
                bool chosen = false;
                for (int j = 1; j < n; j++) chosen |= member[j] == c;                      // :250
                if (chosen) continue;
                float cum = 0.0f;
                for (int k = 0; k < n; k++) cum += table[order[k] * C + c];                // :252-256
                if (cum < best) { best = cum; best_slot = c; }                             // :257-261 (c ascends: the lowest slot stays)
            }
            for (int o = 32; o > 0; o >>= 1) kf_take_less(best, best_slot, __shfl_xor(best, o), __shfl_xor(best_slot, o));
            if (lane == 0) { red_cum[wave] = best; red_slot[wave] = best_slot; }
            __syncthreads();
            if (tid == 0) {
                for (int w = 1; w < kKfSelectWaves; w++) kf_take_less(best, best_slot, red_cum[w], red_slot[w]);
                pick[0] = best_slot;
                if (best_slot != INT_MAX) {                                                // :263: column n joins the summation order by its slot
                    member[n] = best_slot;
                    int q = 0;
                    while (q < n - 1 && member[order[q]] < best_slot) q++;
                    for (int k = n; k > q; k--) order[k] = order[k - 1];
                    order[q] = n;
                }
            }
            __syncthreads();
            const int p = pick[0];
            if (p == INT_MAX) break;                                                       // no candidate below FLT_MAX: the set stops growing
            for (int c = tid; c < count; c += kKfSelectThreads) table[n * C + c] = keyframes_distance(pool + 16 * (size_t)c, pool + 16 * (size_t)p);
            n++;
            __syncthreads();
        }
    }
    __syncthreads();
    // :286: rows by frame id (a pool slot before the new frame on equal ids, lower slots first); order[] becomes each member's row
    const int nid = new_frame_id[s];
    if (tid < n) {
        const int mi = member[tid];
        const int id_i = mi < 0 ? nid : P.frame_id[(size_t)s * C + mi], tie_i = mi < 0 ? INT_MAX : mi;
        int rank = 0;
        for (int j = 0; j < n; j++) {
            const int mj = member[j];
            const int id_j = mj < 0 ? nid : P.frame_id[(size_t)s * C + mj], tie_j = mj < 0 ? INT_MAX : mj;
            rank += id_j < id_i || (id_j == id_i && tie_j < tie_i);
        }
        const size_t row = (size_t)s * max_BA + rank;
        O.window_slot[row] = mi;
        O.window_frame_id[row] = id_i;
        O.window_frame_key[row] = mi < 0 ? (new_frame_key ? new_frame_key[s] : 0ull) : P.frame_key[(size_t)s * C + mi];
        if (mi < 0) O.newframe_index[s] = rank;
        order[tid] = rank;
    }
    if (tid == 0) O.n_window[s] = n;
    __syncthreads();
    for (int e = tid; e < n * 16; e += kKfSelectThreads) {                                 // :334-341
        const int i = e >> 4, k = e & 15, mi = member[i];
        O.window_pose[((size_t)s * max_BA + order[i]) * 16 + k] = mi < 0 ? fresh[k] : pool[16 * (size_t)mi + k];
    }
}

// Bundler.cpp:353-357: the solved poses of the window's keyframes back into the pool.  The new frame's row (slot -1) is not a pool member.
__global__ void k_keyframes_writeback(KfPool P, int max_BA, const int32_t *active, const int32_t *n_window, const int32_t *window_slot, const float *pose)
{
    const int s = blockIdx.x;
    if (s >= P.n_sessions || !kf_active(active, s)) return;
    const int C = P.capacity, count = kf_count(P, s), n = min(max(n_window[s], 0), max_BA);
    for (int e = threadIdx.x; e < n * 16; e += blockDim.x) {
        const int row = e >> 4, k = e & 15, slot = window_slot[(size_t)s * max_BA + row];
        if (slot >= 0 && slot < count) P.poses[((size_t)s * C + slot) * 16 + k] = pose[((size_t)s * max_BA + row) * 16 + k];
    }
}

}  // namespace btba
