// btba_keyframes_layout.hpp -- pool records and the select kernel's LDS layout of the device keyframe memory (btba_keyframes_*,
// include/btba.h).  No HIP: the kernels (btba_keyframes.hpp) index with it, the host (btba_api_keyframes.hip) sizes with it, and
// tests/cpp/keyframes_host.cpp walks it under the host sanitizers.
//
// The pool of S sessions with room for C keyframes each, one device block, every region a multiple of 256 bytes:
//   poses      float  [S][C][16]   row-major 4 x 4 camera -> model, slot k = the k-th keyframe that joined
//   frame_id   int32  [S][C]
//   frame_key  uint64 [S][C]       the caller's cache key of the frame (btba_optimize_frames_keyed)
//   count      int32  [S]          keyframes in the pool
//   overflow   int32  [S]          frames that should have joined a full pool
//
// The select kernel, one workgroup of kKfSelectThreads per session, in dynamic LDS (every region a multiple of 16 bytes):
//   table      float  [max_BA][C]  table[j][c]: distance of pool slot c to the j-th member that joined the chosen set (j = 0: the new frame);
//                                  C * max_BA floats, member-major so that a wave's lanes (consecutive c) read consecutive banks at any max_BA
//   member     int32  [max_BA]     the members in joining order: a pool slot, or -1 for the new frame
//   order      int32  [max_BA]     the columns in summation order: members' slots ascending, the new frame last
//   red_cum    float  [waves], red_slot int32 [waves], pick int32 [4]: the reduction across waves and the round's pick
#pragma once
#include <cstddef>
#include <cstdint>

namespace btba {

constexpr int kKfMinBA = 2, kKfMaxBA = 85;                       // max_BA_frames the solve serves
constexpr int kKfSelectThreads = 256, kKfSelectWaves = kKfSelectThreads / 64;
constexpr size_t kKfLdsLimit = 160 * 1024;                        // the select kernel's dynamic LDS: about 1024 keyframes at max_BA_frames <= 32
constexpr int64_t kKfMaxSlots = (int64_t)1 << 24;                 // S * C: 1 GiB of poses, and every element index fits an int32

struct KeyframesPool {
    size_t poses = 0, frame_id = 0, frame_key = 0, count = 0, overflow = 0, total = 0;      // byte offsets, each a multiple of 256
};
struct KeyframesLds {
    size_t table = 0, member = 0, order = 0, red_cum = 0, red_slot = 0, pick = 0, total = 0;      // byte offsets, each a multiple of 16
};

// false: a size outside the limits (nothing is ever truncated to fit)
inline bool keyframes_lds_layout(int capacity, int max_BA, KeyframesLds *L)
{
    if (capacity < 1 || max_BA < kKfMinBA || max_BA > kKfMaxBA) return false;
    auto up = [](size_t x) { return (x + 15) & ~(size_t)15; };
    KeyframesLds l;
    l.table = 0;
    l.member = up(sizeof(float) * (size_t)capacity * (size_t)max_BA);
    l.order = l.member + up(sizeof(int32_t) * (size_t)max_BA);
    l.red_cum = l.order + up(sizeof(int32_t) * (size_t)max_BA);
    l.red_slot = l.red_cum + up(sizeof(float) * kKfSelectWaves);
    l.pick = l.red_slot + up(sizeof(int32_t) * kKfSelectWaves);
    l.total = l.pick + up(sizeof(int32_t) * 4);
    if (l.total > kKfLdsLimit) return false;
    if (L) *L = l;
    return true;
}

inline bool keyframes_pool_layout(int n_sessions, int capacity, KeyframesPool *L)
{
    if (n_sessions < 1 || capacity < 1 || (int64_t)n_sessions * capacity > kKfMaxSlots) return false;
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t S = (size_t)n_sessions, SC = S * (size_t)capacity;
    KeyframesPool l;
    l.poses = 0;
    l.frame_id = up(sizeof(float) * 16 * SC);
    l.frame_key = l.frame_id + up(sizeof(int32_t) * SC);
    l.count = l.frame_key + up(sizeof(uint64_t) * SC);
    l.overflow = l.count + up(sizeof(int32_t) * S);
    l.total = l.overflow + up(sizeof(int32_t) * S);
    if (L) *L = l;
    return true;
}

}  // namespace btba
