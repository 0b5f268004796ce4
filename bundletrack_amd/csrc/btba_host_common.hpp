// btba_host_common.hpp -- what every host unit of libbtba.so (btba_api*.hip) needs: the HIP error slot, the self-freeing buffers,
// the scratch carver, the workspace and its device guard.  Internal: nothing here is exported.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <new>
#include <string>
#include <map>
#include <memory>
#include <utility>
#include <vector>

#include "../../include/btba.h"
#include "btba_device.hpp"
#include "btba_lfnet_weights.hpp"

// The types below are members of btba_workspace, which every unit sees: a named namespace, hidden, instead of an anonymous one per unit.
namespace btba_host __attribute__((visibility("hidden"))) {

extern thread_local int g_last_hip_error;      // defined in btba_api.hip: btba_last_hip_error() reports an error raised in any unit

// Growable device memory that frees itself.  Move-only: a copy would be a second owner of p.
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept
    {
        if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    ~DevBuf() { release(); }
    int ensure(size_t bytes)
    {
        if (bytes <= cap) return BTBA_OK;
        if (p) { hipError_t e = hipFree(p); p = nullptr; cap = 0; if (e != hipSuccess) { g_last_hip_error = (int)e; return BTBA_EHIP; } }
        size_t want = bytes + bytes / 4 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) { g_last_hip_error = (int)e; p = nullptr; return e == hipErrorOutOfMemory ? BTBA_ENOMEM : BTBA_EHIP; }
        cap = want;
        return BTBA_OK;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    template <class T> T *as() const { return reinterpret_cast<T *>(p); }
};

// Growable pinned host memory that frees itself.  `want` is the capacity allocated when the block has to grow.
struct PinBuf {
    void *p = nullptr;
    size_t cap = 0;
    PinBuf() = default;
    PinBuf(const PinBuf &) = delete;
    PinBuf &operator=(const PinBuf &) = delete;
    ~PinBuf() { if (p) (void)hipHostFree(p); }
    int ensure(size_t bytes, size_t want = 0)
    {
        if (bytes <= cap) return BTBA_OK;
        if (p) { (void)hipHostFree(p); p = nullptr; cap = 0; }
        if (!want) want = bytes + bytes / 2 + 4096;
        hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
        if (e != hipSuccess) { g_last_hip_error = (int)e; p = nullptr; return e == hipErrorOutOfMemory ? BTBA_ENOMEM : BTBA_EHIP; }
        cap = want;
        return BTBA_OK;
    }
};

// The layout of one call's scratch in a DevBuf.  Regions are added in order; a present region takes its bytes rounded up to
// 256, an absent one takes none and reads as nullptr.  After bind() a region converts to its typed device pointer.
struct Scratch {
    size_t bytes = 0;
    unsigned char *base = nullptr;
    template <class T> struct Region {
        const Scratch *s; size_t off; bool present;
        operator T *() const { return present ? reinterpret_cast<T *>(s->base + off) : nullptr; }
    };
    template <class T> Region<T> add(size_t count, bool present = true)
    {
        Region<T> r{ this, bytes, present };
        if (present) bytes += (sizeof(T) * count + 255) & ~(size_t)255;
        return r;
    }
    int bind(DevBuf &buf, size_t floor = 0) { int rc = buf.ensure(bytes > floor ? bytes : floor); base = buf.as<unsigned char>(); return rc; }
};

inline bool misaligned(const void *q, size_t a) { return (reinterpret_cast<uintptr_t>(q) & (a - 1)) != 0; }

struct EventPair { hipEvent_t a, b; int kind; };   // kind 0 dense, 1 sparse, 2 system, 3 solve region, 4 cache

}  // namespace btba_host

#define HIP_TRY(expr)                                   \
    do {                                                \
        hipError_t e_ = (expr);                         \
        if (e_ != hipSuccess) {                         \
            btba_host::g_last_hip_error = (int)e_;      \
            return BTBA_EHIP;                           \
        }                                               \
    } while (0)

using namespace btba;
using namespace btba_host;

struct btba_workspace {
    hipStream_t stream = nullptr;
    bool owns_stream = false;
    int device = 0;
    DevBuf x, T, Tinv, sparse_part, dense_part, pairsum, dense_pairs, ptrs, big_A, solve_tab;
    DevBuf corr, offsets, poses, campos, normals, nvalid;   // optimize_frames staging
    DevBuf valid_lists, valid_counts;                       // per-frame lists of pixels with a depth (compact cache)
    DevBuf block_ranges;                                    // per (frame, 8 x 8 block) usable depth range: dead-block test of the dense sweep
    DevBuf corr24_tmp;                                      // re-layout of a call's EntryJ array written by its first iteration's sparse sweep (BTBA_OPT_RELAYOUT)
    DevBuf live_blocks;                                     // BTBA_OPT_COUNT_LIVE: one uint64 the block-walk workgroups add their walked blocks to
    bool count_live = false;
    // Developer / tuning switches.  Read from the environment ONCE, when the workspace is created (never on the solve path), and settable
    // per workspace through btba_workspace_set_option (include/btba.h: BTBA_OPT_*).  None of them changes what is computed.
    struct Tuning {
        bool dense_order = true;       // BTBA_OPT_DENSE_ORDER   (env BTBA_NO_DENSE_ORDER=1 turns it off): dense pairs worked off heaviest first
        bool tile_major = true;        // BTBA_OPT_TILE_MAJOR    (env BTBA_PAIR_MAJOR=1 turns it off): (band, pair) instead of (pair, band) work order
        bool block_walk = true;        // BTBA_OPT_BLOCK_WALK    (env BTBA_NO_BLOCK_WALK=1): waves walk 8 x 8 blocks instead of 64 x 1 strips
        bool block_skip = true;        // BTBA_OPT_BLOCK_SKIP    (env BTBA_NO_BLOCK_SKIP=1): provably dead blocks are not walked
        int sparse_tail_256 = -1;      // BTBA_OPT_SPARSE_TAIL   (env BTBA_SPARSE_TAIL): share (x / 256) of the sparse items that close the fused launch; -1 = the library's choice
        bool big_assembly = true;      // BTBA_OPT_BIG_ASSEMBLY  (env BTBA_NO_BIG_ASSEMBLY=1): many-workgroup reduction / assembly from 24 frames on
        int overlap_groups = 2;        // BTBA_OPT_OVERLAP_GROUPS (env BTBA_GROUPS): instance groups of BTBA_FLAG_OVERLAP
        bool overlap_equal_prio = false;   // BTBA_OPT_OVERLAP_EQUAL_PRIO (env BTBA_GROUP_PRIO=e...)
        size_t keyed_corr_min_bytes = (size_t)1 << 20;   // BTBA_OPT_KEYED_CORR_MIN_BYTES (env of the same name): below it the keyed correspondence cache is not used
        int corr_nt = -1;              // BTBA_OPT_CORR_NONTEMPORAL (env BTBA_CORR_NT): non-temporal correspondence loads  1 always, 0 never, -1 (default) the library's choice (corr_nt_auto)
        int corr_nt_partial = 1;       // env BTBA_CORR_NT_PARTIAL=0 (developer): all instances stream non-temporally once the batch exceeds the cache, not only those that do not fit
        long long last_level_cache = 224ll << 20;   // env BTBA_LLC_MB: what of the 256 MB memory-side cache a batch's frames + correspondences may fill before the stream is read non-temporally
        bool relayout = false;         // BTBA_OPT_RELAYOUT (env BTBA_RELAYOUT=1 turns it on): a batch given as EntryJ is re-laid out to 24-byte records by its first iteration's sweep
        bool solve_small = true;       // BTBA_OPT_SOLVE_SMALL (env BTBA_SOLVE_LEGACY=1 turns it off): k_solve_small for windows of <= 21 frames
        int prepare_keep_T = 0;        // env BTBA_PREPARE_KEEP_T (developer / experiment builds): a solve's incoming matrices are its first iterate's T as they are (k_prepare)
        int debug_lds_pad = 0;         // env BTBA_DEBUG_LDS_PAD (developer): extra dynamic LDS bytes per sweep workgroup -- what a larger LDS footprint costs the fused sweep
    } tune;
    std::vector<int32_t> dense_pairs_host;                  // what dense_pairs currently holds
    int dense_pairs_frames = -1;
    size_t dense_work_offset = 0;                           // ints into dense_pairs: the fused sweep's work table
    int work_formula = 0;                                   // SolveDims::work_formula of that table
    int solve_tab_frames = -1;                              // window size solve_tab was built for
    std::vector<EventPair> events;                          // pending timed regions
    std::vector<hipEvent_t> event_pool;
    btba_stats stats{};
    bool lds_attr_set = false, small_attr_set = false, mid_attr_set = false, vos_attr_set = false, lfnet_attr_set = false, lfnet_det_attr_set = false;
    bool always_time_region = false;   // optimize_frames: ms_solve is part of its stats contract
    static constexpr int kMaxGroups = 8;
    uint64_t solves_enqueued = 0;      // rotates the sampled iteration of BTBA_FLAG_TIME_SAMPLED
    hipStream_t aux_streams[kMaxGroups - 1] = {};  // groups 1 .. G-1 of a batch run here (software pipelining across instances)
    hipEvent_t ev_fork = nullptr, ev_join[kMaxGroups - 1] = {}, ev_order = nullptr;
    // optimize_frames (round 6): the EntryJ / pose upload runs on a stream of its own while the frame cache is built on `stream`; small tables the cache build and
    // the solve need (pointer tables, slot maps, valid counts) go through ONE pinned staging block, so that no call has to synchronise just to keep a local alive
    hipStream_t copy_stream = nullptr;
    hipEvent_t ev_copy = nullptr, ev_cache = nullptr;
    PinBuf pin;
    PinBuf pin_io;                                          // pinned: [poses out | poses in | pair offsets] of one optimize_frames call (small pageable copies cost ~10 us of host time each)
    struct PendingSlot { int slot; uint64_t key; const float *depth, *normal; };
    std::vector<PendingSlot> pool_pending;                  // frames cached by the call in flight: committed (live, n_valid) once their counts have come back

    // persistent frame cache (btba_optimize_frames_keyed): compact (z, n) frames, their valid-pixel lists and counts
    // live in pool slots that survive across calls; a keyframe is cached once, not once per BA call.
    struct FrameSlot { uint64_t key = 0; const float *depth = nullptr, *normal = nullptr; uint64_t stamp = 0; bool live = false; int32_t n_valid = 0; };
    DevBuf pool_zn, pool_lists, pool_counts, pool_nvalid, pool_map, pool_ranges;
    size_t pool_map_offset = 0;                             // bytes into pool_map at which the window's frame -> slot map starts (behind the call's pointer table)
    // keyed correspondence cache (BTBA_FLAG_KEYED_CORR): the EntryJ segment of a frame PAIR stays on the device under the pair's two
    // frame keys; a sliding window then uploads only the new frame's K - 1 segments
    struct CorrSeg { uint32_t off = 0, count = 0; };
    DevBuf corr_pool, corr_desc, corr_stage_dev, corr_lens;   // pool of 24-byte correspondences; staging of a call's fresh EntryJ segments; the window's segment lengths
    std::map<std::pair<uint64_t, uint64_t>, CorrSeg> corr_index;
    size_t corr_pool_used = 0;                              // in entries
    PinBuf corr_stage;                                      // pinned host staging of the segments uploaded by one call
    DevBuf ransac;                                          // btba_ransac_pairs staging (points, samples, per-trial poses and counts, results)
    DevBuf ransac_u;                                        // the reference's sample stream: n_trials x 3 uniforms (btba_xorwow.hpp), kept per (seed, n_trials)
    std::vector<float> ransac_u_host;
    DevBuf match;                                           // btba_match_pairs: tables, norms, candidate lists, selections, counts, host-form staging
    DevBuf mask;                                            // btba_apply_masks: labels, counts, argmax keys, row extents, spans, hull stacks, ROI slots
    DevBuf eval;                                            // btba_pose_errors: chunk tables, host-form poses and outputs, per-point minima
    DevBuf nocs;                                            // btba_nocs_errors: item words, boxes, step table, host-form poses and outputs
    DevBuf corres;                                          // btba_corres_chain: frame / pair tables, NN output, working lists, per-pair words
    DevBuf vos;                                             // btba_vos_propagate: the key splits' partial (m, l, acc) per item and target position
    DevBuf lfnet;                                           // btba_lfnet_*: per-map moments, peak flags, the compacted peak list
    DevBuf lfnet_desc;                                      // btba_lfnet_descriptors: two buffers of a chunk's widest layer
    DevBuf lfnet_det;                                       // btba_lfnet_scores: the residual stream and conv1's output of a pass, NHWC
    DevBuf vos_net;                                         // btba_vos_features: the four NHWC activation buffers of a pass
    DevBuf window;                                          // btba_procrustes_pairs: segment table, moments, host-form poses and outputs
    DevBuf marginals;                                       // btba_linearize_batch_zn_aux: the copy of the poses and the record of its one traced iterate
    bool marginals_attr_set = false;
    DevBuf objective;                                       // btba_objective_batch_zn_aux: the matrices of the caller's poses, the partial records of tiles and chunks
    DevBuf fusion;                                          // btba_fuse_frames: the voxel planes (count, position, normal and colour sums), the compaction's block counts
    DevBuf registration;                                    // btba_register_frames: the partial records, current poses and stop flags
    uint64_t ransac_u_seed = 0;
    std::vector<FrameSlot> pool_slots;
    int pool_H = 0, pool_W = 0, pool_npix = 0;
    float pool_downscale = 0.0f, pool_K[9] = {0};
    uint64_t pool_stamp = 0;
    uint64_t pool_hits = 0, pool_misses = 0;

    hipEvent_t get_event()
    {
        if (!event_pool.empty()) { hipEvent_t e = event_pool.back(); event_pool.pop_back(); return e; }
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) return nullptr;
        return e;
    }
};

// A workspace belongs to the device that was current when it was created.  A process that drives several GPUs from one thread
// ("one process looping hipSetDevice") may call in with another device current: every entry point that takes a
// workspace switches to the workspace's device for the duration of the call and back afterwards.
struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(const btba_workspace *ws)
    {
        int cur = -1;
        if (ws && hipGetDevice(&cur) == hipSuccess && cur != ws->device && hipSetDevice(ws->device) == hipSuccess) prev = cur;
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};

// btba_objective_batch_zn_aux behind its argument checks (btba_api_objective.hip): the dense pair list and its device table as solve_enqueue derives
// them, the scratch, k_prepare and the launches of btba_objective.hpp.  Defined in btba_api.hip, the one unit that holds the sweeps' device functions.
struct ObjectiveCall {
    const btba_params *prm;
    int B, N, H, W, Hd, Wd;
    const float *K, *zn, *poses;
    const void *corr; bool corr24; int64_t corr_stride;     // nullptr: no sparse term
    const uint32_t *pair_offsets; uint32_t max_corr_per_pair;
    const int32_t *dense_pairs; int n_dense_pairs;          // host list, or nullptr: every i < j
    btba_objective_total *total; btba_objective_pair *sparse, *dense;
};
int objective_enqueue(btba_workspace *ws, const ObjectiveCall &c);

// The argument checks btba_fuse_bounds / btba_fuse_frames make of params and segments, and whether a segment is a frame (btba_api_fusion.hip);
// btba_register_frames takes the same segments and refuses what fusion refuses.
namespace btba_host {
bool fuse_segments_ok(const btba_fuse_params *prm, int n_instances, int n_segments, const btba_fuse_segment *seg, int H, int W, const float *K, bool need_colour);
bool fuse_has_frames(int n_segments, const btba_fuse_segment *seg);
}

// What a model handle of either LF-Net net starts with: its workspace, that workspace's device and the arena's device copy.
struct LfnetModelBase {
    btba_workspace *ws = nullptr;
    int device = 0;
    DevBuf dev;
    int upload(const LfnetArena &a)
    {
        if (int rc = dev.ensure(sizeof(float) * a.total)) return rc;
        HIP_TRY(hipMemcpy(dev.p, a.host.data(), sizeof(float) * a.total, hipMemcpyHostToDevice));
        return BTBA_OK;
    }
};

// The destroy of a handle with a `device` member that owns device memory and is not part of a workspace.
template <class M> void destroy_on_device(M *m)
{
    if (!m) return;
    int prev = -1;
    if (hipGetDevice(&prev) != hipSuccess || prev == m->device || hipSetDevice(m->device) != hipSuccess) prev = -1;
    (void)hipDeviceSynchronize();                                     // delete frees the buffers; no workspace access
    delete m;
    if (prev >= 0) (void)hipSetDevice(prev);
}

inline void scaled_intrinsics(int H, int W, int Hd, int Wd, const float *K, float intr[4], Mat4 *Kinv)
{
    // CUDACache.cpp:20-24
    intr[0] = K[0] * ((float)Wd / (float)W);
    intr[1] = K[4] * ((float)Hd / (float)H);
    intr[2] = K[2] * ((float)(Wd - 1) / (float)(W - 1));
    intr[3] = K[5] * ((float)(Hd - 1) / (float)(H - 1));
    // m_inputIntrinsicsInv (CUDACache.cpp:33): generic cofactor inverse of the 4x4 embedding of K, in fp32
    const float m[16] = { K[0], K[1], K[2], 0, K[3], K[4], K[5], 0, K[6], K[7], K[8], 0, 0, 0, 0, 1 };
    auto minor = [&](int r0, int r1, int r2, int c0, int c1, int c2) {
        return m[4 * r0 + c0] * (m[4 * r1 + c1] * m[4 * r2 + c2] - m[4 * r1 + c2] * m[4 * r2 + c1])
             - m[4 * r0 + c1] * (m[4 * r1 + c0] * m[4 * r2 + c2] - m[4 * r1 + c2] * m[4 * r2 + c0])
             + m[4 * r0 + c2] * (m[4 * r1 + c0] * m[4 * r2 + c1] - m[4 * r1 + c1] * m[4 * r2 + c0]);
    };
    float adj[16];
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) {
            int rr[3], cc[3], a = 0, b = 0;
            for (int k = 0; k < 4; k++) { if (k != r) rr[a++] = k; if (k != c) cc[b++] = k; }
            float mn = minor(rr[0], rr[1], rr[2], cc[0], cc[1], cc[2]);
            adj[4 * c + r] = ((r + c) & 1) ? -mn : mn;
        }
    const float det = m[0] * adj[0] + m[1] * adj[4] + m[2] * adj[8] + m[3] * adj[12];
    const float rdet = 1.0f / det;
    for (int k = 0; k < 16; k++) Kinv->m[k] = adj[k] * rdet;
}
