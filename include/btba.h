/*
 * btba.h -- C ABI of the MI355X-native pose-graph bundle adjustment (libbtba.so).
 *
 * Drop-in boundary for BundleTrack's  OptimizerGpu::optimizeFrames
 *   (/root/reference/src/cuda/LossGPU.h:40-52, LossGPU.cu:53-139; call site src/Bundler.cpp:350-351)
 * and for the C-linkage seams underneath it
 *   (solveBundlingStub, buildVariablesToCorrespondencesTableCUDA, convertLiePosesToMatricesCU:
 *    src/cuda/Solver/CUDASolverBundling.cpp:8-16; convertMatricesToPosesCU / convertPosesToMatricesCU:
 *    src/cuda/SBA.cpp:10-13).
 *
 * Plain C: pointers, sizes, PODs.  No torch / Eigen / YAML types.  Device pointers are raw HIP
 * device addresses; `stream` arguments are hipStream_t passed as void*.  No entry point ever
 * exits, aborts or spins (the reference does all three: cutil_inline_runtime.h:261-269,
 * SolverBundling.cu:621-625): errors come back as an int status.
 */
#ifndef BTBA_H_
#define BTBA_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BTBA_VERSION 105     /* 105: BTBA_OPT_SOLVE_SMALL, btba_params.n_weights_per_iter; 104: chained launch (BTBA_OPT_CHAIN*, BTBA_ESCHED, btba_stats.chain_iterations), btba_params.weights_*_per_iter, btba_workspace_live_blocks; 103: btba_params.reduction_mode, BTBA_FLAG_KEYED_CORR = 4096,
                                btba_workspace_set_option, btba_zn_aux.corr24 + btba_pack_correspondences24.  A caller built against another version's structs must not
                                call in: check btba_version() == BTBA_VERSION once after loading the library (the Python and C++ host layers do). */

#if defined(__GNUC__)
#define BTBA_API __attribute__((visibility("default")))
#else
#define BTBA_API
#endif

/* ---- status codes ---------------------------------------------------------------------- */
enum {
    BTBA_OK       = 0,
    BTBA_EINVAL   = 1,   /* bad argument (n_frames < 2, null pointer, unsorted batch correspondences, ...) */
    BTBA_EHIP     = 2,   /* a HIP runtime call failed; btba_last_hip_error() has the hipError_t */
    BTBA_ENUMERIC = 3,   /* a non-finite value reached the output poses */
    BTBA_ENOMEM   = 4,
    BTBA_ESCHED   = 5    /* reserved: the retired chained launch's scheduling failure; no longer returned */
};

/* ---- wire formats ---------------------------------------------------------------------- */
/* struct EntryJ, src/cuda/SIFTImageManager.h:44-59: 32 bytes; invalid <=> imgIdx_i == 0xFFFFFFFF.
 * pos_i / pos_j are the matched 3-D points in the camera frames of frame i / frame j
 * (Bundler.cpp:311-316: i < j, pos_i = _ptB_cam, pos_j = _ptA_cam). */
typedef struct btba_entryj {
    uint32_t imgIdx_i;
    uint32_t imgIdx_j;
    float pos_i[3];
    float pos_j[3];
} btba_entryj;

/* Dense pair orientation (the reference derives it from device
 * allocation addresses, SolverBundling.cu:25-33, so it must be an explicit choice here). */
enum {
    BTBA_PAIRS_TARGET_LOWER      = 0,  /* every i<j once, target = i (BundleFusion behaviour; default) */
    BTBA_PAIRS_TARGET_MORE_VALID = 1,  /* target = frame with more valid depth pixels, ties i<j; literal
                                          FlipJtJ semantics: the cross block vanishes when target > source */
    BTBA_PAIRS_EXPLICIT          = 2,  /* caller passes the ordered (target, source) list */
    BTBA_PAIRS_TARGET_HIGHER     = 3   /* every i<j once, target = j: what FindImageImageCorr_Kernel emits when the per-frame
                                          d_num_valid_points allocations have ASCENDING addresses in frame order (one cudaMalloc per
                                          frame in a fresh CUDACache, CUDACacheUtil.h:14) -- every dense cross block is then above
                                          the diagonal and erased by FlipJtJ_Kernel (SolverBundling.cu:49-59) */
};

/* How the sweeps' sums are reduced.  DETERMINISTIC (default): every workgroup stores its partial record, k_system_solve adds them in a
 * fixed order -- run-to-run reproducible bits.  ATOMIC: what the reference does (SolverBundlingDenseUtil.h:217-285, SolverBundling.cu
 * warpReduce + atomicAdd throughout): workgroups add into one record per frame pair with hardware float atomics, in whatever order they
 * finish -- results move in the last bits from run to run, exactly as the reference's do; no partial arrays, one reduction pass less.
 * Not available together with BTBA_FLAG_TRACE (the decision traces are defined on the reproducible sums). */
enum {
    BTBA_REDUCE_DETERMINISTIC = 0,
    BTBA_REDUCE_ATOMIC        = 1
};

enum {
    BTBA_FLAG_TRACE         = 1,    /* record per-GN-iterate trace (btba_trace_layout)                            */
    BTBA_FLAG_TIME_KERNELS  = 2,    /* bracket every sweep / solve launch with hipEvents (btba_stats)             */
    BTBA_FLAG_TIME_SAMPLED  = 2048, /* with TIME_KERNELS: bracket the launches of ONE Gauss-Newton iteration per solve only (the iteration
                                       rotates from solve to solve): 28 event records per 7-iteration solve cost ~4 % of a c3 x 32 step,
                                       4 do not; the per-launch averages in btba_stats are over the sampled launches              */
    BTBA_FLAG_OVERLAP       = 32,   /* split a batch over two streams (main + low-priority) so one half's k_system_solve
                                       overlaps the other half's sweeps; per-kernel timings then overlap too (+4 % at c3 x 32) */
    BTBA_FLAG_NO_FUSE       = 64,   /* launch the sparse and the dense sweep separately (default: ONE interleaved launch) */
    BTBA_FLAG_FLOAT4_CACHE  = 256,  /* btba_optimize_frames: build the reference-layout float4 cache instead of the compact one */
    /* 128: reserved.  It was BTBA_FLAG_FUSE ("accepted for compatibility") up to version 100 and must not acquire a meaning: ignored. */
    BTBA_FLAG_KEYED_CORR    = 4096, /* btba_optimize_frames_keyed: keep every frame PAIR's correspondence segment on the device under the
                                       pair's two frame keys and upload only segments not seen before (in a sliding window: the new
                                       frame's n_frames - 1 pairs).  CONTRACT: the correspondences of a pair do not change while both
                                       frames stay cached -- the reference never recomputes a pair's matches either (findCorres returns
                                       early when _matches holds the pair, FeatureManager.cpp:176) -- and n_match_per_pair is given.  A
                                       segment whose length changed is uploaded again (its superseded copy stays in the pool until one of the
                                       pair's frames is evicted or the cache is cleared); a cached segment is not checked for pair order
                                       again; btba_frame_cache_evict / _clear drop segments */
    BTBA_FLAG_NO_COMPACTION = 512,  /* compact cache: always walk all Wd x Hd source pixels                        */
    BTBA_FLAG_COMPACTION    = 1024  /* compact cache: walk each source frame's ordered list of pixels that carry a depth
                                       (masked scenes).  btba_optimize_frames decides by itself from the valid-pixel counts
                                       unless one of the two is set; btba_solve_batch_zn (asynchronous, no read-back) uses
                                       lists only when this flag is set */
};

/* Solver parameters.  Defaults = shipping config of the reference:
 *   config_ycbineoat.yml:23-31,63-65; SBA.cpp:27-32; CUDASolverBundling.cpp:93-98. */
typedef struct btba_params {
    int32_t n_gn_iters;           /* bundle.num_iter_outter      7      */
    int32_t n_pcg_iters;          /* bundle.num_iter_inner       5      */
    float   robust_delta;         /* bundle.robust_delta         0.005  */
    float   dense_dist_thresh;    /* p2p.max_dist                0.02   */
    float   dense_normal_thresh;  /* cos(p2p.max_normal_angle)   cos 45 deg */
    float   depth_min;            /* denseDepthMin               0.1    */
    float   depth_max;            /* denseDepthMax               9999   */
    float   weight_sparse;        /* m_localWeightsSparse        1      */
    float   weight_dense_depth;   /* m_localWeightsDenseDepth    1  (0 disables the dense term)       */
    float   image_downscale;      /* bundle.image_downscale      4      */
    int32_t pair_policy;          /* BTBA_PAIRS_*                                                       */
    int32_t dense_tiles;          /* workgroups per dense frame pair (0 = auto)                        */
    int32_t sparse_chunks;        /* workgroups per correspondence segment (0 = auto)                  */
    int32_t flags;                /* BTBA_FLAG_*                                                        */
    int32_t reduction_mode;       /* BTBA_REDUCE_*                                                      */
    /* Optional per-iteration weights, the form the solveBundlingStub seam takes them in (input.weightsSparse[nIter], input.weightsDenseDepth[nIter],
     * SolverBundling.cu:948-951; SBA.cpp:27-32 fills both with constants): HOST arrays of n_gn_iters floats >= 0, or NULL = weight_sparse /
     * weight_dense_depth in every iteration.  As in the reference, an iteration with dense weight 0 builds no dense system (useDense = false,
     * :951-953), and an iteration with sparse weight 0 still derives its Jacobi preconditioner from the correspondences (the preconditioner carries
     * no weight, SolverBundlingEquationsLie.h:107-108) while right-hand side and operator take the factor 0. */
    const float *weights_sparse_per_iter;
    const float *weights_dense_per_iter;
    int32_t n_weights_per_iter;   /* length of the arrays above as the caller allocated them: with either pointer set it must equal n_gn_iters (BTBA_EINVAL
                                   * otherwise -- the library never reads past what was stated); ignored when both are NULL.  btba_params_default: 0 */
} btba_params;

/* Timing / diagnostics filled by the solve entry points (all times in milliseconds, measured
 * with hipEvents on the workspace stream; per-kernel fields need BTBA_FLAG_TIME_KERNELS). */
/* Largest window: 85 frames, the reference's MAX_NUM_IMAGES (GlobalDefines.h:8; its solver spins forever above it,
 * SolverBundling.cu:621-625; it ships max_BA_frames = 15, config_ycbineoat.yml:27).  Up to BTBA_MAX_FRAMES_LDS frames the
 * 6N x 6N normal matrix of an instance lives in one CU's 160 KB of LDS (186 x 188 floats at N = 31) and a single wave runs
 * the PCG; larger windows keep the matrix in an L2-resident device scratch and run a 16-wave PCG (slower per iterate, same
 * arithmetic).  A window of more than BTBA_MAX_FRAMES frames is BTBA_EINVAL. */
#define BTBA_MAX_FRAMES 85
#define BTBA_MAX_FRAMES_LDS 31

typedef struct btba_stats {
    int32_t n_instances, n_frames, n_pairs, n_dense_pairs;
    int64_t n_corr;               /* total correspondences over all instances                          */
    int32_t dense_tiles, sparse_chunks;
    float ms_total;               /* whole call, host wall clock                                       */
    float ms_upload;              /* H2D of EntryJ + poses (optimize_frames only)                      */
    float ms_cache;               /* frame cache build (A3)                                            */
    float ms_solve;               /* pose-in -> pose-out region on the stream                          */
    float ms_dense_sweep;         /* sum over GN iterations of the dense Jacobian sweep kernel         */
    float ms_sparse_sweep;        /* ... of the sparse sweep kernel                                    */
    float ms_system_solve;        /* ... of the assemble + PCG + update kernel                         */
    int32_t n_dense_launches, n_sparse_launches, n_solve_launches;
    int64_t bytes_dense_alg;      /* algorithmic bytes of ONE dense sweep launch  (64 * Pd * npix * B) */
    int64_t bytes_sparse_alg;     /* algorithmic bytes of ONE sparse sweep launch (32 * C)             */
    int32_t fused_sweeps;         /* 1: sparse + dense sweeps ran as ONE launch (timed as ms_dense_sweep) */
    int32_t cache_frames_built;   /* optimize_frames: frames cached in this call (n_frames unless keyed and already cached) */
    int32_t corr_pairs_uploaded;  /* optimize_frames: frame-pair segments that crossed PCIe in this call (all P unless BTBA_FLAG_KEYED_CORR) */
    int32_t chain_iterations;     /* always 0: the chained launch was retired (kept for the struct's layout) */
} btba_stats;

/* Per-instance, per-GN-iteration trace record (floats), written when BTBA_FLAG_TRACE is set.
 * Record r = instance * n_gn_iters + iteration; record size = btba_trace_layout.record_floats.
 *   x_after     [N][6]   (rot, trans) after the update
 *   T_after     [N][16]  Exp(x_after), row-major
 *   rhs         [N][6]   (rRot, rTrans): PCG right-hand side  (frame 0 = 0)
 *   precond     [N][6]   (precRot, precTrans)                 (frame 0 = 0)
 *   pcg         [n_pcg][4]  pAp, alpha, rz_new, beta
 *   delta       [N][6]   PCG solution (deltaRot, deltaTrans)
 *   dense_pair  [Pd][28] S (21, upper triangle row-major of the 6x6 in [trans,rot] order), g (6), count
 *   A           [6N][6N] assembled normal matrix (sparse + dense), reference dense layout
 *   clk         [8]      shader-clock stamps of k_system_solve's phases (reduce, congruence, assemble, PCG, update)
 */
typedef struct btba_trace_layout {
    int64_t record_floats;
    int64_t off_x, off_T, off_rhs, off_precond, off_pcg, off_delta, off_dense_pair, off_A, off_clk;
} btba_trace_layout;

typedef struct btba_workspace btba_workspace;

/* ---- API -------------------------------------------------------------------------------- */
BTBA_API void btba_params_default(btba_params *p);
BTBA_API const char *btba_strerror(int status);
BTBA_API int btba_last_hip_error(void);
BTBA_API int btba_version(void);

/* One workspace = one HIP stream + reusable device scratch.  `stream` may be NULL (the
 * workspace then creates and owns a non-blocking stream: the caller orders it against its own streams with
 * btba_workspace_wait_stream / _signal_stream).  Re-entrant across workspaces.  A workspace lives on the device that is
 * current when it is created; every call that takes it switches to that device for its duration and restores the caller's
 * (one thread may drive several GPUs, one workspace each; buffers handed to a call must live on the workspace's device). */
BTBA_API int btba_workspace_create(btba_workspace **out, void *stream);
/* Same, but `stream` is used as given even when it is the NULL (legacy default) stream -- what a framework whose
 * "current stream" is the default stream (PyTorch) needs so that its own copies and kernels order with the solver. */
BTBA_API int btba_workspace_create_on_stream(btba_workspace **out, void *stream);
BTBA_API void btba_workspace_destroy(btba_workspace *ws);
BTBA_API int btba_workspace_sync(btba_workspace *ws);

/* Developer / tuning switches of a workspace.  None of them changes WHAT is computed (only schedules and which of two equivalent
 * code paths runs); they exist for A/B measurements and for tests that hold one path against the other.  Each also has an environment
 * variable that sets the initial value -- read once, inside btba_workspace_create*, never on the solve path. */
enum {
    BTBA_OPT_DENSE_ORDER          = 1,  /* 1 (default): dense pairs worked off heaviest first (|i - j| ascending); 0: list order.  env BTBA_NO_DENSE_ORDER */
    BTBA_OPT_TILE_MAJOR           = 2,  /* 1 (default): (band, pair) work order inside an instance; 0: (pair, band).            env BTBA_PAIR_MAJOR     */
    BTBA_OPT_BLOCK_WALK           = 3,  /* 1 (default): pinhole sweep walks 8 x 8 pixel blocks; 0: 64 x 1 strips.               env BTBA_NO_BLOCK_WALK  */
    BTBA_OPT_BLOCK_SKIP           = 4,  /* 1 (default): provably dead blocks are not walked; 0: every block is.                 env BTBA_NO_BLOCK_SKIP  */
    BTBA_OPT_BIG_ASSEMBLY         = 5,  /* 1 (default): many-workgroup reduction / assembly from 24 frames on; 0: one workgroup. env BTBA_NO_BIG_ASSEMBLY */
    BTBA_OPT_OVERLAP_GROUPS       = 6,  /* instance groups of BTBA_FLAG_OVERLAP, 1 .. 8 (default 2).                            env BTBA_GROUPS         */
    BTBA_OPT_OVERLAP_EQUAL_PRIO   = 7,  /* 1: the groups' streams get equal priority (default 0: lowest for groups >= 1).        env BTBA_GROUP_PRIO=e   */
    BTBA_OPT_SPARSE_TAIL          = 9,  /* 0 .. 256: share (x / 256) of the sparse items that close the fused sweep instead of being interleaved (fills the launch's drain); -1 (default): 256 on full frames, 0 on object-masked ones. env BTBA_SPARSE_TAIL */
    BTBA_OPT_KEYED_CORR_MIN_BYTES = 8,  /* BTBA_FLAG_KEYED_CORR is ignored below this many bytes of correspondences (default 1 MiB). env of the same name */
    BTBA_OPT_CHAIN                = 10, /* retired (the chained launch): -1 .. 1 is accepted and ignored, no launch supports the solve */
    BTBA_OPT_CHAIN_SPARSE_PERIOD  = 11, /* retired: 0 or 2 .. 64 is accepted and ignored */
    BTBA_OPT_CHAIN_TIMEOUT_MS     = 12, /* retired: 1 .. 60000 is accepted and ignored */
    BTBA_OPT_RELAYOUT             = 14, /* 1: a batch whose correspondences arrive as EntryJ (4 MiB or more, three iterations or more, full frames) is re-laid out to
                                           24-byte records BY ITS FIRST ITERATION'S SWEEP, and the other iterations stream those; 0 (default): every iteration reads
                                           EntryJ.  Same bits; measured a wash at c3 x 32 (the first launch's extra writes cost what the others save).  env BTBA_RELAYOUT */
    BTBA_OPT_CORR_NONTEMPORAL     = 15, /* how the sparse items read the correspondences: -1 (default) with plain loads while the batch's frames + correspondences fit the
                                           memory-side cache (224 MiB of MI355X's 256 MB; env BTBA_LLC_MB), beyond that the instances whose correspondences no longer
                                           fit beside the frames are read with NON-TEMPORAL loads, so that the read-once stream does not evict the frames the dense items
                                           re-read every iteration (c3 x 32: 185 -> 198 k GN it/s; never on object-masked frames); 0: plain loads always; 1: non-temporal
                                           always.  A cache policy: same bits.                                                    env BTBA_CORR_NT */
    BTBA_OPT_COUNT_LIVE           = 13, /* 1: the dense sweep's block-walk workgroups add the number of 8 x 8 pixel blocks they actually walk (the blocks the hull
                                           test could not prove dead) to a counter of the workspace -- setting the option clears it, btba_workspace_live_blocks
                                           reads it.  Measurement aid (bench.py: roofline.executed); one atomic per workgroup while it is on. */
    BTBA_OPT_SOLVE_SMALL          = 16  /* 1 (default): windows of <= 21 frames run the per-instance system solve k_solve_small (round 5: register-resident
                                           multi-wave PCG, frame-sum assembly, sixteen-lane inverse); 0: k_system_solve, the kernel of rounds 1-4, as for larger
                                           windows.  Same sums in another order: results agree to rounding (tests/test_gpu_parity.py).   env BTBA_SOLVE_LEGACY=1 = 0 */
};
BTBA_API int btba_workspace_set_option(btba_workspace *ws, int option, int64_t value);
/* Blocks walked by the dense sweeps enqueued since BTBA_OPT_COUNT_LIVE was last set to 1 (synchronises with the workspace stream). */
BTBA_API int btba_workspace_live_blocks(btba_workspace *ws, uint64_t *blocks);
/* Stream ordering without a host wait, for callers whose producers / consumers run on another HIP stream (PyTorch's
 * current stream, a camera driver's copy stream): _wait_stream makes everything enqueued on the workspace stream AFTER the
 * call wait for what `stream` holds at the time of the call (inputs uploaded or rendered there); _signal_stream makes
 * `stream` wait for what the workspace stream holds (poses / caches / filtered maps produced by the asynchronous entry
 * points).  `stream` = NULL is the legacy default stream.  No-ops when `stream` is the workspace's own stream. */
BTBA_API int btba_workspace_wait_stream(btba_workspace *ws, void *stream);
BTBA_API int btba_workspace_signal_stream(btba_workspace *ws, void *stream);

/* Drop-in for OptimizerGpu::optimizeFrames (LossGPU.cu:53-139).
 *   corres_host       : n_corres EntryJ on the host (any order; pair-major order as produced by
 *                       Bundler::optimizeGPU is used as is, anything else is bucketed by frame pair).
 *   n_match_per_pair  : may be NULL (the reference stores it and never reads it, SBA.cpp:85).  When given -- P = n(n-1)/2
 *                       segment lengths in pair order (0,1) (0,2) ... as Bundler::optimizeGPU builds them -- and adding
 *                       up to n_corres, the array is taken as pair-major and uploaded without a host pass; the device
 *                       verifies every entry against its segment's pair and the call falls back to host bucketing if
 *                       that check fails, so a wrong or inconsistent array costs time, never correctness.
 *   depth_dev[k]      : device float[H*W], metres, 0 = invalid          (Frame.h:73)
 *   normal_dev[k]     : device float4[H*W], xyz unit, w = 0, zeros = invalid (Frame.h:75)
 *   poses_rowmajor    : host float[n_frames*16], camera->model, in/out  (LossGPU.cu:88-97,121-130)
 *   K_rowmajor        : host float[9] full-resolution intrinsics
 *   dense_pairs       : BTBA_PAIRS_EXPLICIT only: n_dense_pairs (target, source) int32 pairs, host.
 * ws may be NULL: like the reference, everything is then allocated and freed inside the call, and the call runs on the
 * legacy NULL stream like the reference does -- depth / normal maps produced by earlier work on the default stream (or by
 * any blocking stream) are ordered before the cache build without the caller doing anything.  A caller that passes NULL
 * only for some calls must not race them against its own non-blocking streams.
 * n_match_per_pair must hold P = n_frames (n_frames - 1) / 2 ints when non-NULL (the host wrappers pass NULL when the
 * caller's vector has another length).
 * Synchronous: poses are valid on return.  Inside the call (round 6) the host is not synchronised before the end: the frame cache is built on the workspace's stream while
 * the EntryJ array and the poses are uploaded on a second, non-blocking stream the workspace owns (it touches the workspace's own buffers only; the solve waits for its event),
 * and every small table crosses through pinned blocks of the workspace -- with ws == NULL those are created and destroyed per call like everything else. */
BTBA_API int btba_optimize_frames(btba_workspace *ws, const btba_params *params,
                         int n_frames, int H, int W, const float *K_rowmajor,
                         const btba_entryj *corres_host, uint32_t n_corres, const int *n_match_per_pair,
                         const float *const *depth_dev, const float *const *normal_dev,
                         const int32_t *dense_pairs, int n_dense_pairs,
                         float *poses_rowmajor, btba_stats *stats);

/* btba_optimize_frames with a PERSISTENT frame cache.  frame_keys[k] is a caller-chosen id
 * of frame k that is stable across calls (the tracker's Frame::_id, Frame.h:61).  A frame whose (key, depth pointer,
 * normal pointer) was cached by an earlier call on the same workspace, with the same H, W, K and image_downscale, is
 * NOT cached again: its compact (z, n) pixels, its valid-pixel list and count stay in a pool slot of the workspace
 * (least-recently-used slots are recycled; pool = max(32, 2 n_frames) slots for the largest window so far: a window
 * that needs more re-allocates the pool, and so does another H, W, K or image_downscale -- every frame is then cached
 * again; which of several slots last used by the same call goes first is not specified).  In a tracker only the new frame is
 * built per call, the keyframes were cached when they were new -- the reference re-caches all K frames every call
 * (LossGPU.cu:74-78).  The caller must not modify a frame's device buffers while it is cached under the same key
 * (keyframes are immutable after Frame's constructor, Frame.cpp:107-149); btba_frame_cache_clear drops everything.
 * Results are bit-identical to btba_optimize_frames.  ws must not be NULL; BTBA_FLAG_FLOAT4_CACHE is rejected. */
BTBA_API int btba_optimize_frames_keyed(btba_workspace *ws, const btba_params *params,
                         int n_frames, int H, int W, const float *K_rowmajor,
                         const btba_entryj *corres_host, uint32_t n_corres, const int *n_match_per_pair,
                         const float *const *depth_dev, const float *const *normal_dev, const uint64_t *frame_keys,
                         const int32_t *dense_pairs, int n_dense_pairs,
                         float *poses_rowmajor, btba_stats *stats);
BTBA_API int btba_frame_cache_clear(btba_workspace *ws);
/* Forget ONE cached frame (a tracker dropping a frame whose id it may hand out again, Bundler.cpp:96-104: a failed frame is
 * popped and the next one gets the same id).  Unknown keys are not an error. */
BTBA_API int btba_frame_cache_evict(btba_workspace *ws, uint64_t frame_key);

/* Frame cache build alone (CUDACache::CUDACache + storeFrame, CUDACache.cpp:14-38,76-88).
 * Outputs (device): campos float4[n_frames][Hd*Wd], normals float4[n_frames][Hd*Wd],
 * n_valid int32[n_frames] (may be NULL); intr_out (host) = downscaled (fx, fy, cx, cy).
 * Asynchronous on the workspace stream. */
BTBA_API int btba_build_cache(btba_workspace *ws, int n_frames, int H, int W, const float *K_rowmajor,
                     float image_downscale, const float *const *depth_dev, const float *const *normal_dev,
                     float *campos_dev, float *normals_dev, int32_t *n_valid_dev, float *intr_out);

/* Batched solve over device-resident instances that share n_frames and the cache resolution
 * (the solveBundlingStub seam, SolverBundling.cu:931-1003, for many independent trackers).
 *   campos_dev / normals_dev : float4 [n_instances][n_frames][Hd*Wd]
 *   corr_dev                 : EntryJ [n_instances][corr_stride], each instance pair-major over the
 *                              canonical pair order (0,1),(0,2)..(N-2,N-1)
 *   pair_offsets_dev         : uint32 [n_instances][P+1] segment starts inside the instance's block
 *   max_corr_per_pair        : upper bound of any segment length (sizes the launch)
 *   poses_dev                : float [n_instances][n_frames][16] in/out
 *   dense_pairs (host)       : ordered (target, source) list or NULL for TARGET_LOWER
 *   trace_dev                : NULL or float [n_instances*n_gn_iters*record_floats]
 * Asynchronous on the workspace stream; stats (if non-NULL) are complete after
 * btba_workspace_sync() and a following btba_collect_stats(). */
BTBA_API int btba_solve_batch(btba_workspace *ws, const btba_params *params,
                     int n_instances, int n_frames, int Hd, int Wd, const float *intr,
                     const float *campos_dev, const float *normals_dev,
                     const btba_entryj *corr_dev, int64_t corr_stride,
                     const uint32_t *pair_offsets_dev, uint32_t max_corr_per_pair,
                     const int32_t *dense_pairs, int n_dense_pairs,
                     float *poses_dev, float *trace_dev);
/* SURVEY.md 8(b)'s single-instance cached entry (one tracker, frame cache already built by btba_build_cache): the same
 * solve as btba_solve_batch with n_instances = 1 and corr_stride = n_corr. */
BTBA_API int btba_solve_cached(btba_workspace *ws, const btba_params *params, int n_frames, int Hd, int Wd, const float *intr,
                     const float *campos_dev, const float *normals_dev,
                     const btba_entryj *corr_dev, uint32_t n_corr,
                     const uint32_t *pair_offsets_dev, uint32_t max_corr_per_pair,
                     const int32_t *dense_pairs, int n_dense_pairs,
                     float *poses_dev, float *trace_dev);
BTBA_API int btba_collect_stats(btba_workspace *ws, btba_stats *stats);

BTBA_API void btba_trace_layout_get(int n_frames, int n_dense_pairs, int n_pcg_iters, btba_trace_layout *out);

/* Host helpers (A0/A6 side): bucket arbitrary EntryJ by canonical frame pair.
 * out_sorted (n entries) and out_offsets (P+1) are host buffers.  Returns BTBA_EINVAL if an
 * entry references a frame >= n_frames or has imgIdx_i >= imgIdx_j. Invalid entries are dropped
 * (offsets[P] = number kept). */
BTBA_API int btba_bucket_correspondences(const btba_entryj *in, uint32_t n, int n_frames,
                                btba_entryj *out_sorted, uint32_t *out_offsets);

/* SE(3) seams (convertMatricesToPosesCU / convertPosesToMatricesCU / convertLiePosesToMatricesCU)
 * on device data; n transforms, x = (rot, trans) float[n][6]; any output may be NULL. */
BTBA_API int btba_matrices_to_poses(btba_workspace *ws, int n, const float *T_dev, float *x_dev);
BTBA_API int btba_poses_to_matrices(btba_workspace *ws, int n, const float *x_dev, float *T_dev, float *Tinv_dev);

/* ---- the step before the boundary (what Frame's constructor runs per frame) ---- */
/* Frame::processDepth (src/Frame.cpp:152-180): erode (CUDAImageUtil.cu:676-718) then the mean-gated bilateral
 * filter twice (CUDAImageUtil.cu:735-797), fused in ONE launch.  depth_in_dev / depth_out_dev: device float[H*W]
 * (must not alias).  Defaults of config_ycbineoat.yml:9-16: erode radius 1, diff 0.001, ratio 0.8; filter radius 2,
 * sigma_D 2, sigma_R 100000.  Asynchronous on the workspace stream. */
BTBA_API int btba_process_depth(btba_workspace *ws, int H, int W, const float *depth_in_dev, float *depth_out_dev,
                                int erode_radius, float erode_diff, float erode_ratio,
                                int bf_radius, float sigma_d, float sigma_r);

/* Frame::depthToCloudAndNormals (src/Frame.cpp:182-233): depth -> camera-space points (CUDAImageUtil.cu:310-327)
 * -> normals (computeNormals_Kernel, CUDAImageUtil.cu:342-412), ONE launch.  normals_dev: device float4[H*W]
 * (xyz unit, w = 0, zeros = invalid: the optimiser's input format); xyz_dev: device float4[H*W] or NULL. */
BTBA_API int btba_depth_to_normals(btba_workspace *ws, int H, int W, const float *K_rowmajor,
                                   const float *depth_dev, float *normals_dev, float *xyz_dev);

/* ---- compact frame cache ("ZN") ------------------------------------------------------------------------
 * camPos is a pure function of (full-resolution pixel, depth) -- CUDAImageUtil.cu:310-327 -- so the cache can hold
 * float4 (z, nx, ny, nz) per pixel, 16 B instead of the reference's 32 B (CUDACachedFrame, CUDACacheUtil.h:10-53), and
 * the sweep re-derives camPos with the cache builder's exact fp32 operations: identical results, half the bytes,
 * half the load instructions.  btba_optimize_frames uses it internally (BTBA_FLAG_FLOAT4_CACHE switches back).
 * CONTRACT of the z lane: it is the GATED depth -- 0 wherever the reference's cached camPos is (0, 0, 0, 0), i.e. where
 * the full-resolution depth is below 0.1 m or NaN (CUDAImageUtil.cu:310-327) -- exactly camPos.z of the reference
 * layout.  btba_build_cache_zn and btba_pack_zn produce it; a caller that fills the cache itself must apply the gate. */
BTBA_API int btba_build_cache_zn(btba_workspace *ws, int n_frames, int H, int W, const float *K_rowmajor,
                                 float image_downscale, const float *const *depth_dev, const float *const *normal_dev,
                                 float *zn_dev /* float4[n_frames][Hd*Wd] */, int32_t *n_valid_dev, float *intr_out);
/* float4 camPos + float4 normals (reference layout) -> compact cache.  camPos.xy are dropped and re-derived from z, so
 * the input must have been produced by the standard formula (btba_build_cache or CUDACache). */
BTBA_API int btba_pack_zn(btba_workspace *ws, int64_t n_pixels_total, const float *campos_dev, const float *normals_dev, float *zn_dev);
/* btba_solve_batch on compact caches: zn_dev float4 [n_instances][n_frames][Hd*Wd]; H, W, K_rowmajor describe the
 * FULL-resolution frames the caches were built from (Hd = H / image_downscale, ...). */
BTBA_API int btba_solve_batch_zn(btba_workspace *ws, const btba_params *params, int n_instances, int n_frames,
                                 int H, int W, const float *K_rowmajor, const float *zn_dev,
                                 const btba_entryj *corr_dev, int64_t corr_stride,
                                 const uint32_t *pair_offsets_dev, uint32_t max_corr_per_pair,
                                 const int32_t *dense_pairs, int n_dense_pairs, float *poses_dev, float *trace_dev);

/* Data derived from compact caches ALONE (not from poses or parameters): a caller that keeps its caches across solves builds them
 * once per set of frames and hands them to btba_solve_batch_zn_aux; btba_solve_batch_zn derives what it needs inside every solve
 * (one pass over all frames each: 2 % of a c3 x 32 solve for the block ranges, 6 % of a masked one for the lists);
 * btba_optimize_frames / _keyed keep both with their frame cache.  All pointers are device pointers and optional (NULL).
 *   block_ranges : float2 [n_frames_total][(Hd / 8) * (Wd / 8)] -- depth range [min, max] of the valid pixels of every 8 x 8 block,
 *                  (+inf, -inf) for a block without a valid depth (Hd, Wd multiples of 8).  The pinhole dense sweep uses it to
 *                  drop blocks that provably project outside the target image before touching their pixels (exact: DESIGN.md 4.2).
 *   valid_lists  : uint32 [n_frames_total][Hd * Wd] -- per frame, the ascending list of the pixels that carry a depth,
 *   valid_counts : int32 [n_frames_total] -- and its length; walked instead of all pixels under BTBA_FLAG_COMPACTION. */
typedef struct btba_zn_aux {
    const float *block_ranges;
    const uint32_t *valid_lists;
    const int32_t *valid_counts;
    const float *corr24;              /* the correspondences as 24-byte records (btba_pack_correspondences24): used INSTEAD of corr_dev, with the
                                         same corr_stride / pair_offsets_dev.  NULL: corr_dev (EntryJ) is read */
} btba_zn_aux;
/* Builders (asynchronous on the workspace stream). */
BTBA_API int btba_zn_block_ranges(btba_workspace *ws, int n_frames_total, int Hd, int Wd, const float *zn_dev, float *ranges_dev);
BTBA_API int btba_zn_valid_lists(btba_workspace *ws, int n_frames_total, int Hd, int Wd, const float *zn_dev, uint32_t *lists_dev, int32_t *counts_dev);
/* Device-resident correspondences without their frame indices.  A pair-major array implies (imgIdx_i, imgIdx_j) of every entry through the
 * segment it lies in, so a batch that STAYS on the device (or the keyed pool of btba_optimize_frames_keyed) can drop those 8 of 32 bytes:
 * the sparse sweep streams the array once per Gauss-Newton iteration and is bound by exactly that stream on feature-only windows and on
 * object-masked frames.  24 bytes per entry, kept in groups of 64 entries as three planes of float2 -- (pos_i.x, pos_i.y)[64],
 * (pos_i.z, pos_j.x)[64], (pos_j.y, pos_j.z)[64] -- so that a wave's loads are contiguous: entry E (counted from the start of the array,
 * E = instance * corr_stride + e) has its k-th float2 at float2 index (E / 64) * 192 + k * 64 + E % 64; entry e of the input is entry e of
 * the output (same offsets, same stride, counted in entries).  corr24_dev must hold 24 * 64 * ceil(n_instances * corr_stride / 64) bytes.
 * An invalid entry (imgIdx_i = 0xFFFFFFFF) keeps its place with the bit pattern 0xFFFFFFFF in pos_i.x --
 * consequently a VALID entry whose pos_i.x has that pattern (one particular NaN) is dropped where the reference would propagate the NaN.
 * The wire format at the boundary stays EntryJ (A1).  order_flag_dev (may be NULL): int on the device, ORed with 1 when a valid entry
 * does not carry the pair of its segment (the array was not pair-major).  Asynchronous on the workspace stream. */
BTBA_API int btba_pack_correspondences24(btba_workspace *ws, int n_instances, int n_frames, const btba_entryj *corr_dev, int64_t corr_stride,
                                         const uint32_t *pair_offsets_dev, uint32_t max_corr_per_pair, float *corr24_dev, int32_t *order_flag_dev);
/* btba_solve_batch_zn with the caches' derived data supplied (aux NULL, or any member NULL: as btba_solve_batch_zn). */
BTBA_API int btba_solve_batch_zn_aux(btba_workspace *ws, const btba_params *params, int n_instances, int n_frames,
                                     int H, int W, const float *K_rowmajor, const float *zn_dev, const btba_zn_aux *aux,
                                     const btba_entryj *corr_dev, int64_t corr_stride,
                                     const uint32_t *pair_offsets_dev, uint32_t max_corr_per_pair,
                                     const int32_t *dense_pairs, int n_dense_pairs, float *poses_dev, float *trace_dev);

/* ---- correspondence RANSAC (the step before correspondences enter BA) ------------
 * Replaces ransacMultiPairGPU (src/cuda/cuda_ransac.cu:1228-1323) as called by SiftManager::runRansacMultiPairGPU
 * (FeatureManager.cpp:659-741): for every frame pair, n_trials 3-point rigid hypotheses ptsA -> ptsB, inlier vote with
 * |ptB - pose ptA| <= dist_thres, the inliers of the best trial.
 *   ptsA_host / ptsB_host : float4 (x, y, z, 1) points of ALL pairs back to back (model frame, as the reference uploads
 *                           them); pair p owns n_pts[p] consecutive points.
 *   samples_host          : NULL, or int32 [n_pairs][n_trials][3] explicit sample indices (the rand_list of
 *                           ransacMultiPairKernel, :1105).  NULL: the reference's generator, RESTATED AND UNVERIFIED -- trial t draws
 *                           round(u (n_pts-1)) three times from cuRAND's XORWOW generator after curand_init(seed, t, 0)
 *                           (ransacEstimateModelKernel, :1154-1161; the reference's literal seed is 0 -- pass seed = 0 for its
 *                           triples).  That stream does not depend on the pair, so it is one table of n_trials x 3 uniforms,
 *                           computed on the host from cuRAND's published algorithm (btba_ransac_reference_uniforms below),
 *                           kept in the workspace and read by the vote kernel.  No cuRAND exists on this side: operators, jumps
 *                           and recurrence are pinned against rocRAND's engine, the four seed constants and the uniform
 *                           conversion rest on the published headers (INTEGRATION.md gives the CUDA snippet that settles it).  With BTBA_RANSAC_DRAW_HASH (btba_ransac_pairs_ex)
 *                           the triples come from a counter hash of (seed, pair, trial, draw) instead: same round(u (n-1))
 *                           shape, but every pair gets its own triples.  Trials with repeated / negative / out-of-range
 *                           indices are skipped (:1164-1165).
 *   inlier_ids_out        : int32, same layout as the points: pair p's ascending inlier indices in its first
 *                           n_inliers_out[p] entries.  best_trial_out[p] = -1 when no trial was usable.
 *   best_pose_out         : may be NULL; float [n_pairs][16] row-major 4x4 of the winning 3-point hypothesis.
 *   trial_counts_out / trial_poses_out : may be NULL; int32 [n_pairs][n_trials], float [n_pairs][n_trials][12] (3x4).
 * Best trial = most inliers, lowest trial id among equals (the reference: whichever thread writes last).
 * Deterministic; synchronous (results valid on return).
 * Hypotheses: btba_ransac_pairs uses BTBA_RANSAC_REFERENCE_SVD -- procrustesKernel (cuda_ransac.cu:998-1103) with the reference's
 * APPROXIMATE 3x3 SVD (McAdams et al., UW-Madison TR1690, pasted into cuda_ransac.cu:48-975) restated operation for operation,
 * including its "R is not valid" failure: per-trial poses, inlier counts and the winner equal the reference's on identical sample
 * triples (pinned against the reference's own functions, tests/test_gpu_ransac.py).  BTBA_RANSAC_HORN (btba_ransac_pairs_ex) is the
 * exact Kabsch optimum by Horn's quaternion method instead: never fails, rejects (near-)collinear samples by the eigenvalue gap;
 * on 3-point samples the reference's approximate SVD is more than 4e-3 away from it in ~5 % of the trials.
 * btba_ransac_pairs_ex also takes device_resident = 1: ptsA / ptsB / samples and every output are DEVICE pointers (n_pts stays
 * on the host), nothing but the 4 (n_pairs + 1)-byte offset table crosses PCIe, and the call is asynchronous on the workspace
 * stream (the host-buffer form spends ~60 % of a tracker-size call in its copies). */
enum { BTBA_RANSAC_REFERENCE_SVD = 0, BTBA_RANSAC_HORN = 1,
       BTBA_RANSAC_DRAW_HASH = 0x100 /* ORed into `hypothesis`: counter-hash triples instead of the restated cuRAND stream */ };
BTBA_API int btba_ransac_pairs_ex(btba_workspace *ws, int hypothesis, int device_resident, int n_pairs, const float *ptsA, const float *ptsB,
                                  const int32_t *n_pts, int n_trials, float dist_thres, const int32_t *samples, uint64_t seed,
                                  int32_t *inlier_ids_out, int32_t *n_inliers_out, int32_t *best_trial_out, float *best_pose_out,
                                  int32_t *trial_counts_out, float *trial_poses_out);
BTBA_API int btba_ransac_pairs(btba_workspace *ws, int n_pairs, const float *ptsA_host, const float *ptsB_host, const int32_t *n_pts,
                               int n_trials, float dist_thres, const int32_t *samples_host, uint64_t seed,
                               int32_t *inlier_ids_out, int32_t *n_inliers_out, int32_t *best_trial_out, float *best_pose_out,
                               int32_t *trial_counts_out, float *trial_poses_out);

/* The reference's RANSAC sample stream as numbers (restated from cuRAND's published headers; unverified against a CUDA run): u_out[3 t + k] = the k-th curand_uniform() after curand_init(seed, t, 0) of
 * cuRAND's XORWOW generator, t = 0 .. n_trials-1 (cuda_ransac.cu:1154-1161); trial t of a pair with n points samples
 * round(u * (n - 1)).  Host-only (no GPU, no workspace): Marsaglia's xorwow recurrence, cuRAND's seed scrambling and its
 * 2^67-step subsequence jump as a GF(2) matrix power (bundletrack_amd/csrc/btba_xorwow.hpp).  BTBA_EINVAL on bad arguments. */
BTBA_API int btba_ransac_reference_uniforms(uint64_t seed, int n_trials, float *u_out);

/* ---- descriptor matching (the step before RANSAC) ---------------------------------------------------------------
 * Replaces SiftManager::findCorresbyNN / findCorresbyNNMultiPair (src/FeatureManager.cpp:247-437: OpenCV's brute-force
 * kNN matcher, pruneMatches, collectMutualMatches) for many frame pairs in one call.  For every pair (A, B), A first:
 *   1. kNN A -> B: for every keypoint i of A the min(k, nB) keypoints of B nearest in L2, ascending (d2, index in B).
 *   2. Gate: walk i's neighbours in that order and keep the FIRST j that passes, then stop.  Both keypoints are rounded
 *      with roundf (halves away from zero) and must land in 0 <= u < W, 0 <= v < H; the camera-space points there (the
 *      ones btba_depth_to_normals writes to xyz_dev, bit for bit) must both have z >= 0.1 (params.min_z); points
 *      (R p + t) and normals (R n) move into the model frame with the frames' poses; reject when |PA - PB| > max_dist
 *      or dot(normalize(nA), normalize(nB)) < cos_max_normal (a zero normal stays zero).  Pairs with |idA - idB| == 1
 *      use the *_neighbor thresholds, all others the *_no_neighbor ones.
 *   3. With params.mutual: the same with the roles swapped (B -> A).
 *   4. Output: the A -> B matches in ascending A index, then the B -> A matches in ascending B index.  No consistency
 *      filter and no de-duplication (the reference's collectMutualMatches has neither): RANSAC's triples index this list.
 * Distance arithmetic (fixed, so that a CPU restatement reproduces the output bit for bit):
 *   na = sum_k a_k^2 and dot = sum_k a_k b_k are each ONE sequential fmaf chain over k = 0 .. D-1 from +0;
 *   d2 = fmaf(-2, dot, na + nb), replaced by +0 unless it is > 0 (negative, -0 and NaN become +0);
 *   rank on (d2, train index); dist = sqrtf(d2).  d2 is symmetric, B -> A ranks the same numbers.
 * Gate arithmetic: uncontracted fp32 in the order written: P_r = ((T_r0 x + T_r1 y) + T_r2 z) + T_r3,
 * N_r = (T_r0 nx + T_r1 ny) + T_r2 nz, |PA - PB| = sqrtf((dx dx + dy dy) + dz dz), normalize = n / sqrtf(|n|^2) when |n|^2 > 0.
 *
 *   desc_dev[f]   : device float [n_kpts[f]][D] descriptors, D a multiple of 4, 4 .. 512
 *   kpts_dev[f]   : device float2 [n_kpts[f]] keypoints (x, y) in full-resolution pixels
 *   n_kpts[f]     : 0 .. 8192 (host)
 *   depth_dev[f], normal_dev[f] : device float [H*W] and float4 [H*W] maps of the frame (btba_depth_to_normals' format)
 *   poses         : host float [n_frames][16] row-major camera -> model;  frame_ids: host int32 [n_frames] (Frame::_id)
 *   pairs         : host int32 [n_pairs][2] frame indices (A first, A != B); frames may belong to many windows
 *   matches_out   : btba_match records of all pairs back to back: pair p starts at sum_{q<p} n_out[q].  Capacity: the
 *                   bound of btba_match_capacity, sum (nA + nB) (sum nA without mutual)
 *   ptsA_model_out / ptsB_model_out : NULL, or float4 (x, y, z, 1) model-frame points of every match, in the same layout:
 *                   exactly what btba_ransac_pairs_ex takes (the arithmetic of the host transform around it)
 *   n_out         : host int32 [n_pairs], valid on return
 * device_resident = 1: matches_out and ptsA/B_model_out are device pointers; 0: host pointers.  Synchronous on the
 * workspace stream.  Scratch is grow-only in the workspace. */
typedef struct btba_match_params {
    int32_t k;                              /* neighbours per query, 1 .. 8 (default 5) */
    int32_t mutual;                         /* 1 (default): also match B -> A */
    float max_dist_neighbor;                /* 0.03 m  (config_ycbineoat.yml feature_corres) */
    float cos_max_normal_neighbor;          /* (float)cos(45 / 180 pi) */
    float max_dist_no_neighbor;             /* 0.02 m */
    float cos_max_normal_no_neighbor;       /* (float)cos(45 / 180 pi) */
    float min_z;                            /* 0.1 m: camera-space z a matched point needs */
} btba_match_params;

typedef struct btba_match {                 /* 40 bytes */
    int32_t idx_a, idx_b;                   /* keypoint indices in A and in B */
    float dist;                             /* descriptor distance sqrtf(d2) */
    int32_t dir;                            /* 0: found A -> B, 1: found B -> A */
    float ptA_cam[3], ptB_cam[3];           /* camera-space points at the rounded keypoints */
} btba_match;

BTBA_API void btba_match_params_default(btba_match_params *p);
/* Validates every host-side argument of btba_match_pairs (BTBA_EINVAL: params NULL, k outside 1..8, n_frames < 1, H or W < 1,
 * D not a multiple of 4 or outside 4..512, n_kpts NULL or a count outside 0..8192, n_pairs < 0, pairs NULL, a pair with A == B or
 * an index out of range) and returns the output capacity the call needs in *capacity_out.  Host-only: no GPU, no workspace. */
BTBA_API int btba_match_capacity(const btba_match_params *params, int n_frames, int H, int W, int D, const int32_t *n_kpts,
                                 int n_pairs, const int32_t *pairs, int64_t *capacity_out);
BTBA_API int btba_match_pairs(btba_workspace *ws, const btba_match_params *params, int device_resident, int n_frames, int H, int W,
                              const float *K_rowmajor, const float *const *desc_dev, int D, const float *const *kpts_dev,
                              const int32_t *n_kpts, const float *const *depth_dev, const float *const *normal_dev, const float *poses,
                              const int32_t *frame_ids, int n_pairs, const int32_t *pairs,
                              btba_match *matches_out, float *ptsA_model_out, float *ptsB_model_out, int32_t *n_out);

/* ---- frame ingest (what makes a frame's device maps from its two images) ------------------------------------------
 * Replaces the body of Frame's constructor after the two imreads (src/Frame.cpp:45-89 with Utils::readDepthImage,
 * src/Utils.cpp:50-69) for many frames in one call: the depth decode, Frame::updateColorGPU, Frame::processDepth and
 * Frame::depthToCloudAndNormals.  _gray is not produced (the reference never reads it).  Every rule is exact, so a CPU
 * restatement reproduces the decode and the colour bit for bit, and the depth chain and the normals equal the per-frame calls':
 *   Decode, depth_format 0: for the code u, d = (float)((double)(float)u * 0.001): the product in double, rounded to float once.
 *       The result is 0 when (double)d < 0.1.  That is exactly u < 100 -> 0: code 100 gives 0.1f, the smallest float above
 *       0.1, and is kept.  (u * 0.001f, the product in float, differs from it in the last bit for 38 850 of the 65 536 codes.)
 *   Decode, depth_format 1: the floats pass through unchanged; the call is then a batched btba_process_depth +
 *       btba_depth_to_normals.
 *   Colour: pixel p of the BGR image (bytes 3p, 3p + 1, 3p + 2) -> (B, G, R, 0), Frame::updateColorGPU.
 *   Depth chain and normals: depth_out is btba_process_depth of the decoded depth with the six parameters below; normal_out and
 *       xyz_out are btba_depth_to_normals(..., xyz) of depth_out with the same K (the same device functions, the same Kinv):
 *       bit for bit what those two calls give frame by frame.
 *
 *   depth_in_dev[f]      : device uint16 [H*W] (2-byte aligned; format 0) or device float [H*W] (format 1)
 *   bgr_in_dev           : NULL, or [f] device uint8 [H*W*3] (entries may be NULL), cv::imread's layout; any alignment (a
 *                          4-byte-aligned image is read a dword at a time)
 *   depth_out_dev[f]     : device float [H*W]: the processed depth (Frame::_depth_gpu)
 *   normal_out_dev[f]    : device float4 [H*W], 16-byte aligned (Frame::_normal_gpu; btba_depth_to_normals' format)
 *   color_out_dev        : NULL, or [f] device uchar4 [H*W], 4-byte aligned (entries NULL where bgr_in is NULL) (Frame::_color_gpu)
 *   depth_raw_out_dev    : NULL, or [f] device float [H*W] (entries may be NULL): the decoded, unfiltered depth (Frame::_depth_raw)
 *   xyz_out_dev          : NULL, or [f] device float4 [H*W], 16-byte aligned (entries may be NULL): camera-space points, w = 1
 *                          (zeros where depth_out < 0.1): the contents of Frame::_cloud together with the normals
 * Asynchronous on the workspace stream: no host synchronisation, no scratch, and no host memory is read after the call returns
 * (frames go in chunks of BTBA_INGEST_CHUNK whose pointers travel as kernel arguments; two launches per chunk).
 * BTBA_EINVAL, decided before the first launch: NULL ws, params, K_rowmajor, depth_in_dev, depth_out_dev or normal_out_dev, or a
 * NULL entry in one of those three tables; n_frames < 1, H < 1 or W < 1; depth_format outside 0 .. 1; btba_process_depth's limits
 * (a negative radius, erode_radius + 2 bf_radius > 16, sigma_d or sigma_r not > 0); a misaligned depth code map, normal, xyz or
 * colour output; a colour output entry without its BGR input; any output of a frame that overlaps that frame's depth input. */
#define BTBA_INGEST_CHUNK 32     /* frames per launch */
typedef struct btba_ingest_params {
    int32_t depth_format;            /* 0 (default): uint16 codes, as cv::imread(path, CV_16UC1) gives them; 1: float32 metres, taken as they are */
    int32_t erode_radius;            /* btba_process_depth's six, same defaults: 1, 0.001, 0.8 */
    float erode_diff, erode_ratio;
    int32_t bf_radius;               /* 2, 2, 100000 */
    float sigma_d, sigma_r;
} btba_ingest_params;
BTBA_API void btba_ingest_params_default(btba_ingest_params *p);
BTBA_API int btba_ingest_frames(btba_workspace *ws, const btba_ingest_params *params, int n_frames, int H, int W,
                                const float *K_rowmajor, const void *const *depth_in_dev, const uint8_t *const *bgr_in_dev,
                                float *const *depth_out_dev, float *const *normal_out_dev, uint8_t *const *color_out_dev,
                                float *const *depth_raw_out_dev, float *const *xyz_out_dev);

/* ---- mask propagation (where a frame's object mask comes from) ---------------------------------------------------
 * Replaces transductive-vos.pytorch/run_video.py around its backbone: rgb_normalize (:81,113-114), prepare_first_frame (:68-82),
 * lib/predict.py::predict with sample_frames and get_spatial_weight (:11-59, :62-78, :118-134), the one-hot history entry (:145)
 * and the upsampled arg-max mask (:151-155).  The backbone is the caller's torch model or btba_vos_features (below): it maps
 * btba_vos_inputs' output to features float [C][Hd][Wd], Hd = ceil(H / 8), Wd = ceil(W / 8).  The mask btba_vos_masks writes is what
 * btba_apply_masks takes.
 *
 * btba_vos_sample_frames (host only; no GPU, no workspace): the history indices predict reads for target frame frame_idx >= 1
 * (frame 0 is the annotated one) and how many of them, counted from the end, take sigma_dense:
 *   frame_idx <= ref_num :  0 .. frame_idx - 1
 *   otherwise            :  trunc(np.linspace(ref_start, ref_end, ref_num - (continuous_frames - 1))), then the continuous_frames - 1
 *                           frames before the target, with ref_end = frame_idx - continuous_frames, ref_start = max(ref_end - range, 0).
 *                           linspace is numpy's: in double, element i = (double)i * step + ref_start with step = (ref_end - ref_start) /
 *                           (n - 1), product and sum rounded separately, the last element ref_end itself; one element = ref_start.
 *   n_dense = n for frame_idx <= sparse_after, else min(continuous_frames, n): the last FOUR selected frames take the dense sigma
 *   although only three of them are the contiguous ones (predict:48-55; kept, the scores depend on it).
 *   idx_out needs room for ref_num entries.  EINVAL: NULL arguments, frame_idx < 1, or parameters outside: continuous_frames >= 1,
 *   max(1, continuous_frames - 1) <= ref_num <= BTBA_VOS_MAX_REF, range >= 0, sparse_after >= 0, both sigmas > 0, temperature finite.
 *
 * btba_vos_propagate: n_items independent videos in one call.  Item b has n_ref[b] reference frames (their pointers are consecutive
 * in the two flat tables, item after item), of which the last n_dense[b] take sigma_dense and the others sigma_sparse.  With
 * k = (r, p) a reference and a position in it, q a target position, (py, px) = (p / Wd, p % Wd):
 *   s[k,q]    = temperature * sum_c ref_r[c,p] * tgt[c,q]                     fp32 products and sums (fp32-input MFMA: an fma chain over c)
 *   P[k,q]    = exp(s[k,q] - m[q]) / sum_k' exp(s[k',q] - m[q]),  m[q] = max_k' s[k',q]      ONE softmax over all references' positions
 *   w[k,q]    = exp(-((py-qy)^2 + (px-qx)^2) / sigma(r)^2)                    applied after the softmax, not renormalised
 *   pred[c,q] = sum_k label_r[c,p] * P[k,q] * w[k,q]
 * and, where onehot_out_dev is given, onehot[c,q] = 1 for the lowest c that attains max_c pred[c,q], else 0 (run_video.py:145).
 * The similarity matrix and the weight tables are never formed: an online softmax over key tiles, the keys split over workgroups
 * and the splits merged in a fixed order without atomics, so a call returns the same bits every time and an item's bits do not
 * depend on the batch around it.  Against the fp64 evaluation of the formulas the error is that of the fp32 logits; the bars the
 * tests hold it to are measured from the reference's own fp32 run.
 *   ref_feat_dev[k]   : device float [C][Hd*Wd] (the backbone's output as it is)
 *   ref_label_dev[k]  : device float [d][Hd*Wd] (btba_vos_first_labels' output for frame 0, one-hot afterwards)
 *   target_dev[b]     : device float [C][Hd*Wd]
 *   pred_out_dev[b]   : device float [d][Hd*Wd]
 *   onehot_out_dev    : NULL, or [b] device float [d][Hd*Wd] (entries may be NULL)
 * Asynchronous on the workspace stream; no host memory is read after the call returns (items go in chunks whose pointers travel as
 * kernel arguments; two launches per chunk).  Scratch: 16 (2 + d) Hd Wd floats per item in the workspace.
 * BTBA_EINVAL, decided before any GPU work: NULL ws, params or table, a NULL or misaligned (4 bytes) entry; n_items < 1; C not a
 * multiple of 8 in 8 .. BTBA_VOS_MAX_CHANNELS; d outside 2 .. BTBA_VOS_MAX_CLASSES; Hd or Wd < 1 or Hd*Wd > BTBA_VOS_MAX_POSITIONS;
 * n_ref[b] outside 1 .. BTBA_VOS_MAX_REF; n_dense[b] outside 0 .. n_ref[b]; parameters outside btba_vos_sample_frames' limits.
 *
 * btba_vos_first_labels: the one-hot of a uint8 [H][W] label image (classes 0 .. d-1; another value belongs to no class) taken
 * bilinearly to [d][Hd][Wd], Hd = ceil(H / 8), Wd = ceil(W / 8).  btba_vos_masks: pred [d][Hd][Wd] taken bilinearly to H x W and the
 * arg-max class (lowest on ties) written as uint8 [H][W]; the d x H x W image is never stored.  Both interpolate as torch's
 * interpolate(mode='bilinear', align_corners=False) does, all in fp32: src = (float)in / (float)out * (dst + 0.5f) - 0.5f, below 0 -> 0;
 * i0 = (int)src, i1 = i0 + (i0 < in - 1), w1 = src - i0, w0 = 1 - w1; value = wy0 (wx0 v00 + wx1 v01) + wy1 (wx0 v10 + wx1 v11).
 * EINVAL: NULL pointers, sizes < 1, d outside 2 .. BTBA_VOS_MAX_CLASSES, Hd*Wd > BTBA_VOS_MAX_POSITIONS.
 *
 * btba_vos_inputs: bgr_dev[f] device uint8 [H*W*3] (cv::imread's layout) -> rgb_out_dev float [n_frames][3][H][W], planes R, G, B:
 * ((float)v / 255.0f - mean) / std in fp32 with mean (0.485, 0.456, 0.406), std (0.229, 0.224, 0.225).  EINVAL: NULL ws, table,
 * entry or output, n_frames, H or W < 1. */
#define BTBA_VOS_MAX_REF 32
#define BTBA_VOS_MAX_CLASSES 16
#define BTBA_VOS_MAX_CHANNELS 512
#define BTBA_VOS_MAX_POSITIONS 65536
typedef struct btba_vos_params {
    int32_t ref_num;                 /* 9: reference frames sampled per target */
    int32_t range;                   /* 40: how far back the sparse references reach */
    float sigma_dense, sigma_sparse; /* 8, 21: the Gaussian's sigma in grid cells */
    float temperature;               /* 1 */
    int32_t continuous_frames;       /* 4: references that take sigma_dense once frame_idx > sparse_after */
    int32_t sparse_after;            /* 15 */
} btba_vos_params;
BTBA_API void btba_vos_params_default(btba_vos_params *p);
BTBA_API int btba_vos_sample_frames(const btba_vos_params *params, int frame_idx, int32_t *idx_out, int32_t *n_out, int32_t *n_dense_out);
BTBA_API int btba_vos_first_labels(btba_workspace *ws, int H, int W, int d, const uint8_t *label_dev, float *labels_out_dev);
BTBA_API int btba_vos_propagate(btba_workspace *ws, const btba_vos_params *params, int n_items, int C, int d, int Hd, int Wd,
                                const int32_t *n_ref, const int32_t *n_dense, const float *const *ref_feat_dev,
                                const float *const *ref_label_dev, const float *const *target_dev, float *const *pred_out_dev,
                                float *const *onehot_out_dev);
BTBA_API int btba_vos_masks(btba_workspace *ws, int d, int Hd, int Wd, int H, int W, const float *pred_dev, uint8_t *mask_out_dev);
BTBA_API int btba_vos_inputs(btba_workspace *ws, int n_frames, int H, int W, const uint8_t *const *bgr_dev, float *rgb_out_dev);

/* ---- the segmentation backbone (between btba_vos_inputs and btba_vos_propagate) ---------------------------------------
 * transductive-vos.pytorch/modeling/network.py::VOSNet on modeling/backbone/resnet.py with model.eval(), as run_video.py:167-180
 * runs it: rgb float [n][3][H][W] (what btba_vos_inputs writes) -> features float [n][256][Hd][Wd], Hd = ceil(H / 8), Wd = ceil(W / 8)
 * (what btba_vos_propagate takes).  fp32 operands with fp32 accumulation throughout; no reduced precision.
 *
 * The net:
 *   stem          conv 7 x 7, stride 2, pad 3, 3 -> 64, no bias; batch norm; relu; max pool 3 x 3, stride 2, pad 1 (padding never
 *                 wins: torch pads with -inf).
 *   layer1 .. 4   layers[s] blocks of planes 64 / 128 / 256 / 256 with strides 1 / 2 / 1 / 1 (layer4 is NOT torchvision's: 256 planes
 *                 at stride 1).  Only a layer's first block carries its stride; it has a downsample (conv 1 x 1 with that stride,
 *                 batch norm) on the shortcut where the stride is not 1 or the width changes.
 *   bottleneck    conv 1 x 1 -> bn -> relu -> conv 3 x 3 (stride, pad 1) -> bn -> relu -> conv 1 x 1 (to 4 x planes) -> bn, + shortcut, relu.
 *   basic         conv 3 x 3 (stride, pad 1) -> bn -> relu -> conv 3 x 3 (pad 1) -> bn, + shortcut, relu.
 *   tail          bottleneck nets only: adjust_dim, conv 1 x 1, 1024 -> 256, no bias; bn256; no relu.  A basic net ends at layer4.
 *   batch norm    inference mode, eps = bn_eps: scale = weight / sqrt(running_var + eps), shift = bias - running_mean * scale,
 *                 in fp64 on the host, rounded once; y = conv * scale + shift in fp32 (one fmaf), then the shortcut is added, then relu.
 *   convolution   a tap outside the image contributes 0.  Output size (in + 2 pad - k) / stride + 1, integer division.
 *   summation     every convolution output element is ONE fp32 fmaf chain over k = (ky, kx, c_in), in that order with c_in fastest,
 *                 from 0 (v_mfma_f32_32x32x2_f32 behind the stem, fmaf in the stem): no split of K.  The order does not depend on
 *                 the grid position, the batch, the frame's place in it or the pass, so a frame gives the same bits alone, anywhere
 *                 in a batch and in any pass.
 * The widths are the reference's.  resnet18 is block 0 with layers 2, 2, 2, 2; resnet50 block 1 with 3, 4, 6, 3 (the default, as
 * run_video.py's); resnet101 block 1 with 3, 4, 23, 3.
 *
 * Weights: n_layers records of host arrays in PyTorch's own layouts, weight [C_out][C_in][k][k] and four [C_out] arrays, in forward
 * order: the stem (backbone.0, backbone.1); for layer s = 1 .. 4 (backbone.{3 + s}) and each of its blocks in turn conv1 + bn1,
 * conv2 + bn2, for a bottleneck conv3 + bn3, and where the block has one downsample.0 + downsample.1; for a bottleneck net last
 * adjust_dim + bn256.  btba_vos_net_layer_count gives n_layers for a configuration (-1 for a bad one).
 * btba_vos_net_model_create checks the configuration and every array, re-lays each weight to [K][C_out] once, folds the batch norms
 * and uploads.  It is the one call here that allocates and waits.  A model belongs to the workspace it was created with and must be
 * destroyed before it.
 * btba_vos_features: asynchronous on the workspace stream, no host wait, no allocation once the workspace scratch has grown.  Frames
 * are worked in passes of at most BTBA_VOS_NET_PASS_PIXELS input pixels (a larger single frame is a pass of its own): the scratch is
 * four NHWC buffers, each of the widest layer's output per frame of a pass (64 ceil(H / 2) ceil(W / 2) floats behind the stem or 256
 * ceil(H / 4) ceil(W / 4) behind a bottleneck layer1, whichever is larger: about 16 H W).  n_frames == 0 is success without a launch; the pointers may then be NULL.
 * BTBA_EINVAL, decided before any GPU work.  create: NULL ws, config, layers or out; block not 0 or 1; layers[i] outside 1 ..
 * BTBA_VOS_NET_MAX_BLOCKS; bn_eps not finite or < 0; n_layers not btba_vos_net_layer_count(config); a NULL array in a record; a
 * non-finite value; running_var + bn_eps <= 0.  features: NULL ws or model; n_frames < 0; H or W outside 1 .. BTBA_VOS_NET_MAX_SIZE;
 * with n_frames > 0 a NULL pointer or one not aligned to 16 bytes; a model created with another workspace.  out_size: NULL outputs,
 * H or W outside 1 .. BTBA_VOS_NET_MAX_SIZE. */
#define BTBA_VOS_NET_BASIC 0
#define BTBA_VOS_NET_BOTTLENECK 1
#define BTBA_VOS_NET_MAX_BLOCKS 64
#define BTBA_VOS_NET_MAX_SIZE 4096
#define BTBA_VOS_NET_PASS_PIXELS (1 << 20)
typedef struct btba_vos_net_config {
    int32_t block;                   /* 1: 0 BasicBlock, 1 Bottleneck */
    int32_t layers[4];               /* 3, 4, 6, 3: blocks of layer1 .. layer4 */
    float bn_eps;                    /* 1e-5 */
} btba_vos_net_config;
typedef struct btba_vos_net_layer {
    const float *weight;             /* the convolution's, [C_out][C_in][k][k] */
    const float *bn_weight, *bn_bias, *running_mean, *running_var;   /* the batch norm's behind it, [C_out] each */
} btba_vos_net_layer;
typedef struct btba_vos_net_model btba_vos_net_model;
BTBA_API void btba_vos_net_config_default(btba_vos_net_config *c);
BTBA_API int btba_vos_net_layer_count(const btba_vos_net_config *config);
BTBA_API int btba_vos_net_model_create(btba_workspace *ws, const btba_vos_net_config *config, const btba_vos_net_layer *layers, int n_layers,
                                       btba_vos_net_model **out);
BTBA_API void btba_vos_net_model_destroy(btba_vos_net_model *model);
BTBA_API int btba_vos_net_out_size(int H, int W, int32_t *Hd, int32_t *Wd);
BTBA_API int btba_vos_features(btba_workspace *ws, const btba_vos_net_model *model, int n_frames, int H, int W, const float *rgb_dev,
                               float *features_out_dev);

/* ---- foreground-mask segmentation (the first step of every frame) ------------------------------------------------
 * Replaces Frame::segmentationByMaskFile minus the PNG read (src/Frame.cpp:236-373, called first by Bundler::processNewFrame,
 * src/Bundler.cpp:80,84) for many frames in one call.  Every rule is exact integer logic, so a CPU restatement reproduces the
 * output bit for bit:
 *   M0, plain path (largest_component_hull = 0, the shipping YCBInEOAT configuration): M0 = (mask != 0).
 *   M0, hull path (largest_component_hull = 1, the reference's "data_dir contains NOCS"): the 8-connected components of
 *       (mask != 0); the one with the most pixels wins, ties to the one whose first pixel in raster (row-major) order comes first
 *       (how OpenCV and scipy.ndimage.label number components; the reference breaks ties by the iteration order of an
 *       unordered_map, which is unspecified).  M0(x, y) = 1 iff the integer point (x, y) lies in the CLOSED convex hull of the
 *       winner's pixel coordinates, decided with integer cross products; a one-point hull or a segment sets its lattice points.
 *       An empty mask gives M0 = 0.
 *   Dilation: M(x, y) = OR of M0 over the dilate x dilate square centred at (x, y); pixels outside the image count as 0 (OpenCV's
 *       default dilation border).
 *   Invalidation: where M = 0, depth = 0, normal = (0, 0, 0, 0), colour = (0, 0, 0, 0); where M = 1 every map stays bit for bit
 *       as it was.  (The reference's updateNormalGPU also zeroes normals inside the mask where (double) z <= 0.1.  For a float z
 *       that holds exactly when z < 0.1f, 0.1f being the smallest float above 0.1: the pixels btba_depth_to_normals already
 *       gives zero normals, CC.z < 0.1f.)
 *   ROI: roi_out[f] = (umin, umax, vmin, vmax) over the pixels with M = 1 as floats, started from the reference's
 *       (9999, 0, 9999, 0) (Frame.cpp:359): (9999, 0, 9999, 0) for an empty mask.
 * Deliberate differences from the reference:
 *   - cv::fillConvexPoly rounds span ends and rasterises the outline, so it may also paint pixels whose centres lie up to half
 *     a pixel outside the hull; the rule above does not.  Unmeasured (no OpenCV to compare with); after the dilation any
 *     difference can only sit on the outer boundary of the final mask.
 *   - the reference's _fg_mask keeps dilated grey values; mask_out is 0 / 1.  Only zero against non-zero is ever read
 *     (Frame.cpp:349,364; Bundler.cpp:389).
 *
 *   mask_dev[f]     : device uint8 [H*W], nonzero = foreground (as imread gives it)
 *   depth_dev[f]    : device float [H*W], zeroed outside the final mask, in place
 *   normal_dev[f]   : device float4 [H*W] (btba_depth_to_normals' format, 16-byte aligned), zeroed outside, in place
 *   color_dev       : NULL, or [f] device uchar4 [H*W] (entries may be NULL), zeroed outside, in place
 *   mask_out_dev    : NULL, or [f] device uint8 [H*W] (entries may be NULL): the final mask as 0 / 1; must not alias mask_dev
 *   roi_out         : NULL, or host float [n_frames][4].  With roi_out the call is synchronous; without, it is asynchronous
 *                     on the workspace stream (no host memory is read after it returns).
 * Scratch (labels, counts, row extents, hull) is grow-only in the workspace.  BTBA_EINVAL: ws or params NULL, dilate even or
 * outside 1..15, n_frames < 1, H or W < 1, H * W >= 2^31 (the argmax key packs a 32-bit pixel index), NULL mask_dev /
 * depth_dev / normal_dev or any of their entries, a misaligned normal map, a mask_out entry equal to its mask entry. */
typedef struct btba_mask_params {
    int32_t largest_component_hull;  /* 0 (default): YCBInEOAT path; 1: NOCS path (largest 8-connected component -> convex hull -> fill) */
    int32_t dilate;                  /* side of the square dilation element, odd, 1 .. 15 (default 5; 1 = no dilation) */
} btba_mask_params;
BTBA_API void btba_mask_params_default(btba_mask_params *p);
BTBA_API int btba_apply_masks(btba_workspace *ws, const btba_mask_params *params, int n_frames, int H, int W,
                              const uint8_t *const *mask_dev, float *const *depth_dev, float *const *normal_dev,
                              uint8_t *const *color_dev, uint8_t *const *mask_out_dev, float *roi_out);

/* ---- detector front end (the step between the mask and the matcher) ----------------------------------------------
 * Replaces the image and point arithmetic of Lfnet::detectFeature (src/FeatureManager.cpp:811-908, called by
 * Bundler::processNewFrame, src/Bundler.cpp:103-117) with rot_deg = 0 (the only value the reference passes): the masked colour
 * image cropped to the ROI, zero-padded into a square and resized to S x S (S = out_size, 400 in the reference), the grey float
 * image the LF-Net server makes of it (lf-net-release/run_server.py:160-165), and the detector's keypoints mapped back to
 * full-resolution pixels.  The detector itself stays with the caller.  Every rule is exact integer or fp32 arithmetic, so a CPU
 * restatement reproduces the output bit for bit:
 *   Crop: roi = (umin, umax, vmin, vmax) as btba_apply_masks writes it (integral floats).  Wc = (int)(umax - umin),
 *       Hc = (int)(vmax - vmin) (column umax and row vmax are left out, as in the reference), side = max(Wc, Hc).
 *       I(y, x) = colour(vmin + y, umin + x) for x < Wc, y < Hc, else (0, 0, 0): the padding goes right and below.  Channels are
 *       the B, G, R bytes of the uchar4 colour map (Frame::updateColorGPU's layout); the fourth byte is ignored.
 *   Resize (cv::resize INTER_LINEAR, OpenCV's fixed-point path for 8-bit images), inv = (double)S / side, scale = 1.0 / inv:
 *       per output column dx: fx = (float)((dx + 0.5) * scale - 0.5) in double, uncontracted; sx = floor(fx); fx -= sx in float;
 *       sx < 0 -> fx = 0, sx = 0; sx >= side - 1 -> fx = 0, sx = side - 1.  a0 = rint_even((1.f - fx) * 2048),
 *       a1 = rint_even(fx * 2048); h = I[sx] * a0 + I[sx + 1] * a1 (int; the second tap is not read when sx = side - 1, a1 = 0).
 *       Per output row dy: fy, sy the same, but fy is NOT zeroed at the border: the two source rows are clamp(sy, 0, side - 1) and
 *       clamp(sy + 1, 0, side - 1), b0 = rint_even((1.f - fy) * 2048), b1 = rint_even(fy * 2048).
 *       Vertical combine, the SIMD form (VResizeLinearVec_32s8u, which an x86 build applies to nearly every pixel):
 *           out = sat_u8((((h0 >> 4) * b0 >> 16) + ((h1 >> 4) * b1 >> 16) + 2) >> 2).
 *       OpenCV's scalar form, (h0 * b0 + h1 * b1 + (1 << 21)) >> 22, can differ from it by one level; which form the reference's
 *       OpenCV applies to a given pixel depends on its version and SIMD dispatch.  UNMEASURED (no OpenCV to compare with).
 *       side == S is a plain copy (the rule gives one).  side == 2 S is INTER_AREA, as cv::resize switches it:
 *           out = (I(2y, 2x) + I(2y, 2x + 1) + I(2y + 1, 2x) + I(2y + 1, 2x + 1) + 2) >> 2   (only a ROI 2 S wide or high).
 *   Grey: OpenCV 4's RGB2GRAY on the BGR bytes, as the server calls it: g = (9798 * B + 19235 * G + 3735 * R + 16384) >> 15, then
 *       g / 255.0f correctly rounded.  OpenCV 3 used 14-bit weights (4899, 9617, 1868); which one the reference's server ran is
 *       unknown.
 *   Transform (btba_detector_transform): s = (float)S / (float)side; forward F = [[s, 0, 0 - fl(s * umin)], [0, s, 0 - fl(s * vmin)],
 *       [0, 0, 1]] (the product Eigen forms of the scale and translation matrices: -fl(s * umin), +0 for umin = 0).  Backward: Eigen's
 *       3 x 3 cofactor inverse of F in fp32: det = fl(s * s), invdet = fl(1 / det), r00 = r11 = fl(s * invdet),
 *       r02 = fl(fl(fl(s * umin) * s) * invdet), r12 likewise with vmin, r22 = fl(det * invdet), the other four entries +0 (Eigen's
 *       may be -0, which changes no keypoint but a -0 input).  fwd and bwd are written row-major.  A keypoint (kx, ky) maps to
 *       (fl(fl(r00 * kx) + r02), fl(fl(r11 * ky) + r12)), uncontracted.  This is what the reference computes on any x86 build: every
 *       term an FMA could fuse with is an exact zero (0 * x, or a cofactor made of zero products), and fl(r00 * kx) + r02 is the sum
 *       of two different products of which Eigen's row sum forms the first before adding the second.
 *
 *   color_dev[f]     : device uchar4 [H * W] (4-byte aligned), the masked colour map (btba_apply_masks leaves it so)
 *   roi_host         : host float [n_frames][4]
 *   bgr_out_dev      : NULL, or device uint8 [n_frames][S][S][3] (4-byte aligned): exactly the bytes the reference sends the server
 *   gray_out_dev     : NULL, or device float [n_frames][S][S] (16-byte aligned): g / 255.0f
 *   kpts_in_dev[f]   : device float2 [n_kpts[f]] in detector pixels (0 <= n_kpts[f] <= 8192; NULL allowed where n_kpts[f] = 0)
 *   kpts_out_dev[f]  : device float2 [n_kpts[f]] in full-resolution pixels, btba_match_pairs' kpts_dev format; may equal
 *                      kpts_in_dev[f] (in place)
 * Both device calls are asynchronous on the workspace stream and read no host memory after they return (frames go in chunks
 * whose pointers and coefficients travel as kernel arguments).  BTBA_EINVAL: NULL ws, params or tables, or a NULL entry in one of
 * them (a NULL kpts entry with n_kpts[f] > 0); a non-integral ROI, Wc < 1 or Hc < 1, or a crop outside the H x W image; out_size
 * not a multiple of 4 in 4 .. 4096; n_frames < 1, H < 1 or W < 1; a misaligned color_dev entry, output or keypoint buffer (float2:
 * 8 bytes); n_kpts[f] outside
 * 0 .. 8192.  btba_detector_transform needs no GPU and no workspace. */
typedef struct btba_detector_params {
    int32_t out_size;                /* S: the detector's square input side (default 400, Lfnet::detectFeature's H_input = W_input) */
} btba_detector_params;
BTBA_API void btba_detector_params_default(btba_detector_params *p);
BTBA_API int btba_detector_transform(const btba_detector_params *params, const float *roi, float *fwd, float *bwd);
BTBA_API int btba_detector_inputs(btba_workspace *ws, const btba_detector_params *params, int n_frames, int H, int W,
                                  const uint8_t *const *color_dev, const float *roi_host, uint8_t *bgr_out_dev, float *gray_out_dev);
BTBA_API int btba_detector_keypoints_to_image(btba_workspace *ws, const btba_detector_params *params, int n_frames, const float *roi_host,
                                              const float *const *kpts_in_dev, const int32_t *n_kpts, float *const *kpts_out_dev);

/* ---- keypoint head (between the detector's two conv nets) ---------------------------------------------------------
 * Replaces the non-learned stage of lf-net-release/run_server.py between its score net and its descriptor net:
 * inference.py::build_multi_scale_deep_detector_3DNMS (:159-241) and build_patch_extraction (:243-262), on det_tools.py
 * (instance_normalization, soft_nms_3d, soft_max_and_argmax_1d, end_of_frame_masks, non_max_suppression,
 * make_top_k_sparse_tensor, extract_keypoints, batch_gather_keypoints, soft_argmax_2d) and spatial_transformer.py::transformer_crop.
 * The two conv nets stay with the caller.  The photo is what btba_detector_inputs writes as grey.  All images are row-major.
 *
 * Stage A, btba_lfnet_heatmaps.  score_dev[s]: device float [n_frames][map_h[s]][map_w[s]], the score maps of scale s for all frames
 * (each scale has its own size; the detector makes them at int(H / s + 0.5)); scale_factors, map_h, map_w: host [S].
 *   per map   mean, var = the mean and the biased variance (tf.nn.moments), accumulated in fp64;
 *             logit = x * inv - mean * inv, inv = 1 / sqrt(var + 1e-3), in fp32 (tf.nn.batch_normalization)
 *   resize    to H x W as TF1's resize_images: src = dst * (in / (float)out); lower tap floor(src), upper min(lower + 1, in - 1);
 *             top = tl + (tr - tl) * fx, bottom = bl + (br - bl) * fx, value = top + (bottom - top) * fy
 *   soft_nms_3d, N(q) = all S scales x the sm_ksize x sm_ksize window of q, cut to the image:
 *             M(q) = max over N(q);  e_s(q) = exp(com_strength * (logit_s(q) - M(q)));  p_s(q) = e_s(q) / (sum over N(q) of e + 1e-6)
 *   soft_max_and_argmax_1d over the S values of a pixel, m = max_s p_s:
 *             heat  = sum_s p_s * (a_s / (sum_s a_s + 1e-8)),                a_s = exp(score_com_strength * (p_s - m))
 *             scale = sum_s scale_factors[s] * (b_s / (sum_s b_s + 1e-8)),   b_s = exp(scale_com_strength * (p_s - m))
 *   max_heatmaps = heat where pad_size <= y < H - pad_size and pad_size <= x < W - pad_size, else 0;  max_scales = scale.
 * Outputs: device float [n_frames][H][W] each.  Two launches for all frames; the main one makes a workgroup tile with its halo
 * in LDS (btba_lfnet.hpp) and writes nothing full-size but the two outputs.  The fp32 summation order is the kernel's own; the
 * tests hold it to bars measured from the reference's fp32 run against fp64.
 *
 * Stage B, btba_lfnet_select: exact on any fp32 heat map float [n_frames][H][W] without NaN.
 *   works = heat < nms_thresh ? 0 : heat;  peak(q) = works(q) > works(r) for all nms_ksize^2 - 1 neighbours r, 0 outside the image
 *   score = heat * peak * (crop_radius frame mask);  tf.nn.top_k(score over the flattened frame, top_k): equal values go to the
 *   lower flat index;  of the chosen positions those that are peaks survive, in raster order.
 * With fewer than top_k positive scores the zero scores fill up from flat index 0 on, so a zero-score peak (one between pad_size and
 * crop_radius) survives if its flat index minus the number of nonzero scores before it is below top_k minus the positive count.
 * Outputs: kpts_xy_dev int32 [n_frames][top_k][2] (x, y; slots past the count are 0) and n_kpts_dev int32 [n_frames].
 *
 * Stage C, btba_lfnet_crops.  photo_dev float [n][H][W]; ori_dev float [n][H][W][2] (cos, sin, as the detector gives them); heat_dev and
 * scales_dev: stage A's outputs; kpts_xy_dev, n_kpts_dev: stage B's.  Per keypoint (kx, ky): s = scales[ky][kx], (c, sn) = ori[ky][kx];
 *   transformer_crop(img, n, (px, py), a b / c d): g_i = -1 + i * (2 / (n - 1)); for row i, column j
 *             x = (a g_j + b g_i) * n / 2 + px,  y = (c g_j + d g_i) * n / 2 + py;  x0 = clamp(floor(x)), x1 = clamp(floor(x) + 1) into
 *             0 .. W - 1, y likewise;  value = (x1 - x)(y1 - y) I[y0][x0] + (x1 - x)(y - y0) I[y1][x0] + (x - x0)(y1 - y) I[y0][x1] +
 *             (x - x0)(y - y0) I[y1][x1] -- the weights from the CLAMPED taps, so a sample outside the image is zero or an odd blend,
 *             not the border pixel (the descriptor was trained on that)
 *   soft_kpts: v = transformer_crop(heat, kp_loc_size, (kx, ky), s 0 / 0 s);  w = do_softmax_kp_refine ? exp(kp_com_strength *
 *             (v - max v)) / (sum + 1e-8) : v;  (dx, dy) = sum w * (g_j, g_i);  kpt = (kx, ky) + (dx, dy) * s * kp_loc_size / 2
 *             (without soft_kpts: kpt = (kx, ky) as floats)
 *   patch   = transformer_crop(photo, patch_size, kpt, s c  -s sn / s sn  s c)
 * Outputs: kpts_out_dev float [n][top_k][2], kpts_scale_out_dev float [n][top_k], kpts_ori_out_dev float [n][top_k][2],
 * patches_out_dev float [n][top_k][patch_size][patch_size]; slots past n_kpts are written as zero.  One wave per keypoint slot.
 *
 * btba_lfnet_keypoints: A, B and C for n_frames in one call without a host wait in between; bit-identical to the three calls.
 * With n_kpts_host non-NULL the counts are copied there and the call waits once at the end; otherwise it is asynchronous on the
 * workspace stream, as the three stages are.  Scratch: 9 H W bytes per frame in the workspace.
 * BTBA_EINVAL, decided before any GPU work: NULL ws, params, pointer or table entry, or one not aligned to 4 bytes; n_frames < 1; H or W
 * outside 1 .. BTBA_LFNET_MAX_SIZE; a map size < 1; S outside 1 .. BTBA_LFNET_MAX_SCALES; sm_ksize or nms_ksize even or outside
 * 1 .. BTBA_LFNET_MAX_KSIZE; top_k outside 1 .. BTBA_LFNET_MAX_TOP_K; pad_size or crop_radius negative, or twice one of them not below
 * min(H, W); patch_size or kp_loc_size outside 2 .. 64. */
#define BTBA_LFNET_MAX_SCALES 16
#define BTBA_LFNET_MAX_KSIZE 31
#define BTBA_LFNET_MAX_TOP_K 2048
#define BTBA_LFNET_MAX_SIZE 8192
typedef struct btba_lfnet_params {
    int32_t sm_ksize;                /* 15: the scale-space soft-max window */
    float com_strength;              /* 3 */
    float score_com_strength;        /* 100 */
    float scale_com_strength;        /* 100 */
    float nms_thresh;                /* 0 */
    int32_t nms_ksize;               /* 5 */
    int32_t top_k;                   /* 500 */
    int32_t pad_size;                /* 16: the detector's own border */
    int32_t crop_radius;             /* 16 */
    int32_t soft_kpts;               /* 1 */
    int32_t kp_loc_size;             /* 9 */
    int32_t do_softmax_kp_refine;    /* 1 */
    float kp_com_strength;           /* 1 */
    int32_t patch_size;              /* 32 */
} btba_lfnet_params;
BTBA_API void btba_lfnet_params_default(btba_lfnet_params *p);
BTBA_API int btba_lfnet_heatmaps(btba_workspace *ws, const btba_lfnet_params *params, int n_frames, int H, int W, int S,
                                 const float *const *score_dev, const int32_t *map_h, const int32_t *map_w, const float *scale_factors,
                                 float *max_heatmaps_dev, float *max_scales_dev);
BTBA_API int btba_lfnet_select(btba_workspace *ws, const btba_lfnet_params *params, int n_frames, int H, int W, const float *heat_dev,
                               int32_t *kpts_xy_dev, int32_t *n_kpts_dev);
BTBA_API int btba_lfnet_crops(btba_workspace *ws, const btba_lfnet_params *params, int n_frames, int H, int W, const float *photo_dev,
                              const float *ori_dev, const float *heat_dev, const float *scales_dev, const int32_t *kpts_xy_dev,
                              const int32_t *n_kpts_dev, float *kpts_out_dev, float *kpts_scale_out_dev, float *kpts_ori_out_dev,
                              float *patches_out_dev);
BTBA_API int btba_lfnet_keypoints(btba_workspace *ws, const btba_lfnet_params *params, int n_frames, int H, int W, int S,
                                  const float *const *score_dev, const int32_t *map_h, const int32_t *map_w, const float *scale_factors,
                                  const float *photo_dev, const float *ori_dev, float *max_heatmaps_dev, float *max_scales_dev,
                                  int32_t *kpts_xy_dev, int32_t *n_kpts_dev, float *kpts_out_dev, float *kpts_scale_out_dev,
                                  float *kpts_ori_out_dev, float *patches_out_dev, int32_t *n_kpts_host);

/* ---- descriptor net (between the keypoint head's crops and the matcher) ---------------------------------------------
 * LF-Net's descriptor net, lf-net-release/models/simple_desc.py::get_model on common/tf_layer_utils.py, in inference: `depth`
 * stride-2 3 x 3 convolutions (1 -> channels -> 2 channels -> ...), each followed by batch norm and the activation, flatten, a
 * fully connected layer to fc_dim with batch norm and the activation, a fully connected layer to out_dim, l2_normalize.  All of it in
 * fp32 with fp32 accumulation (the convolutions from layer 2 on and the fully connected layers on v_mfma_f32_32x32x2_f32, whose result
 * is a k-ordered fmaf chain; layer 1 on the vector ALU), every dot product in ONE fixed k order: a patch's descriptor is the same
 * bits whatever the batch around it, its slot or its frame.
 *
 * The rules:
 *   convolution   TensorFlow's SAME with stride 2 pads asymmetrically: out = ceil(in / 2), total = max((out - 1) * 2 + 3 - in, 0),
 *                 before = total / 2 (integer division) and the rest after.  For an even size nothing is padded before and ONE row
 *                 and ONE column after: output (oy, ox) reads input rows 2 oy .. 2 oy + 2 and columns 2 ox .. 2 ox + 2.
 *                 weights [3][3][C_in][C_out]; the sum runs over (ky, kx, c_in) in that order.
 *   batch norm    folded at model creation, in fp64 on the host and rounded once to fp32:
 *                 scale = gamma / sqrt(moving_variance + bn_eps),  shift = beta + (bias - moving_mean) * scale;
 *                 y = acc * scale + shift.  Without batch norm (NULL moving_*): scale = 1, shift = bias.
 *   activation    0 relu: max(y, 0);  1 leaky relu: y >= 0 ? y : leaky_alpha * y
 *   flatten       (h, w, c): the last convolution's NHWC output as it lies
 *   l2_normalize  x * rsqrt(max(sum x^2, 1e-12)) over a descriptor
 *
 * btba_lfnet_desc_model_create checks the configuration and every array (finite values; moving_variance + bn_eps > 0), folds the batch
 * norms, and uploads the weights in the [K][C_out] layout the kernels' B operand reads (K = 9 C_in or the fully connected layer's
 * inputs).  It is the one call here that allocates and waits.  A model belongs to the workspace it was created with and must be
 * destroyed before it.
 * btba_lfnet_descriptors: patches_dev float [n_frames][slots][P][P] -> desc_dev float [n_frames][slots][out_dim].  n_kpts_dev: int32
 * [n_frames] on the device, the number of leading slots of each frame that hold a patch (values outside 0 .. slots are clamped), or
 * NULL for all.  Slots past the count are written as zero and their work is skipped.  Asynchronous on the workspace stream, no
 * allocation once the workspace scratch has grown, no host wait.  n_frames * slots == 0 is success without a launch (the three device
 * pointers are then not looked at).
 * BTBA_EINVAL, decided before any GPU work.  create: NULL ws, config, weights or out; patch_size outside 8 .. 64 or not divisible by
 * 2^depth; depth outside 1 .. 4; channels not a multiple of 16 in 16 .. 128; fc_dim not a multiple of 16 in 16 .. 1024; out_dim not a
 * multiple of 16 in 16 .. 512; activation not 0 or 1; norm not 0 or 1; leaky_alpha or bn_eps not finite, bn_eps < 0; flatten size
 * (patch_size / 2^depth)^2 * channels * 2^(depth - 1) above 16384; a NULL `weights` array of a used layer; only one of moving_mean and
 * moving_variance given; a non-finite value; moving_variance + bn_eps <= 0.  descriptors: NULL ws, model, patches_dev or desc_dev, or
 * one of the three device pointers not aligned to 4 bytes; n_frames or slots negative; slots above BTBA_LFNET_MAX_TOP_K; n_frames * slots above 2^24; a model created with another workspace. */
#define BTBA_LFNET_DESC_MAX_DEPTH 4
typedef struct btba_lfnet_desc_config {
    int32_t patch_size;              /* 32 */
    int32_t depth;                   /* 3: convolution layers */
    int32_t channels;                /* 64: of layer 1; layer i has channels * 2^i */
    int32_t fc_dim;                  /* 512 */
    int32_t out_dim;                 /* 256 */
    int32_t activation;              /* 0 relu, 1 leaky relu */
    float leaky_alpha;               /* 0.2 */
    int32_t norm;                    /* 0 l2norm, 1 none */
    float bn_eps;                    /* 1e-5: _BATCH_NORM_EPSILON of tf_layer_utils.tf_batch_norm_act */
} btba_lfnet_desc_config;
/* One layer's arrays, host pointers in TensorFlow's own layouts: weights [3][3][C_in][C_out] or [in][out]; the others [C_out].
 * NULL biases = none; NULL moving_mean and moving_variance = no batch norm on the layer (gamma and beta are then not read);
 * NULL gamma = 1, NULL beta = 0. */
typedef struct btba_lfnet_desc_layer {
    const float *weights, *biases, *gamma, *beta, *moving_mean, *moving_variance;
} btba_lfnet_desc_layer;
typedef struct btba_lfnet_desc_weights {
    btba_lfnet_desc_layer conv[BTBA_LFNET_DESC_MAX_DEPTH];     /* SimpleDesc/conv{i+1} and SimpleDesc/bn{i+1}; the first `depth` are read */
    btba_lfnet_desc_layer fc1;                                 /* SimpleDesc/fc1 and SimpleDesc/fc-bn1 */
    btba_lfnet_desc_layer fc2;                                 /* SimpleDesc/fc2: weights and biases (no activation follows) */
} btba_lfnet_desc_weights;
typedef struct btba_lfnet_desc_model btba_lfnet_desc_model;
BTBA_API void btba_lfnet_desc_config_default(btba_lfnet_desc_config *c);
BTBA_API int btba_lfnet_desc_model_create(btba_workspace *ws, const btba_lfnet_desc_config *config, const btba_lfnet_desc_weights *weights,
                                          btba_lfnet_desc_model **out);
BTBA_API void btba_lfnet_desc_model_destroy(btba_lfnet_desc_model *model);
BTBA_API int btba_lfnet_descriptors(btba_workspace *ws, const btba_lfnet_desc_model *model, int n_frames, int slots,
                                    const float *patches_dev, const int32_t *n_kpts_dev, float *desc_dev);

/* ---- detector net (before the keypoint head) ------------------------------------------------------------------------
 * LF-Net's detector net, lf-net-release/models/mso_resnet_detector.py::get_model on common/tf_layer_utils.py, in inference: the grey
 * photo to the per-scale score maps btba_lfnet_heatmaps takes and the orientation map btba_lfnet_crops takes.  photo_dev float
 * [n][H][W] is used as it is (run_server.py normalises the photo into a variable nobody reads).  C = channels, k = ksize; NHWC,
 * fp32 operands with fp32 accumulation; the C -> C convolutions on v_mfma_f32_16x16x4_f32 (a k-ordered fmaf chain), the thin ends
 * (1 -> C, C -> 1, C -> 2) on the vector ALU; every output element is ONE chain over (ky, kx, c_in) in that order, so a frame's
 * results are the same bits whatever the batch, the frame's place in it or the pass.
 *
 * The rules:
 *   convolution   k x k, stride 1, SAME: k / 2 zeros on every side, plus bias.  The zeros pad the tensor AFTER batch norm and
 *                 activation: a tap outside the image contributes 0, not act(shift).
 *   init_conv     1 -> C.
 *   block i       x <- conv2(act(mid-bn(conv1(act(pre-bn(x)))))) + x, i = 1 .. blocks; both convolutions C -> C; the shortcut is
 *                 the block's input before pre-bn.
 *   features      f = act(fin-bn(x))
 *   score map j   h_j = (int)((float)H * (float)(1.0 / s_j) + 0.5f), w_j likewise (fp32, as tf.cast(base_height_f * inv_s + 0.5,
 *                 tf.int32)); f resized to h_j x w_j per channel by TF1's resize_images (stage A's rule above: src = dst * (in /
 *                 (float)out), lower tap floor(src), upper min(lower + 1, in - 1), top / bottom / value lerps in that order); then
 *                 score_conv_j, C -> 1, no activation.  float [n][h_j][w_j].
 *   orientation   ori_conv, C -> 2, then l2_normalize over the two channels: x * rsqrt(max(x0^2 + x1^2, 1e-12)).  float [n][H][W][2].
 *   batch norm    tf.layers.batch_normalization with epsilon bn_eps.  mid-bn is folded into conv1 with its bias at model creation
 *                 as the descriptor net's are (fp64 on the host, rounded once).  pre-bn and fin-bn sit behind the residual sum:
 *                 each is a per-channel pair scale = gamma / sqrt(moving_variance + bn_eps), shift = beta - moving_mean * scale
 *                 (fp64, rounded once), y = x * scale + shift.
 *   activation    0 relu, 1 leaky relu with leaky_alpha (as the descriptor net's)
 *   pad_size      (2 blocks + 2) * (k / 2): the reference's num_conv * (conv_ksize // 2), 16 for the release net; what
 *                 btba_lfnet_params.pad_size takes.
 *   scale factors np.exp(np.linspace(log(max_scale), log(min_scale), num_scales)) in double, largest first; num_scales == 1: [1.0].
 *
 * btba_lfnet_det_model_create checks the configuration and every array, folds the batch norms and uploads.  It is the one call here
 * that allocates and waits.  A model belongs to the workspace it was created with and must be destroyed before it.
 * btba_lfnet_det_scales, btba_lfnet_det_map_size, btba_lfnet_det_map_sizes, btba_lfnet_det_pad_size: host helpers, no GPU work.
 * map_size is the rule above for one side and one scale factor; map_sizes applies it to a model's factors and writes num_scales
 * entries; pad_size returns -1 for a NULL model.
 * btba_lfnet_scores: score_dev is a HOST table of num_scales device pointers, score_dev[j] float [n][h_j][w_j]; ori_dev float
 * [n][H][W][2].  Asynchronous on the workspace stream, no host wait, no allocation once the workspace scratch has grown.  Frames are
 * worked in passes of at most BTBA_LFNET_DET_PASS_PIXELS frame-pixels (a larger single frame is a pass of its own): the scratch is
 * two NHWC buffers of 4 C bytes per pixel of a pass.  n_frames == 0 is success without a launch.
 * BTBA_EINVAL, decided before any GPU work: a NULL argument or table entry, a device pointer not aligned to 4 bytes; channels not a
 * multiple of 16 in 16 .. 64; ksize not 3 or 5; blocks outside 1 .. BTBA_LFNET_DET_MAX_BLOCKS; num_scales outside 1 ..
 * BTBA_LFNET_MAX_SCALES; a scale factor not finite or <= 0; n_frames negative; H, W or a map size outside 1 .. BTBA_LFNET_MAX_SIZE;
 * activation not 0 or 1; leaky_alpha or bn_eps not finite, bn_eps < 0; a NULL `weights` array of a convolution; only one of
 * moving_mean and moving_variance given; a non-finite value; moving_variance + bn_eps <= 0; a model created with another workspace. */
#define BTBA_LFNET_DET_MAX_BLOCKS 8
#define BTBA_LFNET_DET_PASS_PIXELS (1 << 20)
typedef struct btba_lfnet_det_config {
    int32_t channels;                /* 16 */
    int32_t ksize;                   /* 5 */
    int32_t blocks;                  /* 3 */
    int32_t num_scales;              /* 5 */
    double scale_factors[BTBA_LFNET_MAX_SCALES];   /* sqrt(2) .. 1 / sqrt(2), largest first; the first num_scales are read */
    int32_t activation;              /* 1: 0 relu, 1 leaky relu */
    float leaky_alpha;               /* 0.2 */
    float bn_eps;                    /* 1e-5 */
} btba_lfnet_det_config;
/* Host arrays in TensorFlow's layouts under the checkpoint's names (btba_lfnet_desc_layer's NULL rules).  A record that stands for
 * a batch norm alone (pre_bn, fin_bn) is read for gamma, beta, moving_mean and moving_variance only. */
typedef struct btba_lfnet_det_block {
    btba_lfnet_desc_layer pre_bn;    /* ConvOnlyResNet/block-{i}/pre-bn */
    btba_lfnet_desc_layer conv1;     /* .../conv1/{weights [k][k][C][C], biases} and .../mid-bn */
    btba_lfnet_desc_layer conv2;     /* .../conv2/{weights, biases} */
} btba_lfnet_det_block;
typedef struct btba_lfnet_det_weights {
    btba_lfnet_desc_layer init_conv;                              /* ConvOnlyResNet/init_conv: weights [k][k][1][C], biases */
    btba_lfnet_det_block block[BTBA_LFNET_DET_MAX_BLOCKS];        /* block-{i+1}; the first `blocks` are read */
    btba_lfnet_desc_layer fin_bn;                                 /* ConvOnlyResNet/fin-bn */
    btba_lfnet_desc_layer score_conv[BTBA_LFNET_MAX_SCALES];      /* score_conv_{j}: weights [k][k][C][1], biases [1] */
    btba_lfnet_desc_layer ori_conv;                               /* ori_conv: weights [k][k][C][2], biases [2] */
} btba_lfnet_det_weights;
typedef struct btba_lfnet_det_model btba_lfnet_det_model;
BTBA_API void btba_lfnet_det_config_default(btba_lfnet_det_config *c);
BTBA_API int btba_lfnet_det_scales(double min_scale, double max_scale, int num_scales, double *out);
BTBA_API int btba_lfnet_det_model_create(btba_workspace *ws, const btba_lfnet_det_config *config, const btba_lfnet_det_weights *weights,
                                         btba_lfnet_det_model **out);
BTBA_API void btba_lfnet_det_model_destroy(btba_lfnet_det_model *model);
BTBA_API int btba_lfnet_det_map_size(double scale_factor, int size);      /* one side of one map; -1 for a bad argument */
BTBA_API int btba_lfnet_det_map_sizes(const btba_lfnet_det_model *model, int H, int W, int32_t *map_h, int32_t *map_w);
BTBA_API int btba_lfnet_det_pad_size(const btba_lfnet_det_model *model);
BTBA_API int btba_lfnet_scores(btba_workspace *ws, const btba_lfnet_det_model *model, int n_frames, int H, int W, const float *photo_dev,
                               float *const *score_dev, float *ori_dev);

/* ---- pose accuracy: ADD and ADD-S (the YCBInEOAT evaluation) -------------------------------------------------------
 * The per-frame errors the reference's evaluation averages into its AUC figures (scripts/eval_ycbineoat.py:54-163 with
 * scripts/Utils.py:69-95, add / adi), for many evaluations in one call.  One evaluation is a model point set x_0 .. x_{N-1}
 * (object frame, metres), a predicted pose P and a ground-truth pose G, both row-major 4 x 4 OBJECT-IN-CAMERA (the
 * reference's poses/*.txt, Bundler.cpp:372-376; the tracker's own camera -> model poses are their inverses).
 *   q_i = G x_i (queries), c_j = P x_j (candidates), each row one fmaf chain:
 *       p_r = fmaf(T_r2, z, fmaf(T_r1, y, fmaf(T_r0, x, T_r3)))
 *   d2(a, b) = fmaf(dz, dz, fmaf(dy, dy, dx * dx)) with d = a - b (dx * dx a plain multiply; nothing else contracted)
 *   add_i  = sqrtf(d2(q_i, c_i))
 *   adds_i = sqrtf(min_j d2(q_i, c_j))                 (the reference's adi: a tree on the predicted points, queried with
 *                                                         the ground-truth points)
 *   sqrtf is the IEEE, correctly rounded square root.
 *   ADD = mean_i add_i, ADD-S = mean_i adds_i, each summed in fp64 in a fixed order: slot l of 256 sums (double) d_i for
 *   i = l (mod 256) in ascending i from +0; then s = 128, 64, .., 1: acc[l] += acc[l + s] for l < s; output
 *   (float)(acc[0] / N).
 * Consequences: adds_i <= add_i bit for bit (j = i is a candidate, same arithmetic), so ADD-S <= ADD; P == G gives 0 and 0.
 * An evaluation with a non-finite entry among its 32 pose entries gives a quiet NaN in both outputs; the others are
 * unaffected.  Model points must be finite (precondition, not checked).
 *
 *   model_pts_dev[m] : device float [n_pts[m]][3] (4-byte aligned), 1 <= n_pts[m] <= 2^22 (host int32 array)
 *   model_index      : host int32 [n_evals], each in 0 .. n_models - 1
 *   poses_pred, poses_gt : float [n_evals][16] row-major object-in-camera
 *   add_out, adds_out    : float [n_evals]
 * device_resident = 1: poses and outputs are device pointers; 0: host pointers.  n_evals == 0 is a no-op.  Synchronous on the
 * workspace stream; scratch (per-point minima, at most 64 MB: evaluations go in chunks) is grow-only in the workspace.
 * BTBA_EINVAL before any GPU work: ws, a table or an output NULL, a NULL model pointer, n_models < 1, n_evals < 0, a count
 * outside 1 .. 2^22, a model_index entry out of range. */
#define BTBA_EVAL_MAX_POINTS (1 << 22)
BTBA_API int btba_pose_errors(btba_workspace *ws, int device_resident,
                              int n_models, const float *const *model_pts_dev, const int32_t *n_pts,
                              int n_evals, const int32_t *model_index,
                              const float *poses_pred, const float *poses_gt,
                              float *add_out, float *adds_out);

/* ---- pose accuracy: 5 deg 5 cm, IoU25, rotation and translation error (the NOCS evaluation, 6-PACK protocol) -----------
 * The per-frame figures the reference's NOCS scorer turns into its per-class report (scripts/benchmark.py:65-159 called as at
 * :262-272), for many items in one call.  One item is a predicted pose, a ground-truth pose (both row-major 4 x 4 OBJECT-IN-
 * CAMERA, translation in the unit of shift_thresh: the protocol's is mm), a class and a box.  Class ids are the reference's
 * synset_names: 1 bottle, 2 bowl, 3 camera, 4 can, 5 laptop, 6 mug.  An item is ROTATION-SYMMETRIC when its class is 1, 2 or 4,
 * or 6 with handle_visible == 0.  (The reference's third branch names phone / eggbox / glue, classes this list does not have: it
 * is left out.)  All arithmetic is fp64; every product, sum and quotient below is rounded on its own (no fma), sums run left to
 * right as written.
 *   1. Pre-processing (:262-269).  flip_z180_pred: rows 0 and 1 of the predicted pose are negated, translation included.
 *      normalize_columns: each of the first three columns of each pose is divided by sqrt(m_0c^2 + m_1c^2 + m_2c^2 + m_3c^2).
 *      P and G below are the pre-processed prediction and ground truth.
 *   2. Errors (:120-159).  If the bottom row of P or of G is not exactly (0, 0, 0, 1): theta = shift = 10000, iou = NaN.
 *      Otherwise R = M[:3, :3] / cbrt(det M[:3, :3]) for each pose, det by cofactors along row 0:
 *          det = m00 (m11 m22 - m12 m21) - m01 (m10 m22 - m12 m20) + m02 (m10 m21 - m11 m20)
 *      rotation-symmetric: a = (y1 . y2) / (|y1| |y2|), y the second column of R, |y| = sqrt(y . y)
 *      otherwise:          a = (t0 + t1 + t2 - 1) / 2, t_r = the dot product of row r of R1 with row r of R2  (tr(R1 R2^T))
 *      theta = acos(a) * (180 / pi) degrees; shift = sqrt(dx^2 + dy^2 + dz^2), d = T_P - T_G.
 *   3. acos outside [-1, 1].  clamp_acos = 0: NaN, as numpy gives -- round-off puts a at 1 + 1 ulp for a good share of IDENTICAL
 *      pose pairs, whose theta is then NaN and who fail every theta < threshold test; the reference scores them so and the default
 *      keeps scores comparable.  clamp_acos = 1: a > 1 becomes 1 and a < -1 becomes -1 first (a NaN stays).
 *   4. IoU (:65-111; the call at :272 hands the GROUND TRUTH over as the pose that is rotated).  Under a pose M, corner k =
 *      (x, y, z) becomes p_r = (m_r0 x + m_r1 y + m_r2 z + m_r3) / (m_30 x + m_31 y + m_32 z + m_33), r = 0 .. 2.  The reference
 *      reduces its 3 x 8 corner array along axis 0 (:75-78), and so does this: lo_k = min(p_0, p_1, p_2) and hi_k = max(p_0, p_1,
 *      p_2) of corner k -- EIGHT values per pose, one per corner, not three per-axis extents.  It is the published protocol's
 *      figure, not a geometric box overlap.  e_k = min(hi1_k, hi2_k) - max(lo1_k, lo2_k); inter = 0 if any e_k < 0, else
 *      e_0 e_1 .. e_7; iou = inter / (v1 + v2 - inter), v = (hi_0 - lo_0)(hi_1 - lo_1) .. (hi_7 - lo_7), products from the left.
 *      rotation-symmetric: m = 0; for i = 0 .. n_sym_steps - 1: x = iou(G Ry_i, P), m = x if x > m; iou = m -- a NaN x is never
 *      taken.  Ry_i is the rotation about y by 2 pi i / n_sym_steps: columns 0 and 2 of G Ry_i are g_0 c + g_2 (-s) and
 *      g_0 s + g_2 c (all four rows), with (c, s) = (cos, sin) of ((2 pi) i) / n_sym_steps from the host's C library in double:
 *      one table per call, the same bits for every item.
 *      otherwise: iou = iou(G, P) as it comes (NaN when v1 + v2 - inter is 0 / 0).
 *   5. An item with a non-finite entry among its 32 pose entries (as given) has NaN in all three outputs; the others are
 *      unaffected.  Box corners must be finite (precondition, not checked).
 * rot_thresh_deg, shift_thresh and iou_thresh are not read by btba_nocs_errors: they travel with the parameters to the report
 * (btba::nocsReport, bundletrack_amd.nocs_eval.nocs_report), which counts theta < rot_thresh_deg && shift < shift_thresh and
 * iou > iou_thresh.
 *
 *   boxes            : host double [n_boxes][8][3], the eight corner rows of a model_scales/<model>.txt
 *   class_id         : host int32 [n_evals], each in 1 .. 6
 *   handle_visible   : host int32 [n_evals], or NULL (all 1, as the reference's scorer passes)
 *   box_index        : host int32 [n_evals], each in 0 .. n_boxes - 1
 *   poses_pred, poses_gt : double [n_evals][16] row-major
 *   theta_deg_out, shift_out, iou_out : double [n_evals]
 * device_resident = 1: poses and outputs are device pointers (8-byte aligned); 0: host pointers.  params NULL: the defaults.
 * n_evals == 0 is a no-op.  Synchronous on the workspace stream; items go in chunks of 2^18, staging is grow-only in the workspace.
 * BTBA_EINVAL before any GPU work: ws, boxes, a table or an output NULL, n_boxes < 1 or > 2^30, n_evals < 0, n_sym_steps outside
 * 1 .. 32, a class_id outside 1 .. 6, a box_index out of range, a misaligned device pointer. */
typedef struct btba_nocs_params {
    double rot_thresh_deg;           /* 5 */
    double shift_thresh;             /* 50, in the poses' unit (the protocol's mm: 5 cm) */
    double iou_thresh;               /* 0.25 */
    int32_t n_sym_steps;             /* 20 (1 .. 32) */
    int32_t flip_z180_pred;          /* 1 */
    int32_t normalize_columns;       /* 1 */
    int32_t clamp_acos;              /* 0 */
} btba_nocs_params;
BTBA_API void btba_nocs_params_default(btba_nocs_params *p);
BTBA_API int btba_nocs_errors(btba_workspace *ws, const btba_nocs_params *params, int device_resident,
                              int n_boxes, const double *boxes,
                              int n_evals, const int32_t *class_id, const int32_t *handle_visible, const int32_t *box_index,
                              const double *poses_pred, const double *poses_gt,
                              double *theta_deg_out, double *shift_out, double *iou_out);

/* ---- map points and the tracker's findCorres (the step between the matcher and BA) --------------------------------------
 * The memory behind SiftManager::findCorres (src/FeatureManager.cpp:173-240): map points (feature tracks) link the RANSAC inliers
 * of every processed pair (updateFramePairMapPoints, :448-487) and add PROPAGATED correspondences to non-neighbouring pairs
 * (findCorresByMapPoints, :489-521).  The rules below are integer bookkeeping; the GPU reproduces them exactly.
 * State.  Every live frame F has map_F: (u, v) -> map point, keyed by the keypoint's float (u, v) in std::map order (u, then v;
 * Frame::_map_points, Frame.h:71).  A map point has img: frame -> (u, v).  forgetFrame(F) (:142-170) erases img[F] from every
 * map point and touches no other frame's map.  Keys are (u, v) values, not indices: two keypoints of a frame with equal (u, v)
 * (fp32 ==, so -0 == +0) are ONE key, represented by the lowest such index (the canonical index); a non-finite keypoint is
 * BTBA_EINVAL at registration.
 * findCorres(A, B), A newer, the pair not processed before, neighbor = |idA - idB| == 1:
 *   1. NN: when both frames have keypoints, the btba_match_pairs records (A -> B, then B -> A, duplicates kept); neighbor and
 *      fewer than 5 matches marks A FAIL.  With 0 keypoints on either side nothing is appended and nothing is marked.
 *   2. A FAIL (now, or set by an earlier pair): the pair keeps its matches as they are; stop.
 *   3. Propagation (non-neighbours): walk map_A in key order, skip map points without img[B]; candidate (uvA, uvB = img[B]) with
 *      the camera-space points at roundf of each keypoint (the matcher's xyz convention, no gate); drop it if a match already in
 *      the list (candidates appended earlier in this walk included) has the same A key or the same B key; else append it.
 *   4. RANSAC (:561-657, 659-741; the propogated_samples / rand() code there is dead): <= 5 matches are cleared; otherwise
 *      btba_ransac_pairs_ex on the model-frame points of all matches (this pair alone, n_pairs = 1) and the list becomes its
 *      inliers in ascending order, cleared when fewer than 5 (:728-731).
 *   5. (A FAIL: stop -- cannot happen after step 2.)
 *   6. Update, match by match in order: both keys mapped (uvA in map_A, uvB in map_B): skip.  uvB not in map_B: a new map point
 *      with img = {B: uvB}, map_B[uvB] = it; else mp = map_B[uvB].  Then mp.img[A] = uvA and map_A[uvA] = mp (overwriting; for a
 *      map point shared by several matches the last one wins).  Later matches see earlier matches' effects.
 *   7. Fewer than 5 matches: cleared, and A marked FAIL when neighbor.
 *
 * btba_mappoints lives on one workspace's device and stream.  A frame occupies a SLOT from registration to forget:
 *   per slot: its keypoints (copied), canonical indices, walk order, and map_F as one int32 map-point id per keypoint;
 *   per map point: one row of canonical keypoint indices, one per slot (-1 = none); ids of map points whose row becomes empty
 *   on forget are recycled (such a point is unreachable: map_F[uv] = mp implies img[F] is present until F is forgotten).
 * Slot count and map-point capacity are grow-only; capacity is reserved at registration for every map point the live slots can
 * still create, so a chain never allocates.  Beyond the hard limits (1024 slots, 2^28 img entries) registration returns
 * BTBA_ENOMEM and changes nothing.  A chain checks before its first launch that the capacity covers the bound (BTBA_ENOMEM, nothing
 * changed, otherwise); the device allocator also guards every id it hands out.  That guard cannot fire while the bound holds; should it
 * ever fire, the chain returns BTBA_ENOMEM with the memory partly updated and marks it unusable: every later register / forget / chain
 * on it returns BTBA_ENOMEM (destroy and create a new one).  register / forget / export synchronise the workspace stream; _destroy does
 * not touch the workspace (it may be destroyed before or after it).
 *   _register_frame : n_kpts 0 .. 8192 device float2 keypoints (8-byte aligned) -> *slot_out (the lowest free slot)
 *   _forget_frame   : forgetFrame; the slot is free for the next registration
 *   _export         : host copy for tests.  dims_out[4] = {slots S, map-point ids M (high-water mark), sum of live slots' n, overflow
 *                     flag}; any other pointer may be NULL (call once with them NULL to size them): slot_n_out[S] (n, or -1 for a free
 *                     slot), canon_out / map_out (the live slots' arrays back to back in slot order), img_out [M][S] (-1 = none; rows of
 *                     recycled ids are all -1).
 *
 * btba_corres_chain runs findCorres for an ORDERED list of pairs: btba_match_pairs' frame arguments (each frame's keypoints must
 * be the ones its slot was registered with), slots[n_frames] (the frames of one pair list must occupy distinct slots), status
 * [n_frames] host in / out (nonzero = FAIL; the chain writes 1), btba_corres_params (defaults = btba::Config: 2000 trials, 0.01 m,
 * BTBA_RANSAC_REFERENCE_SVD, seed 0).  pairs: [n_pairs][2] frame indices, A first with frame_ids[A] > frame_ids[B], no frame pair
 * twice.  NN runs once for all pairs (five launches); then per pair in order four single-workgroup-or-small launches: propagation,
 * RANSAC vote, RANSAC inlier list, update + gates.  Nothing in between synchronises the host, allocates or copies to the host; the
 * call synchronises once at the end (the host output form copies the records after that).
 *   matches_out      : btba_match records of all pairs back to back, pair p at sum_{q<p} n_out[q]; capacity from
 *                      btba_corres_chain_capacity (sum over pairs of nA + nB (mutual) + nA).  NN records as btba_match_pairs writes
 *                      them; propagated records have dir = 2, dist = -1 and CANONICAL keypoint indices.
 *   n_out            : host int32 [n_pairs]
 *   stage_counts_out : NULL or host int32 [n_pairs][4]: after NN, after propagation, after RANSAC, final (a stage that did not run
 *                      repeats the count before it).
 * device_resident = 1: matches_out is a device pointer; 0: a host pointer. */
typedef struct btba_mappoints btba_mappoints;
typedef struct btba_corres_params {
    int32_t n_trials;                       /* RANSAC trials (ransac.max_iter, 2000) */
    float dist_thres;                       /* inlier distance (ransac.inlier_dist, 0.01 m) */
    int32_t hypothesis;                     /* BTBA_RANSAC_REFERENCE_SVD or BTBA_RANSAC_HORN, optionally | BTBA_RANSAC_DRAW_HASH */
    int32_t pad;
    uint64_t seed;                          /* 0 */
} btba_corres_params;
BTBA_API int btba_mappoints_create(btba_workspace *ws, btba_mappoints **out);
BTBA_API void btba_mappoints_destroy(btba_mappoints *mp);
BTBA_API int btba_mappoints_register_frame(btba_mappoints *mp, int n_kpts, const float *kpts_dev, int32_t *slot_out);
BTBA_API int btba_mappoints_forget_frame(btba_mappoints *mp, int32_t slot);
BTBA_API int btba_mappoints_export(btba_mappoints *mp, int32_t *dims_out, int32_t *slot_n_out, int32_t *canon_out, int32_t *map_out, int32_t *img_out);
BTBA_API void btba_corres_params_default(btba_corres_params *p);
/* btba_match_capacity's validation plus: no frame pair twice.  Host-only: no GPU, no workspace, no map-point memory. */
BTBA_API int btba_corres_chain_capacity(const btba_match_params *params, int n_frames, int H, int W, int D, const int32_t *n_kpts,
                                        int n_pairs, const int32_t *pairs, int64_t *capacity_out);
BTBA_API int btba_corres_chain(btba_workspace *ws, btba_mappoints *mp, const btba_match_params *params, const btba_corres_params *ransac,
                               int device_resident, int n_frames, int H, int W, const float *K_rowmajor, const float *const *desc_dev, int D,
                               const float *const *kpts_dev, const int32_t *n_kpts, const float *const *depth_dev, const float *const *normal_dev,
                               const float *poses, const int32_t *frame_ids, const int32_t *slots, int32_t *status, int n_pairs,
                               const int32_t *pairs, btba_match *matches_out, int32_t *n_out, int32_t *stage_counts_out);

/* ---- window assembly (the step between findCorres and the solver) ------------------------------------------------------
 * The two host steps between btba_corres_chain and btba_solve_batch_zn(_aux), on the chain's device-resident btba_match records:
 * Bundler::optimizeGPU's marshalling (src/Bundler.cpp:286-347) and SiftManager::procrustesByCorrespondence
 * (src/FeatureManager.cpp:523-557 with Utils::solveRigidTransformBetweenPoints, src/Utils.cpp:180-214).
 *
 * Marshalling.  A window is n_frames frames sorted by id (index 0 the oldest); its P = n_frames (n_frames - 1) / 2 canonical pairs
 * (i, j), i < j, come in the order (0,1) (0,2) .. (N-2,N-1).  Pair (i, j) owns a SEGMENT (first record, count) of one btba_match
 * array: the records of findCorres(A = frame j, B = frame i), count 0 for a pair without matches.  Record k of the segment becomes
 *   EntryJ{imgIdx_i = i, imgIdx_j = j, pos_i = ptB_cam, pos_j = ptA_cam}                                (Bundler.cpp:311-316)
 * at entry pair_offsets[p] + k of the window: pair-major, records in their order.  pair_offsets[0] = 0, pair_offsets[p + 1] =
 * pair_offsets[p] + count[p].  n_edges_newframe = the sum of the counts of the pairs that contain the new frame's index; BA runs
 * iff n_edges_newframe > min_fm_edges_newframe (Bundler.cpp:343-347; otherwise the caller marks the frame NO_BA).  Windows of one
 * call share n_frames and corr_stride = the largest window total, as in btba_solve_batch.
 *
 * btba_window_layout: host-only (no GPU, no workspace).
 *   seg_counts      : host int32 [n_windows][P]
 *   newframe_index  : host int32 [n_windows], each in 0 .. n_frames - 1
 *   corr_stride_out : the largest window total (0 when no window has a match: allocate at least one entry, btba_solve_batch_zn
 *                     wants corr_stride >= 1);  max_corr_per_pair_out : the largest count
 *   pair_offsets_out: host uint32 [n_windows][P + 1];  n_edges_newframe_out : host int64 [n_windows];  run_ba_out : host int32
 *                     [n_windows], 1 = the gate passed.  Any output may be NULL.
 *   BTBA_EINVAL: n_windows < 1, n_frames outside 2 .. BTBA_MAX_FRAMES, a NULL table, a negative count, a new-frame index out of
 *   range, a window total beyond uint32.  Nothing is written then.
 *
 * btba_marshal_windows: one launch for all windows, asynchronous on the workspace stream, no atomics, no host synchronisation.
 * Every data pointer is a DEVICE pointer.
 *   matches_dev      : btba_match [n_records] (16-byte aligned; the chain's matches_out with device_resident = 1)
 *   segments_dev     : uint32 [n_windows][P][2] = (first record, count) -- the table btba_window_layout was given, with the records'
 *                      places.  A segment that leaves [0, n_records) is not read and its entries are not written (its count still
 *                      enters the offsets).
 *   max_corr_per_pair, corr_stride : as btba_window_layout returns them (corr_stride may be larger, >= 1)
 *   corr_dev         : btba_entryj [n_windows][corr_stride] (16-byte aligned).  Entries at or beyond pair_offsets[P] of a window
 *                      are NOT written (as are entries at or beyond corr_stride, should the table not match the layout).
 *   pair_offsets_dev : uint32 [n_windows][P + 1]
 *   corr24_dev       : NULL, or the array of btba_pack_correspondences24 for this corr_dev / corr_stride, written in the same pass:
 *                      bit for bit what that call makes of corr_dev.
 *   BTBA_EINVAL: NULL ws / matches_dev (with n_records > 0) / segments_dev / corr_dev / pair_offsets_dev, n_windows < 1, n_frames
 *   outside 2 .. BTBA_MAX_FRAMES, n_records < 0 or beyond uint32, corr_stride < 1, a misaligned array.
 *
 * btba_procrustes_pairs: the Kabsch fit of many pairs in two launches.  Pair e is a segment (first record, count n) of
 * matches_dev and two row-major camera -> model poses TA, TB (frame A = the newer one, as in the records).
 * ARITHMETIC CONTRACT:
 *   a_k = TA ptA_cam, b_k = TB ptB_cam in the matcher's uncontracted fp32: P_r = ((T_r0 x + T_r1 y) + T_r2 z) + T_r3.
 *   n < 5 (countInlierCorres < 5, FeatureManager.cpp:527): pose = identity, err = 0, moments = (n, 0, .., 0).
 *   All sums are fp64 in the fixed order of btba_pose_errors: slot l of 256 sums the terms of k = l (mod 256) in ascending k from
 *   +0; then s = 128, 64, .., 1: acc[l] += acc[l + s] for l < s.  Products are plain fp64 multiplies, nothing is contracted.
 *   m1 = (sum (double) a_k) / n, m2 = (sum (double) b_k) / n;  S_rc = sum ((double) a_k,r - m1_r) * ((double) b_k,c - m2_c): the
 *   reference's P^T Q.  This part is reproducible bit for bit on a CPU (tests/window_ref.py); moments_out = n, m1, m2, S row-major.
 *   R = the proper rotation that maximises tr(R S) -- the reference's V U^T with V's last column flipped when det < 0 -- by Horn's
 *   quaternion method: the eigenvector of the largest eigenvalue of the symmetric 4 x 4 N(S), by cyclic Jacobi in fp64
 *   (bundletrack_amd/csrc/btba_window.hpp writes the algorithm out).  No reflection case exists.  A rank-deficient S gives a finite
 *   proper rotation: one of the maximisers when they are not unique (collinear points), the identity for S = 0.
 *   t_r = m2_r - ((R_r0 m1_0 + R_r1 m1_1) + R_r2 m1_2) in fp64.  R and t are rounded ONCE to fp32 into a row-major 4 x 4 (last row
 *   0 0 0 1).
 *   err = (float) (sqrt(sum_k |d_k|^2) / n), d_k,r = (((R_r0 a_0 + R_r1 a_1) + R_r2 a_2) + t_r) - b_r with the fp64 R, t and the
 *   points converted to fp64, |d|^2 = (d_0^2 + d_1^2) + d_2^2, summed over k in the fixed order: ||R a + t - b||_F / n, the quantity
 *   of FeatureManager.cpp:550.  The library never aborts on it; a caller applies the reference's err > 1e-3 gate if it wants to.
 *   A non-finite moment or a non-finite rounded result gives identity and err = 0 (the reference's isMatrixFinite / isApprox
 *   fallbacks).  A pair never affects another pair.
 *
 *   matches_dev      : device btba_match [n_records] (8-byte aligned)
 *   segments         : HOST int32 [n_pairs][2] = (first record, count)
 *   posesA, posesB   : float [n_pairs][16];  pose_out : float [n_pairs][16];  err_out : float [n_pairs]
 *   moments_out      : NULL, or double [n_pairs][16]
 * device_resident = 1: poses and the three outputs are device pointers; 0: host pointers.  n_pairs == 0 is a no-op.  Synchronous
 * on the workspace stream; scratch (the table, the moments, host-form staging) is grow-only in the workspace.
 * BTBA_EINVAL before any GPU work: NULL ws, n_pairs < 0, n_records < 0 or beyond uint32; with n_pairs > 0 a NULL table, pose array,
 * pose_out or err_out, matches_dev NULL with n_records > 0, a misaligned matches_dev, a negative first record or count, a segment
 * that leaves [0, n_records). */
BTBA_API int btba_window_layout(int n_windows, int n_frames, const int32_t *seg_counts, const int32_t *newframe_index,
                                int32_t min_fm_edges_newframe, int64_t *corr_stride_out, uint32_t *max_corr_per_pair_out,
                                uint32_t *pair_offsets_out, int64_t *n_edges_newframe_out, int32_t *run_ba_out);
BTBA_API int btba_marshal_windows(btba_workspace *ws, int n_windows, int n_frames, const btba_match *matches_dev, int64_t n_records,
                                  const uint32_t *segments_dev, uint32_t max_corr_per_pair, int64_t corr_stride,
                                  btba_entryj *corr_dev, uint32_t *pair_offsets_dev, float *corr24_dev);
BTBA_API int btba_procrustes_pairs(btba_workspace *ws, int device_resident, int n_pairs, const btba_match *matches_dev, int64_t n_records,
                                   const int32_t *segments, const float *posesA, const float *posesB,
                                   float *pose_out, float *err_out, double *moments_out);

/* ---- pose covariances: how well a window constrains the poses a solve returns ----------------------------
 * Two calls, usually made after btba_solve_batch_zn(_aux) on the poses it returned.
 *
 * btba_linearize_batch_zn_aux -- the solver's system at the caller's poses.  The arguments of btba_solve_batch_zn_aux, except that
 * poses_dev is const and never written, there is no trace, and there are two outputs:
 *   info_dev : float [n_instances][na][na], na = 6 (n_frames - 1) -- the Gauss-Newton matrix J^T W J the solve's first iterate would
 *              assemble at these poses, frame 0 (fixed) without rows and columns
 *   rhs_dev  : NULL, or float [n_instances][n_frames - 1][6] -- its right-hand side -J^T W r; the norm is the first-order optimality measure
 * The unknowns are in the public order of btba_matrices_to_poses: per frame (rot, trans), rows 0-2 in radians, rows 3-5 in metres.  They
 * describe the LEFT perturbation the solver applies, x_k <- Log(Exp(delta_k) Exp(x_k)).  Both outputs are, bit for bit, what a traced solve
 * (BTBA_FLAG_TRACE) with n_gn_iters = 1 from the same poses and parameters records: info is the record's A without frame 0's rows and columns
 * and with each frame's halves swapped from the record's [trans, rot] order, rhs the record's rhs of frames 1 .. n_frames - 1.
 * WHAT THE MATRIX IS: the sparse (correspondence) share carries weight_sparse and NO Huber weight on the left-hand side (as in the reference's
 * solver, the robust weight enters its right-hand side only); the dense share is Huber-weighted and carries weight_dense_depth; a dense pair listed
 * only in the reversed direction (target > source) contributes to both frames' diagonal blocks and carries no cross block.  Its inverse is
 * therefore the inverse of the solver's Gauss-Newton matrix, NOT a calibrated covariance: a caller scales it by a residual variance of its own.
 * The scalar weight_sparse / weight_dense_depth are used; n_gn_iters, n_pcg_iters and BTBA_FLAG_TRACE are ignored; every window the solve serves
 * (2 .. BTBA_MAX_FRAMES frames) is served, through whichever solve kernel the dispatch picks for it.  Asynchronous on the workspace stream; scratch
 * (a copy of the poses, one trace record per instance) is grow-only in the workspace; a later solve on the workspace returns the bits it
 * returns without this call, and btba_collect_stats keeps reporting the last solve.
 * BTBA_EINVAL before any GPU work: NULL ws, params, poses_dev or info_dev, n_instances < 1, n_frames outside 2 .. BTBA_MAX_FRAMES, a per-iteration
 * weight array set (weights_sparse_per_iter / weights_dense_per_iter); otherwise what btba_solve_batch_zn_aux returns for a traced solve
 * (BTBA_REDUCE_ATOMIC is BTBA_EINVAL: the trace is defined on the reproducible sums).
 *
 * btba_pose_covariances -- the batched fp64 inverse of that matrix (or of any symmetric positive definite fp32 matrix in the same layout).
 *   info_dev        : float, instance b at info_dev + b * info_stride, [na][na] row-major; the LOWER triangle is read
 *   info_stride     : floats per instance, >= na * na
 *   cov_blocks_dev  : double [n_instances][n_frames][6][6] -- each frame's marginal 6 x 6 block of the inverse, (rot, trans); frame 0: zeros
 *   cov_full_dev    : NULL, or double [n_instances][na][na] -- the whole inverse
 *   pivot_ratio_dev : NULL, or double [n_instances] -- min_j d_j / H_jj over the Cholesky pivots d_j: 1 for a diagonal matrix, towards 0 as
 *                     some unknown becomes determined by the others; the cheap conditioning figure a tracker can threshold
 *   status_dev      : int32 [n_instances] -- 0: the factorisation completed; 1 + j: unknown j (public order) is the first whose pivot d_j is
 *                     not > 0 or not finite.  All covariance outputs of that instance are then quiet NaNs and its pivot_ratio is 0; the
 *                     other instances are not affected.  A frame that nothing constrains has a zero block and an exactly zero pivot.
 * One workgroup per instance: the matrix is widened to fp64 into LDS as a packed lower triangle, factorised H = L L^T over the unknowns in
 * their public order, L inverted in place, Sigma = L^-T L^-1 -- IEEE fp64 throughout (fused multiply-add, correctly rounded division and square
 * root), no atomics, every sum in an order fixed by the window size alone: an instance yields the same bits at any batch position and in
 * any batch size, cov_full is symmetric bit for bit and cov_blocks are its diagonal blocks bit for bit.
 * Windows of 2 .. BTBA_MAX_FRAMES_LDS (31) frames are served: at 31 frames the packed triangle takes 130 320 of a compute unit's 163 840
 * bytes of LDS; a larger window is BTBA_EINVAL.  Asynchronous on the workspace stream; all pointers are device pointers.
 * BTBA_EINVAL before any GPU work: NULL ws, info_dev, cov_blocks_dev or status_dev, n_instances < 1, n_frames outside
 * 2 .. BTBA_MAX_FRAMES_LDS, info_stride < na * na, a misaligned pointer. */
BTBA_API int btba_linearize_batch_zn_aux(btba_workspace *ws, const btba_params *params, int n_instances, int n_frames,
                                         int H, int W, const float *K_rowmajor, const float *zn_dev, const btba_zn_aux *aux,
                                         const btba_entryj *corr_dev, int64_t corr_stride,
                                         const uint32_t *pair_offsets_dev, uint32_t max_corr_per_pair,
                                         const int32_t *dense_pairs, int n_dense_pairs, const float *poses_dev,
                                         float *info_dev, float *rhs_dev);
BTBA_API int btba_pose_covariances(btba_workspace *ws, int n_instances, int n_frames,
                                   const float *info_dev, int64_t info_stride /* floats per instance, >= na*na */,
                                   double *cov_blocks_dev  /* [n_instances][n_frames][6][6]; frame 0: zeros */,
                                   double *cov_full_dev    /* NULL or [n_instances][na][na] */,
                                   double *pivot_ratio_dev /* NULL or [n_instances] */,
                                   int32_t *status_dev     /* [n_instances] */);

/* ---- objective report: the cost the solver descends, at given poses ------------------------------------------
 * btba_objective_batch_zn_aux takes the arguments of btba_linearize_batch_zn_aux and returns, per instance, the value of
 *     objective = weight_sparse * sum rho(||T_i pos_i - T_j pos_j||^2) + weight_dense_depth * sum rho(res^2)
 * with rho the Huber loss (e inside the knee e <= robust_delta^2, 2 delta sqrt(e) - delta^2 beyond it) -- the function whose gradient along the
 * solver's left perturbation is -2 x the right-hand side btba_linearize_batch_zn_aux returns --, and per correspondence segment and per dense
 * pair how many terms there are, how many lie beyond the knee, and which one is worst.
 * Evaluation is at the matrices a solve forms of these poses (Exp(Log(P)) and its inverse, in scratch; poses_dev is never written).  Each
 * residual is computed in fp32 by the sweeps' own expressions: sparse r = T_i pos_i - T_j pos_j over the valid entries of a segment (EntryJ, or the
 * 24-byte records of aux->corr24); dense res = (c_i - q) . n_i over the source pixels that pass the solver's gates (depth range, in-image
 * projection, the clamped 2 x 2 tap blend, normal and distance thresholds), zero-skew and general K.  Everything behind the residual -- square,
 * rho, weight, sums -- is IEEE fp64, no atomics, every sum in an order fixed by the cache size, the segment lengths and the window size: an
 * instance gives the same bytes at any batch position and in any batch size.
 * The dense pairs are those the solve derives from dense_pairs / n_dense_pairs (NULL: every i < j as (target i, source j)); record q belongs to
 * listed pair q.  weight_dense_depth <= 0: no dense term is evaluated, as the solve builds no dense system then -- every dense record is zero with
 * worst = -1; weight_sparse <= 0, no correspondences or max_corr_per_pair == 0: the same for the sparse records.
 * BTBA_FLAG_COMPACTION is IGNORED: every pixel of the source frame is walked (aux's lists and block ranges are not read), which gives what a walk
 * of the lists would give, a listed pixel being one with a depth.  n_gn_iters, n_pcg_iters, pair_policy, reduction_mode and the other flags are
 * ignored as well.
 * Asynchronous on the workspace stream; scratch (the matrices, one partial record per (pair, 1 024 pixels) and per (segment, 1 024 entries)) is
 * grow-only in the workspace; btba_collect_stats keeps reporting the last solve, and a later solve returns the bits it returns without this call.
 * BTBA_EINVAL before any GPU work: NULL ws, params, poses_dev or total_dev, n_instances < 1, n_frames outside 2 .. BTBA_MAX_FRAMES, a
 * per-iteration weight array set, an output not aligned to 8 bytes; also what the solve refuses (NULL K or zn_dev, a cache below 2 x 2, an invalid or
 * repeated dense pair).
 * Not served: the float4 cache of btba_solve_batch and the btba_optimize_frames(_keyed) boundary.  The solve itself makes no use of the report. */
typedef struct btba_objective_pair {      /* 40 bytes; one per (instance, pair) */
    double  sum_sq;     /* sparse: sum ||r||^2.   dense: sum w res^2, w = min(1, delta / |res|) */
    double  sum_rho;    /* sum rho(e), e = ||r||^2 or res^2 */
    double  max_abs;    /* sparse: max over entries of max(|r.x|, |r.y|, |r.z|); dense: max |res|; 0 when count == 0 */
    int32_t count;      /* valid entries of the segment / accepted pixels of the pair */
    int32_t n_outlier;  /* of those, e > delta^2 */
    int32_t worst;      /* entry index within the segment / source pixel index y * Wd + x that attains max_abs, the lowest on ties; -1 when count == 0 */
    int32_t reserved;   /* 0 */
} btba_objective_pair;
typedef struct btba_objective_total {     /* 64 bytes; one per instance */
    double  objective;  /* weight_sparse * sparse_rho + weight_dense_depth * dense_rho */
    double  sparse_rho, dense_rho, sparse_sq, dense_wsq;   /* sums of the pair records in index order, unweighted */
    int64_t n_sparse, n_dense;                             /* sums of the counts */
    int64_t n_residuals;                                   /* 3 * n_sparse + n_dense */
} btba_objective_total;
BTBA_API int btba_objective_batch_zn_aux(btba_workspace *ws, const btba_params *params, int n_instances, int n_frames,
                                         int H, int W, const float *K_rowmajor, const float *zn_dev, const btba_zn_aux *aux,
                                         const btba_entryj *corr_dev, int64_t corr_stride,
                                         const uint32_t *pair_offsets_dev, uint32_t max_corr_per_pair,
                                         const int32_t *dense_pairs, int n_dense_pairs, const float *poses_dev,
                                         btba_objective_total *total_dev  /* [n_instances] */,
                                         btba_objective_pair *sparse_dev  /* NULL or [n_instances][n_frames (n_frames - 1) / 2] */,
                                         btba_objective_pair *dense_dev   /* NULL or [n_instances][Pd], Pd = n_dense_pairs, or n_frames (n_frames - 1) / 2 without a list */);

/* ---- keyframe fusion and voxel-grid downsampling: tracked frames to an object cloud --------------------------------
 * btba_fuse_frames turns the posed keyframes a session ends with (Bundler's keyframes: depth, normal and colour maps already
 * invalidated outside the mask by btba_apply_masks, and a bundle-adjusted pose_in_model) into ONE voxel-grid cloud per object, and
 * is at the same time Utils::downsamplePointCloud (src/Utils.cpp:134-140: pcl::VoxelGrid; used for the model cloud at
 * src/DataLoader.cpp:92 with leaf 0.015 and for drawProjectPoints at src/Utils.cpp:218 with leaf 0.01).  The voxel rule below is
 * pcl::VoxelGrid::applyFilter's, RESTATED FROM PCL'S PUBLISHED HEADER AND UNVERIFIED AGAINST A PCL RUN (PCL is not available to this
 * project).  Every rule is exact, so a CPU restatement (tests/fusion_ref.py) reproduces every output byte.
 *
 * A call serves n_instances independent objects.  Each owns the segments that name it (in any order) and one voxel box.
 *   Frame segment (BTBA_FUSE_FRAME): geom = device float depth [H*W], normal = device float4 [H*W], colour = device uchar4 [H*W]
 *     ((B, G, R, 0), Frame::updateColorGPU), pose = row-major 4 x 4 camera -> model (FrameRef.pose_in_model; row 3 is not read).  The
 *     camera-space point of pixel (x, y) is btba_depth_to_normals' / btba_ingest_frames' xyz_out bit for bit (the same device
 *     function, the same Kinv of K_rowmajor).  A pixel is dropped when its depth fails (double)d >= 0.1 and, with
 *     params.require_normals, when its normal is exactly (0, 0, 0).  normal may be NULL only with require_normals = 0.
 *   Point-list segment (BTBA_FUSE_POINTS): geom = device float4 xyz [n] (w is not read), normal = NULL or device float4 [n], colour =
 *     NULL or device uchar4 [n].  A point with a non-finite coordinate is dropped (VoxelGrid's is_dense = false rule);
 *     require_normals does not apply.  With the identity pose this is the plain downsamplePointCloud.
 * Per surviving point, uncontracted fp32 in the order written:
 *   1. p_r = ((T_r0 x + T_r1 y) + T_r2 z) + T_r3 and n_r = (T_r0 nx + T_r1 ny) + T_r2 nz.  A segment without a normal map gives n = 0; a
 *      rotated normal with a component that is not below 2^16 in magnitude (or NaN) counts as (0, 0, 0).
 *   2. voxel i_a = (int)floorf(p_a * inv_leaf) - min_b_a, inv_leaf = 1.0f / leaf formed once on the host in fp32.  The point is counted in
 *      n_outside[instance] and dropped when some |p_a| is not below 2^16 m (NaN included) or some i_a lies outside 0 <= i_a < dims_a.
 *   3. the voxel's count (uint32) grows by 1, its three position sums (int64) by llrint((double)p_a * 2^20) and its normal sums by
 *      llrint((double)n_a * 2^20) (both exact up to the one rounding to nearest even), its three colour sums (uint32) by the
 *      bytes x, y, z of the uchar4.  Integer atomicAdd on device memory; no float atomics.
 * Output, per instance: the voxels with count >= min_points (VoxelGrid's setMinimumPointsNumberPerVoxel) in ascending linear index
 * lin = ix + dims_x (iy + dims_y iz), VoxelGrid's order after its sort.  Record k of instance b sits at [b * capacity + k]:
 *   xyz_out     float4: (float)((double)sum_a / 2^20 / count) per axis, w = 1
 *   normal_out  float4: the mean normal formed the same way, w = 0; NOT renormalised (VoxelGrid averages every field) unless
 *               params.normalize_normals: then n / sqrtf((nx nx + ny ny) + nz nz), (0, 0, 0) where that length is 0
 *   colour_out  uchar4: (2 sum + count) / (2 count) per channel in integers, w = 0
 *   count_out   uint32, lin_out int32
 *   n_out[b]    the number of qualifying voxels EVEN WHEN IT EXCEEDS capacity; nothing is written at or past [b * capacity + capacity],
 *               and status[b] then has BTBA_FUSE_OVERFLOW set (0 otherwise).  An instance without a surviving point gives n_out = 0.
 * Because every sum is an integer, the result has the same bytes in any execution order, at any batch position, in any segment
 * order and from run to run.  The sums are exact while a voxel receives fewer than 2^27 points (position), 2^24 (colour).
 *
 * The box (min_b[3], dims[3]) per instance is a HOST argument, so the fusion call needs no host synchronisation.  btba_fuse_bounds
 * makes VoxelGrid's data-derived box on the device: over the same segments, min_b_a = min floorf(p_a * inv_leaf) and dims_a = max - min
 * + 1 over the surviving points with every |p_a| below 2^16 (integer atomicMin / atomicMax), six int32 per instance; an instance
 * without such a point gets six zeros.  The caller copies them to the host (its one synchronisation) and passes them on.
 * btba_fuse_layout is host-only (no GPU, no workspace), in the family of btba_match_capacity and btba_window_layout: it validates
 * the boxes (BTBA_EINVAL: a negative side, more than BTBA_FUSE_MAX_VOXELS voxels in the whole call) and returns every instance's first
 * voxel, voxel_offsets_out [n_instances + 1] (NULL: not wanted), and the scratch the call will take, 64 bytes per voxel in
 * structure-of-arrays planes plus the compaction's block counts.  The scratch itself is grow-only in the workspace, as
 * btba_match_pairs' is: the caller passes none.
 *
 * btba_fuse_bounds and btba_fuse_frames are asynchronous on the workspace stream; segments go in chunks of BTBA_FUSE_CHUNK whose
 * pointers, poses and boxes travel as kernel arguments, so no host memory is read after the call returns.  Planes that no output
 * reads (normal sums without normal_out, colour sums without colour_out) are neither cleared nor accumulated.
 * BTBA_EINVAL, decided before the first launch: NULL ws, params, segments (with n_segments > 0), box or a required output (xyz_out,
 * n_out, n_outside, status; box_out_dev); n_instances < 1, n_segments < 0, capacity < 0, n_instances * capacity beyond 2^31 - 1; leaf
 * not > 0, not finite or below 2^-14 m (inv_leaf would let the floor leave int32); min_points < 1; a segment with an unknown kind, an
 * instance outside 0 .. n_instances - 1, a NULL geom (but for a point list with n = 0), n outside 0 .. 2^30 (point list); a frame segment with H < 1, W < 1, H * W >
 * 2^30 or K_rowmajor NULL, or without a normal map under require_normals; geom of a point list, a normal map or a float4 output
 * not 16-byte aligned, a depth, colour map, uchar4, count or lin output not 4-byte aligned; colour_out with a segment that has no colour
 * map; a negative box side, |min_b_a| above 2^30, or more than BTBA_FUSE_MAX_VOXELS voxels.
 * btba_voxel_downsample is btba_fuse_frames on one point-list segment per instance with the identity pose. */
#define BTBA_FUSE_MAX_VOXELS (1 << 24)    /* voxels of one call, all instances together: 1 GiB of scratch */
#define BTBA_FUSE_CHUNK 32                /* segments per launch */
#define BTBA_FUSE_FRAME 0
#define BTBA_FUSE_POINTS 1
#define BTBA_FUSE_OVERFLOW 1              /* status bit: n_out exceeds capacity */
typedef struct btba_fuse_params {
    float leaf;                           /* voxel side in metres (default 0.005) */
    int32_t min_points;                   /* 1 (default): points a voxel needs to be output */
    int32_t require_normals;              /* 1 (default): frame pixels with a zero normal are dropped */
    int32_t normalize_normals;            /* 0 (default): the mean normal as it is */
} btba_fuse_params;
typedef struct btba_fuse_segment {        /* 104 bytes, host memory */
    int32_t kind;                         /* BTBA_FUSE_FRAME or BTBA_FUSE_POINTS */
    int32_t instance;
    int64_t n;                            /* points of a point list; not read for a frame (H * W) */
    const void *geom;                     /* device: float depth [H*W], or float4 xyz [n] */
    const void *normal;                   /* device float4, or NULL */
    const void *colour;                   /* device uchar4, or NULL */
    float pose[16];                       /* row-major camera -> model */
} btba_fuse_segment;
BTBA_API void btba_fuse_params_default(btba_fuse_params *p);
BTBA_API int btba_fuse_layout(int n_instances, const int32_t *box /* host [n_instances][6] */, int64_t *voxel_offsets_out, int64_t *scratch_bytes_out);
BTBA_API int btba_fuse_bounds(btba_workspace *ws, const btba_fuse_params *params, int n_instances, int n_segments,
                              const btba_fuse_segment *segments, int H, int W, const float *K_rowmajor,
                              int32_t *box_out_dev /* [n_instances][6] */);
BTBA_API int btba_fuse_frames(btba_workspace *ws, const btba_fuse_params *params, int n_instances, int n_segments,
                              const btba_fuse_segment *segments, int H, int W, const float *K_rowmajor,
                              const int32_t *box /* host [n_instances][6] */, int capacity,
                              float *xyz_out_dev      /* float4 [n_instances][capacity] */,
                              float *normal_out_dev   /* NULL or float4 [n_instances][capacity] */,
                              uint8_t *colour_out_dev /* NULL or uchar4 [n_instances][capacity] */,
                              uint32_t *count_out_dev /* NULL or [n_instances][capacity] */,
                              int32_t *lin_out_dev    /* NULL or [n_instances][capacity] */,
                              int32_t *n_out_dev, int32_t *n_outside_dev, int32_t *status_dev /* [n_instances] each */);
BTBA_API int btba_voxel_downsample(btba_workspace *ws, const btba_fuse_params *params, int n_instances,
                                   const float *const *xyz_dev, const float *const *normal_dev /* NULL, or entries NULL */,
                                   const uint8_t *const *colour_dev /* NULL, or entries NULL */, const int64_t *n_points,
                                   const int32_t *box, int capacity, float *xyz_out_dev, float *normal_out_dev, uint8_t *colour_out_dev,
                                   uint32_t *count_out_dev, int32_t *lin_out_dev, int32_t *n_out_dev, int32_t *n_outside_dev, int32_t *status_dev);

/* ---- frame-to-model registration: point-to-plane ICP of frames against the fused cloud ---------------------------------
 * btba_register_frames refines the camera -> model pose of many (frame or point list, model) items in one call: batched point-to-plane
 * Gauss-Newton ICP against the voxel cloud btba_fuse_frames / btba_voxel_downsample made, used in place.  It is what brings a frame the
 * tracker marked FAIL back against what the session has learned of the object; with n_iters = 0 it is the numeric half of a pose check
 * (the points of a frame that lie on the model at a pose, and their point-to-plane error); its cost per matched point is the per-frame
 * drift figure where no CAD model exists.  The reference has nothing of the kind (its _need_reinit is set and never read), so the
 * rules below are this project's own; every decision is exact, so a CPU restatement (tests/register_ref.py) reproduces each of them, and
 * every sum is fp64 in a fixed order.
 *
 * An item is a btba_fuse_segment: `instance` names the model, `pose` is the INITIAL camera -> model pose, colour is not read.  A model is
 * the output of the fusion call for n_instances instances with its `capacity` stride: xyz_dev and normal_dev (float4 [n_instances][capacity],
 * both required), the host box, and the cell index btba_register_index builds from lin_out and n_out.  Fuse the model with
 * normalize_normals = 1: the registration does NOT renormalise the model normals, and the residual is a distance only along a unit normal.
 *
 * btba_register_index: cell_index_dev is a caller-owned int32 [V] (V and the instances' first voxels: btba_fuse_layout).  Every cell is set to
 * -1, then cell_index[vox_off[b] + lin[b][k]] = k for k < min(n_out[b], capacity) (n_out is read on the device; a lin outside the
 * instance's box is ignored).  Asynchronous; the index serves every later call on that cloud.
 *
 * Per Gauss-Newton iteration and item, at the item's current fp32 pose T (uncontracted fp32 in the order written, rules 1 - 4):
 *   1. Points are taken and dropped exactly as btba_fuse_frames takes and drops them (the same device function): backprojection, (double)d
 *      >= 0.1, a zero normal under require_normals, a non-finite list point.  q_r = ((T_r0 x + T_r1 y) + T_r2 z) + T_r3; n'_r likewise from
 *      the source normal (fusion's rule 1, its 2^16 clamp included).  n_valid counts the survivors.
 *   2. Cell i_a = (int)floorf(q_a * inv_leaf) - min_b_a, inv_leaf = 1.0f / leaf formed once on the host.  No candidates when some |q_a| is not
 *      below 2^16 (NaN included).  Candidates: the cells i + o, o in [-r, r]^3, r = search_radius, oz outermost and ox innermost (ascending
 *      lin), each tested on its own against 0 <= . < dims (the centre may lie outside the box while neighbours lie inside), with a record
 *      k = cell_index[.] in 0 .. capacity - 1.  d_a = q_a - m_a, d2 = (dx dx + dy dy) + dz dz.  The first candidate is taken; a later one
 *      replaces it only when its d2 is strictly smaller, so a tie goes to the lowest lin.
 *   3. Gates, after the selection: d2 <= max_dist^2 (the square formed once on the host in fp32); the model normal m_n not exactly (0, 0, 0);
 *      and, when the segment has a normal map and min_cos > -1, (n'x mx + n'y my) + n'z mz >= min_cos.
 *   4. r = (nx dx + ny dy) + nz dz with n = m_n, and the row a = (q x n, n) in the public (rot, trans) order, each cross term two products and
 *      one subtraction: (qy nz - qz ny, qz nx - qx nz, qx ny - qy nx, nx, ny, nz).
 *   5. In fp64, the factors promoted exactly: w = 1 when |r| <= huber_delta, else (double)delta / fabs((double)r) (such a point counts in
 *      n_beyond); rho = r^2 inside the knee, 2 delta |r| - delta^2 outside; H_ab += w a_a a_b over the 21 entries of the lower triangle
 *      (row-major: (a, b), b <= a, at a (a + 1) / 2 + b), g_a += w a_a r, cost += rho.  No float atomics: points 2048 k .. 2048 k + 2047 of a
 *      segment are summed by one workgroup in a fixed tree and the workgroups' records in index order, so the sums have the same bytes at
 *      any batch position, with any n_items, and from run to run.
 *   6. Fewer than min_matches matched points: BTBA_REG_TOO_FEW.  Otherwise H xi = -g by Cholesky in IEEE fp64; pivot_ratio = min_j d_j / H_jj
 *      over the pivots d_j, as btba_pose_covariances defines it, and 0 for a failed factorisation; a pivot that is not positive and finite is
 *      BTBA_REG_DEGENERATE (xi = 0).  On TOO_FEW or DEGENERATE the pose stays as it is and the item stops.
 *   7. T <- Exp(xi) T in fp64, xi = (omega, u): R = I + (sin t / t) K + ((1 - cos t) / t^2) K^2, V = I + ((1 - cos t) / t^2) K + ((t - sin t) /
 *      t^3) K^2 with K = [omega]x, t = |omega|; below t = 1e-12, R = I + K and V = I + K / 2.  The fp32 pose is promoted, multiplied and its 12
 *      entries are rounded to fp32 once.  There is NO re-orthonormalisation: 64 roundings move the rotation off SO(3) by about 1e-6.
 *   8. |omega| < eps_rot and |u| < eps_trans (fp64; 0 disables a threshold's side, and with it the stop) ends the item BTBA_REG_CONVERGED after
 *      the step.  A device-side flag makes every later launch skip a stopped item; its later trace entries are zero-filled with status
 *      BTBA_REG_SKIPPED.  An item still running after n_iters ends BTBA_REG_MAX_ITERS.
 * After the loop ONE more accumulation pass, without a solve, evaluates every item at its pose_out: the result's n_valid, n_matched, n_beyond
 * and cost belong to pose_out.  A call with n_iters = 0 is therefore the pose check: pose_out = the initial pose, status BTBA_REG_TOO_FEW
 * when n_matched < min_matches and BTBA_REG_MAX_ITERS otherwise, and its four evaluated fields equal, byte for byte, those of the call that
 * produced that pose.  trace_dev (NULL or [n_items][n_iters]) records every iteration: the sums at the pose the iteration started from, the
 * step, and the pose after it (status BTBA_REG_MAX_ITERS there means "stepped, still running").
 *
 * btba_register_associate runs rule 1 - 3 once at the segments' poses (the accumulate kernel's own device function) and writes per point of
 * item i to match_out[i] ([H*W] or [n] int32 on the device; match_out itself is a host array): the matched record k, or -1 no candidate, -2
 * beyond max_dist, -3 a zero model normal or a failed normal gate, -4 the point was dropped.
 *
 * All three calls are asynchronous on the workspace stream with no host synchronisation inside; items go in chunks of BTBA_FUSE_CHUNK as
 * kernel arguments, so no host memory is read after a call returns.  The scratch (partial records, current poses, flags) is grow-only in
 * the workspace.  BTBA_EINVAL, decided before the first launch: NULL ws, params, segments (n_items > 0), box, xyz_dev, normal_dev,
 * cell_index_dev, pose_out_dev, result_dev (match_out or one of its entries with points; lin_dev, n_out_dev for the index); n_instances < 1,
 * n_items < 0, capacity < 0 or n_instances * capacity beyond 2^31 - 1; search_radius outside 0 .. 2, n_iters outside 0 .. 64, max_dist or
 * huber_delta not finite, max_dist < 0, huber_delta <= 0, min_cos NaN, eps_rot or eps_trans negative or NaN, min_matches < 0; a leaf, a
 * segment or a box that btba_fuse_frames refuses (instance outside 0 .. n_instances - 1 among them); float4 arrays not 16-byte aligned, the
 * cell index, lin, n_out, pose_out or a match array not 4-byte aligned, result_dev or trace_dev not 8-byte aligned; more than 2^22 blocks
 * of 2048 points in one call. */
#define BTBA_REG_CONVERGED 0
#define BTBA_REG_MAX_ITERS 1
#define BTBA_REG_DEGENERATE 2
#define BTBA_REG_TOO_FEW 3
#define BTBA_REG_SKIPPED 4                /* trace entries only: the item had stopped before this iteration */
#define BTBA_REG_MAX_ITERATIONS 64
typedef struct btba_register_params {     /* 44 bytes */
    float leaf;                           /* the model's voxel side (no default: must equal the leaf the cloud was fused with) */
    int32_t search_radius;                /* 1 (default; 0 .. 2): voxels searched around the point's cell, 1 = 27 cells */
    float max_dist;                       /* 0.02 (default): |q - m| gate, the dense sweep's */
    float min_cos;                        /* cos 45 deg (default): normal gate, the dense sweep's; <= -1 switches it off */
    float huber_delta;                    /* 0.005 (default): Huber knee in metres */
    int32_t n_iters;                      /* 10 (default; 0 .. 64): Gauss-Newton iterations */
    float eps_rot, eps_trans;             /* 1e-5 rad, 1e-6 m (defaults): convergence thresholds, 0 disables */
    int32_t min_matches;                  /* 6 (default) */
    int32_t require_normals;              /* 1 (default, as fusion's): frame pixels with a zero normal are dropped */
    int32_t reserved;                     /* 0 */
} btba_register_params;
typedef struct btba_register_iter {       /* 344 bytes */
    int32_t n_valid, n_matched, n_beyond, status;
    double cost;
    double H[21];                         /* lower triangle, row-major */
    double g[6];
    double xi[6];                         /* (omega, u) */
    double pivot_ratio;
    float pose[12];                       /* rows 0 .. 2 of the pose after the step */
} btba_register_iter;
typedef struct btba_register_result {     /* 32 bytes */
    int32_t status, iters_done;           /* iters_done: iterations that accumulated for the item, the one it stopped in included */
    int32_t n_valid, n_matched, n_beyond, reserved;      /* at pose_out */
    double cost;                          /* at pose_out */
} btba_register_result;
BTBA_API void btba_register_params_default(btba_register_params *p);
BTBA_API int btba_register_index(btba_workspace *ws, int n_instances, const int32_t *box /* host [n_instances][6] */, int capacity,
                                 const int32_t *lin_dev /* [n_instances][capacity] */, const int32_t *n_out_dev /* [n_instances] */,
                                 int32_t *cell_index_dev /* [V] */);
BTBA_API int btba_register_frames(btba_workspace *ws, const btba_register_params *params, int n_instances, int n_items,
                                  const btba_fuse_segment *segments, int H, int W, const float *K_rowmajor,
                                  const int32_t *box /* host [n_instances][6] */, int capacity,
                                  const float *xyz_dev, const float *normal_dev /* float4 [n_instances][capacity] each */,
                                  const int32_t *cell_index_dev, float *pose_out_dev /* [n_items][12] */,
                                  btba_register_result *result_dev /* [n_items] */,
                                  btba_register_iter *trace_dev /* NULL or [n_items][n_iters] */);
BTBA_API int btba_register_associate(btba_workspace *ws, const btba_register_params *params, int n_instances, int n_items,
                                     const btba_fuse_segment *segments, int H, int W, const float *K_rowmajor,
                                     const int32_t *box, int capacity, const float *xyz_dev, const float *normal_dev,
                                     const int32_t *cell_index_dev, int32_t *const *match_out /* host [n_items] of device int32 [H*W] or [n] */);

/* ---- device keyframe memory ---------------------------------------------------------------------------------------------------------
 * The "memory" of the memory-augmented pose graph for many tracking sessions at once: Bundler::checkAndAddKeyframe and
 * Bundler::selectKeyFramesForBA (Bundler.cpp:185-274) with Utils::rotationGeodesicDistance (Utils.cpp:42-47), on device memory.  Every
 * call is asynchronous on the workspace stream (export alone synchronises), none uses atomics, and a session's bytes depend on that
 * session alone: the same session gives the same bytes at any batch position and from run to run.
 *
 * The distance is acos(clamp((tr(R1 R2^T) - 1) / 2)): the trace and the clamp in the reference's own float arithmetic, the arc cosine by
 * the memory's own function -- fp64 from IEEE-exact operations in a fixed order, rounded once to float -- so that the host compiler, numpy
 * and the device give the same bits (bundletrack_amd/csrc/btba_keyframes_point.hpp; the C library's acosf differs from it by at most one
 * float ulp).  btba_rotation_distances evaluates it for n pose pairs (row-major 4 x 4 floats, only the rotation blocks are read).
 *
 * btba_keyframes_create: n_sessions >= 1 pools of `capacity` >= 1 keyframes, n_sessions * capacity <= 2^24, max_BA_frames 2 .. 85; the
 * select kernel's table (capacity * max_BA_frames floats and a little more) must fit 160 KB of LDS -- about 1024 keyframes at
 * max_BA_frames <= 32.  Anything else is BTBA_EINVAL; nothing is ever truncated.  _destroy does not touch the workspace.  _reset empties one
 * session's pool (or all: -1) and its overflow counter.
 *
 * Per-session arguments are device arrays [n_sessions]; active_dev (int32, nonzero = take part) may be NULL: all sessions.  An inactive
 * session's state and outputs keep their bytes.
 *   _check_add : one frame per session.  frame_id 0 always joins; any other frame needs status_other != 0, n_keypts >= min_feat_num and
 *                (float)((double)(distance * 180) / pi) >= min_rot_deg against EVERY pool member.  added_out: 1 joined (the next slot), 0 not,
 *                -1 would have joined a full pool -- overflow[s] is incremented and nothing is written.  frame_key_dev may be NULL (keys 0).
 *   _select    : the window for a new frame that is not in the pool.  count + 1 <= max_BA_frames: every keyframe and the new frame.
 *                Otherwise the new frame, slot 0, then in every round the slot with the SMALLEST cum_dist: the float sum of its distances
 *                to the chosen set, summed over the chosen slots ascending and the new frame last; strict `<`, the lowest slot on ties.
 *                Rows are ordered by frame id (on equal ids a pool slot before the new frame, lower slots first): window_slot_out
 *                [S][max_BA] (-1: the new frame), window_frame_id_out, window_frame_key_out, window_pose_out [S][max_BA][16], n_window_out
 *                [S] rows, newframe_index_out [S] the new frame's row.  Rows at and past n_window keep their bytes.
 *   _writeback : pose_dev [S][max_BA][16] rows 0 .. n_window - 1 go to the pool slots window_slot names (Bundler.cpp:353-357); rows of the
 *                new frame (-1) and slots outside the pool are skipped.
 *   _export    : a synchronising host copy, for tests and host adapters: count_out, overflow_out [S], frame_id_out, frame_key_out [S][capacity],
 *                pose_out [S][capacity][16]; any may be NULL.  Slots at and past count hold stale or zero bytes. */
typedef struct btba_keyframes btba_keyframes;
BTBA_API int btba_keyframes_create(btba_workspace *ws, int n_sessions, int capacity, int max_BA_frames, btba_keyframes **out);
BTBA_API void btba_keyframes_destroy(btba_keyframes *kf);
BTBA_API int btba_keyframes_reset(btba_keyframes *kf, int session /* -1: all */);
BTBA_API int btba_keyframes_check_add(btba_keyframes *kf, float min_rot_deg, int min_feat_num, const int32_t *active_dev,
                                      const float *pose_dev /* [S][16] */, const int32_t *frame_id_dev, const uint64_t *frame_key_dev,
                                      const int32_t *status_other_dev, const int32_t *n_keypts_dev, int32_t *added_out_dev);
BTBA_API int btba_keyframes_select(btba_keyframes *kf, const int32_t *active_dev, const float *newpose_dev /* [S][16] */,
                                   const int32_t *new_frame_id_dev, const uint64_t *new_frame_key_dev, int32_t *n_window_out,
                                   int32_t *window_slot_out, int32_t *window_frame_id_out, uint64_t *window_frame_key_out,
                                   float *window_pose_out, int32_t *newframe_index_out);
BTBA_API int btba_keyframes_writeback(btba_keyframes *kf, const int32_t *active_dev, const int32_t *n_window_dev,
                                      const int32_t *window_slot_dev, const float *pose_dev /* [S][max_BA][16] */);
BTBA_API int btba_keyframes_export(btba_keyframes *kf, int32_t *count_out, int32_t *overflow_out, int32_t *frame_id_out,
                                   uint64_t *frame_key_out, float *pose_out);
BTBA_API int btba_rotation_distances(btba_workspace *ws, int n, const float *A_dev, const float *B_dev /* [n][16] each */,
                                     float *dist_out_dev /* [n] */);

#ifdef __cplusplus
}
#endif
#endif /* BTBA_H_ */
