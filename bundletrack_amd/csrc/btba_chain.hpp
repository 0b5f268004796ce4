// btba_chain.hpp -- the chained launch: k_chain and what it needs (ChainDims, the wait, the watchdog's poison kernel, k_prepare_strided).
// Its solve items run system_solve_body<CHAIN> (btba_solve_general.hpp); its LDS budget and region R are sized in btba_solve_layout.hpp.
#pragma once
#include "btba_solve_general.hpp"

namespace btba {

// ---- the chained launch: ALL Gauss-Newton iterations of a batch in ONE launch --------------------------------------------------------------
// The plain schedule is 2 launches per iteration: the fused sweeps (every compute unit busy, then 12-15 % of the launch draining at falling
// occupancy), then k_system_solve (one workgroup per instance: 32 of 256 compute units for ~18 us, VALU busy 0.04) -- seven times per solve, the
// reference's serial tail (PCGInit / PCGStep*, SolverBundling.cu:575-818, 931-1003) in miniature.  Instances are independent, so nothing
// forces instance b's iteration i + 1 to wait for instance c's iteration i.  k_chain puts the work items of all iterations into one grid:
//
//   per XCD x (blocks g = 8 s + x, s = position in the XCD's sequence; the dispatcher places block g on XCD g % 8 and starts an XCD's blocks
//   in order -- observed, used for speed and for forward progress, never for the values computed) and per iteration, for each instance the XCD
//   owns:  [its dense items, heaviest pairs first] [its sparse items] [ONE solve item]
//
//   sweep item (iteration i, instance b): waits until flags[b] >= i (iterate i of b is published: one relaxed agent-scope load per wave, long
//       true in the steady state), does exactly what its k_fused_sweeps workgroup does -- same partial record, bit for bit -- stores the record
//       write-through, drains its stores and adds 1 to arrivals[i][b].
//   solve item (i, b): waits until arrivals[i][b] counts all of b's sweep items, takes an agent-scope acquire, runs system_solve_body<CHAIN>
//       (k_system_solve's sums in k_system_solve's order on 256 threads) from ring slot i into ring slot i + 1, releases at agent scope and
//       sets flags[b] = i + 1.
//
// While instance b is being solved, the compute unit's other five workgroup slots -- and the rest of the chip -- run the sweep items of the
// XCD's other instances; b's next items come up in the sequence (inst_per_xcd - 1) instances later.  No launch boundary, no drain, no idle
// 224 compute units, except once at the very end.
// Forward progress: an item only ever waits for items EARLIER in its own XCD's sequence (all items of an instance sit on one XCD), which are
// resident or finished when it starts; every wait is bounded by a watchdog that raises *error and lets the launch run out (the host then
// reports the solve as failed) -- a misbehaving dispatcher costs a wrong answer that is flagged, never a hung GPU.
// Visibility (MI355X_MICROARCH.md, "inter-workgroup visibility"): every hand-off goes to a region of its own -- ring slot / iteration /
// instance, padded to whole 128-byte lines -- that no workgroup touches before its producer has published it, so no cache can hold an older
// copy of it; producers write through (sweep records: sc1 stores + vmcnt drain) or release at agent scope (solve items) before the relaxed
// agent-scope counter / flag update; the solve item acquires at agent scope; sweep items read the poses through the scalar cache, which they
// invalidate after the wait, and through addresses the compiler cannot move above the wait.
constexpr int kChainMaxParts = 2;     // chunks / tiles per pair the chained solve item reduces (system_solve_body<CHAIN>)
constexpr int kChainMaxFrames = 21;       // (128 lane pairs own the rows of the matrix: 6 N - 6 <= 128; the LDS budget stops at 15 frames before that)
struct ChainDims {
    int n_iter;                 // Gauss-Newton iterations in this launch
    int n_inst;                 // B
    unsigned inst_per_xcd;      // ceil(B / 8): instance b lives on XCD b / inst_per_xcd
    unsigned items_d, items_s;  // sweep items per (instance, iteration): dense_tiles * Pd, sparse_chunks * P
    unsigned sparse_period;     // 0: an instance's sparse items follow its dense items; R >= 2: every R-th slot of the instance is a sparse item until they are used up
    unsigned group;             // instances per GROUP of an XCD's sequence (sparse_period = 0): [dense items of the group's instances][their sparse items][their solve
                                // items] -- the short sparse items then come in fewer, longer runs (1: after every instance; inst_per_xcd: once per iteration)
    int *flags;                 // [B] published iterate of every instance (0 = the k_prepare output): what a waiting wave polls (L2, never a cache above it)
    const int *published;       // [n_iter + 1][B][16]: word 0 of line (e, b) becomes 1 when iterate e of instance b is published -- one 64-byte line per word,
                                // read through the scalar cache: a line that says 1 was fetched after the publication, a line that says 0 may be stale (-> poll flags[b])
    int *arrivals;              // [n_iter][B]
    int *error;                 // != 0: a wait ran into the watchdog (host-visible memory)
    long long timeout_ticks;    // 100 MHz ticks (wall_clock64)
    size_t pose_ring, x_ring;   // floats between two ring slots of T / T^-1, of x
    size_t sp_ring, dp_ring;    // floats between two iterations' sweep partials
    size_t ps_size, A_size;     // floats per (iteration, instance) of the reduced-pair-sum scratch and of the matrix scratch
    unsigned long long *trace;  // developer: per block (start, end of wait, end, kind | it << 8 | b << 16 | hardware id << 32) in 100 MHz ticks, or nullptr
    unsigned long long *stamps; // developer: [n_iter][B][8] phase stamps of the solve items (behind the block records), or nullptr
    int solve_prio;             // s_setprio of a solve item's waves (0 = the default priority of every wave)
    int last_solve_external;    // 1: the solve items of the LAST iteration do nothing -- the host launches k_system_solve for it (16 waves per instance on an
                                // idle chip: ~18 us, against the ~90 us a 4-wave solve item on a busy compute unit would leave exposed at the end of the launch)
    int debug_skip;             // developer TIMING experiments (wrong results by construction): 1 sweep items do not wait, 2 sweep items do not arrive, 4 solve items do not wait, 8 solve items do nothing, 64 solve items do not publish (tests/test_gpu_chain.py: the watchdog)
};

// one wave waits until *word >= want: lane 0 polls with relaxed agent-scope loads (served by L2, never by this CU's L1), sleeping in between
__device__ __forceinline__ void chain_wait_ge(const int *word, int want, const ChainDims &Cn)
{
    const bool lane0 = (item_tid() & 63u) == 0u;
    auto poll = [&]() {
        int v = 0;
        if (lane0) v = __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return __builtin_amdgcn_readfirstlane(v);
    };
    if (poll() >= want) return;
    const long long t0 = wall_clock64();
    for (;;) {
        __builtin_amdgcn_s_sleep(16);
        if (poll() >= want) return;
        if (wall_clock64() - t0 > Cn.timeout_ticks) {
            if (lane0) __hip_atomic_store(Cn.error, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            return;
        }
    }
}

template <int LAYOUT>   // 1: pinhole compact cache, 8 x 8 block walk or strips; 3: the same walking the frames' valid-pixel lists
__global__ void __launch_bounds__(kBlock, BTBA_FUSED_WAVES) k_chain(SolveDims D, ChainDims Cn, const float4 *__restrict__ zn,
                                                    float *T, float *Tinv, float *x, float *dense_partials,
                                                    const float4 *__restrict__ corr, const uint32_t *__restrict__ pair_offsets, float *sparse_partials,
                                                    const uint32_t *__restrict__ valid_lists, const int *__restrict__ valid_counts,
                                                    const int2 *__restrict__ dense_pairs, const int *__restrict__ adj_off, const int *__restrict__ adj,
                                                    const int *__restrict__ solve_tab, float *pairsum_global, float *A_scratch, float *poses_out)
{
    __shared__ float red[kRedFloats];
    extern __shared__ __attribute__((aligned(16))) float dyn_lds[];       // a sweep item's look-up tables, or a solve item's vectors and tables
    const unsigned g = blockIdx.x, xcd = g & 7u, sg = g >> 3;
    const unsigned n_sweep = Cn.items_d + Cn.items_s, slots_per_inst = n_sweep + 1u, per_iter = Cn.inst_per_xcd * slots_per_inst;
    const unsigned it = sg / per_iter, s = sg - it * per_iter;
    unsigned k = s / slots_per_inst, r = s - k * slots_per_inst;
    if (Cn.group > 1u) {
        // groups of `group` instances (the host makes inst_per_xcd a multiple of it): position inside the group -> (instance, kind, index)
        const unsigned per_group = Cn.group * slots_per_inst, gi = s / per_group, rg = s - gi * per_group;
        unsigned kg, rr;
        if (rg < Cn.group * Cn.items_d) { kg = rg / Cn.items_d; rr = rg - kg * Cn.items_d; }
        else if (rg < Cn.group * n_sweep) { const unsigned q = rg - Cn.group * Cn.items_d; kg = q / Cn.items_s; rr = Cn.items_d + (q - kg * Cn.items_s); }
        else { kg = rg - Cn.group * n_sweep; rr = n_sweep; }
        k = gi * Cn.group + kg; r = rr;
    }
    const int b = (int)(xcd * Cn.inst_per_xcd + k);
    if (b >= Cn.n_inst) return;
    const unsigned tid = item_tid();
    const unsigned long long t_start = Cn.trace ? (unsigned long long)wall_clock64() : 0ull;
    unsigned long long t_wait = t_start;
    int kind;
    if (r < n_sweep) {
        // ---- sweep item
        bool is_sparse;
        unsigned idx;                                           // index among the instance's sparse / dense items
        if (Cn.sparse_period >= 2u) {
            const unsigned q = r / Cn.sparse_period, m = r - q * Cn.sparse_period;
            is_sparse = (m == Cn.sparse_period - 1u) && (q < Cn.items_s);
            idx = is_sparse ? q : r - min(q, Cn.items_s);
        } else {
            is_sparse = r >= Cn.items_d;
            idx = is_sparse ? r - Cn.items_d : r;
        }
        const float *T_it = T + (size_t)it * Cn.pose_ring, *Tinv_it = Tinv + (size_t)it * Cn.pose_ring;
        if (it > 0u) {
            // Is iterate `it` of instance b published?  Fast path: its `published` line through the scalar cache (a hit costs ~100 cycles; in the
            // steady state the solve item finished tens of microseconds ago).  The line is this (iterate, instance)'s alone and is only ever
            // fetched by this instance's items of this iteration, so a cached 1 cannot be older than the publication; a 0 may be, and is not
            // trusted: the wave then polls flags[b] in L2.  The poses are read through the scalar cache as well, each 64-byte matrix a line
            // that nobody fetches before this point -- nothing to invalidate -- and through addresses the compiler sees only AFTER the wait, so
            // that no load of a pose can be issued before the publication has been seen (constant-address-space loads may otherwise be hoisted).
            const int seen = (Cn.debug_skip & 1) ? 1 : *as_const(Cn.published + ((size_t)it * Cn.n_inst + b) * 16);
            if (seen == 0) chain_wait_ge(Cn.flags + b, (int)it, Cn);
        }
        asm volatile("" : "+s"(T_it), "+s"(Tinv_it) :: "memory");
        if (Cn.trace) t_wait = (unsigned long long)wall_clock64();
        kind = is_sparse ? 1 : 0;
        if (is_sparse) {
            const int chunk = (int)(idx % (unsigned)D.sparse_chunks), p = (int)(idx / (unsigned)D.sparse_chunks);
            sparse_block(D, corr, pair_offsets, T_it, sparse_partials + (size_t)it * Cn.sp_ring, chunk, p, b, red);
        } else {
            const int tile = D.tile_major ? (int)(idx / (unsigned)D.n_dense_pairs) : (int)(idx % (unsigned)D.dense_tiles);
            const int p = D.tile_major ? (int)(idx % (unsigned)D.n_dense_pairs) : (int)(idx / (unsigned)D.dense_tiles);      // a WORK POSITION (dense_work_item)
            float *dp_it = dense_partials + (size_t)it * Cn.dp_ring;
            if (LAYOUT == 1 && D.walk_blocks) dense_block_pinhole<2>(D, zn, p, T_it, Tinv_it, dp_it, tile, b, red, valid_lists, valid_counts, dyn_lds);
            else if (LAYOUT == 1) dense_block_pinhole<0>(D, zn, p, T_it, Tinv_it, dp_it, tile, b, red, valid_lists, valid_counts, dyn_lds);
            else dense_block_pinhole<1>(D, zn, p, T_it, Tinv_it, dp_it, tile, b, red, valid_lists, valid_counts, dyn_lds);
        }
        // the record was stored write-through by lanes of wave 0: once those stores have been acknowledged, count this item in
        if (tid < 64u && !(Cn.debug_skip & 2)) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (tid == 0u) __hip_atomic_fetch_add(Cn.arrivals + (size_t)it * Cn.n_inst + b, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    } else {
        // ---- solve item: iterate `it` -> iterate `it + 1` of instance b
        kind = 2;
        if ((Cn.debug_skip & 8) || (Cn.last_solve_external && (int)it == Cn.n_iter - 1)) return;
        if (tid < 64u && !(Cn.debug_skip & 4)) {
            chain_wait_ge(Cn.arrivals + (size_t)it * Cn.n_inst + b, (int)n_sweep, Cn);
            if (tid == 0u) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        }
        __syncthreads();
        if (Cn.trace) t_wait = (unsigned long long)wall_clock64();
        const int N = D.n_frames;
        const size_t ib = (size_t)it * Cn.n_inst + b;
        SolveIO io;
        io.sparse_partials = sparse_partials + (size_t)it * Cn.sp_ring + (size_t)b * D.sp_stride;
        io.dense_partials = dense_partials + (size_t)it * Cn.dp_ring + (size_t)b * D.dp_stride;
        io.x_in = x + (size_t)it * Cn.x_ring + (size_t)b * D.x_stride; io.x_out = x + (size_t)(it + 1u) * Cn.x_ring + (size_t)b * D.x_stride;
        io.T_in = T + (size_t)it * Cn.pose_ring + (size_t)b * D.pose_stride;
        io.T_out = T + (size_t)(it + 1u) * Cn.pose_ring + (size_t)b * D.pose_stride;
        io.Tinv_out = Tinv + (size_t)(it + 1u) * Cn.pose_ring + (size_t)b * D.pose_stride;
        io.poses_out = ((int)it == Cn.n_iter - 1) ? poses_out + 16 * (size_t)b * N : nullptr;
        io.pairsum_global = pairsum_global + ib * Cn.ps_size;
        io.A_scratch = A_scratch + ib * Cn.A_size;
        io.trace = nullptr;
        io.stamps = Cn.stamps ? Cn.stamps + 8 * ib : nullptr;
        // a solve item is a chain of short dependent phases on ONE workgroup that shares its compute unit with five sweep workgroups: every
        // instruction of it otherwise queues behind theirs; its instances' next items wait for it, theirs for nothing
        if (Cn.solve_prio == 1) __builtin_amdgcn_s_setprio(1);
        else if (Cn.solve_prio == 2) __builtin_amdgcn_s_setprio(2);
        else if (Cn.solve_prio == 3) __builtin_amdgcn_s_setprio(3);
        system_solve_body<false, false, true, kBlock>(D, (int)it, (int)tid, dyn_lds, io, dense_pairs, adj_off, adj, solve_tab);
        __syncthreads();
        if (tid == 0u && !(Cn.debug_skip & 64)) {           // (64: the watchdog's test -- an iterate that is never published)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // (the compiler may drop the wait behind the write-back: MI355X_MICROARCH.md, compiler hazard)
            __hip_atomic_store(Cn.flags + b, (int)it + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(const_cast<int *>(Cn.published) + ((size_t)(it + 1u) * Cn.n_inst + b) * 16, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (Cn.trace && tid == 0u) {
        unsigned hw, xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)\n s_getreg_b32 %1, hwreg(HW_REG_XCC_ID)" : "=s"(hw), "=s"(xcc));
        unsigned long long *q = Cn.trace + 4 * (size_t)g;
        q[0] = t_start; q[1] = t_wait; q[2] = (unsigned long long)wall_clock64();
        q[3] = (unsigned long long)kind | ((unsigned long long)it << 8) | ((unsigned long long)b << 16) | ((unsigned long long)(hw & 0xFFFFu) << 32) | ((unsigned long long)(xcc & 0xFu) << 48);
    }
}

// after a chained solve: a raised watchdog word (host-visible memory) turns the solve's output poses into NaN
__global__ void __launch_bounds__(256) k_chain_poison(const int *__restrict__ error, float *__restrict__ poses, int n)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < n && __hip_atomic_load(error, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0) poses[e] = __int_as_float(0x7FC00000);
}

// Log / Exp / inverse of the incoming matrices into ring slot 0 of the chained launch (k_prepare with padded instance strides)
__global__ void __launch_bounds__(64) k_prepare_strided(int total, int n_frames, int pose_stride, int x_stride, const float *__restrict__ poses,
                                                        float *__restrict__ x, float *__restrict__ T, float *__restrict__ Tinv)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int b = idx / n_frames, f = idx - b * n_frames;
    const Mat4 M = load_mat4(poses + 16 * (size_t)idx);
    float rot[3], trans[3];
    matrix_to_pose(M, rot, trans);
    float *o = x + (size_t)b * x_stride + 6 * f;
    o[0] = rot[0]; o[1] = rot[1]; o[2] = rot[2]; o[3] = trans[0]; o[4] = trans[1]; o[5] = trans[2];
    se3_opaque(rot, trans);                                        // (as k_prepare: Exp of the pose as a kernel that starts from the stored x forms it)
    const Mat4 E = pose_to_matrix(rot, trans);
    store_mat4(T + (size_t)b * pose_stride + 16 * f, E);
    store_mat4(Tinv + (size_t)b * pose_stride + 16 * f, mat_inverse(E));
}

}  // namespace btba
