// btba_fusion.hpp -- keyframe fusion and voxel-grid downsampling (btba_fuse_bounds / btba_fuse_frames, include/btba.h): posed
// keyframes (depth, normal and colour maps) and unorganised clouds -> one voxel-grid cloud per instance.  The cloud primitive is
// Utils::downsamplePointCloud = pcl::VoxelGrid (src/Utils.cpp:134-140; restated from PCL's public header, unverified against a
// PCL run: PCL is not available to this project).
//
// Segments travel in chunks of BTBA_FUSE_CHUNK as kernel arguments (as btba_ingest_frames' frames do), so an asynchronous call
// keeps no host memory alive.  Launches of one btba_fuse_frames call:
//   k_fuse_accumulate    per chunk, grid (pixel / point blocks, segment): grid-stride over the segment's pixels or points.  An
//                        invalid pixel costs its depth load and nothing else.  Every surviving point adds into its voxel's planes
//                        (btba_fusion_layout.hpp) with 32- and 64-bit INTEGER atomicAdd, so the sums do not depend on arrival
//                        order; points outside the box are counted per thread, folded per wave and added once per wave.
//   k_fuse_block_counts  per chunk of instances, grid (block, instance): qualifying voxels (count >= min_points) of each
//                        1 024-voxel block, from the count plane alone
//   k_fuse_scan          one workgroup per instance: exclusive scan of its block counts in place, n_out and status
//   k_fuse_scatter       grid as k_fuse_block_counts: ranks the block's qualifying voxels in index order behind the block's offset,
//                        forms the means and writes the outputs below the capacity
// and of btba_fuse_bounds: k_fuse_bounds_init, k_fuse_bounds per chunk (at most 64 workgroups per segment; per-thread min / max of
// floorf(p inv_leaf), folded per wave and through LDS per workgroup, six integer atomicMin / atomicMax per workgroup: with six per wave
// of a 1 024-workgroup grid the pass took 0.31 ms for 15 frames, three times the fusion itself, all of it same-address atomics),
// k_fuse_bounds_finish (max -> dims).
// Same-address atomics: neighbouring pixels often share a voxel.  Equal-voxel lanes of a wave are NOT combined before the atomic.
// The measured split (profiles/fusion_timing.json) shows the accumulate launch dominating the call and following the
// number of atomics per point: combining is the next step, not built here.
#pragma once
#include <hip/hip_runtime.h>
#include <climits>
#include <cstdint>
#include "../../include/btba.h"
#include "btba_fusion_point.hpp"
#include "btba_fusion_layout.hpp"

namespace btba {

constexpr double kFuseScale = 1048576.0;               // 2^20

struct FuseSegments {                                  // one chunk, structure-of-arrays; 108 bytes per segment
    const void *geom[kFuseChunk];                      // frame: float depth [H*W]; list: float4 xyz [n]
    const float4 *normal[kFuseChunk];                  // or nullptr
    const uchar4 *colour[kFuseChunk];                  // or nullptr
    float pose[kFuseChunk][12];                        // rows 0 .. 2 of camera -> model
    int32_t n[kFuseChunk];                             // pixels or points
    int32_t kind_instance[kFuseChunk];                 // instance * 2 + kind
    int32_t min_b[kFuseChunk][3], dims[kFuseChunk][3]; // the instance's box
    uint32_t vox_off[kFuseChunk];                      // the instance's first voxel
};
static_assert(sizeof(FuseSegments) <= 3584, "a chunk of segments travels as a kernel argument");

struct FusePlanes {
    uint32_t *count;
    unsigned long long *xyz, *normal;                  // int64 sums as two's-complement words; normal nullptr = not accumulated
    uint32_t *colour;                                  // nullptr = not accumulated
    size_t stride;
};

struct FuseInstances {                                 // one chunk of instances for the compaction launches
    uint32_t vox_off[kFuseChunk], blk_off[kFuseChunk];
    int32_t n_vox[kFuseChunk];
};

struct FuseOutputs {
    float4 *xyz, *normal;                              // [n_instances][capacity]; normal, colour, count, lin may be nullptr
    uchar4 *colour;
    uint32_t *count;
    int32_t *lin;
    int32_t *n_out, *status;
    int capacity;
};

// The model-frame point (and normal) of element e of segment z (fuse_point_at, btba_fusion_point.hpp)
__device__ __forceinline__ bool fuse_point(const FuseSegments &S, int z, int e, int W, const Mat4 &Kinv, bool require_normals, bool want_normal,
                                           float3 &p, float3 &nrm)
{
    return fuse_point_at((S.kind_instance[z] & 1) == BTBA_FUSE_FRAME, S.geom[z], S.normal[z], S.pose[z], e, W, Kinv, require_normals, want_normal, p, nrm);
}

__global__ void __launch_bounds__(256) k_fuse_bounds_init(int n_instances, int32_t *box)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < 6 * n_instances) box[t] = (t % 6) < 3 ? INT_MAX : INT_MIN;
}

__global__ void __launch_bounds__(256) k_fuse_bounds(int W, Mat4 Kinv, float inv_leaf, int require_normals, const FuseSegments S, int32_t *box)
{
    const int z = blockIdx.y, n = S.n[z];
    int lo[3] = { INT_MAX, INT_MAX, INT_MAX }, hi[3] = { INT_MIN, INT_MIN, INT_MIN };
    for (int e = blockIdx.x * 256 + threadIdx.x; e < n; e += gridDim.x * 256) {
        float3 p, nrm;
        int c[3];
        if (!fuse_point(S, z, e, W, Kinv, require_normals != 0, false, p, nrm) || !fuse_cell(p, inv_leaf, c[0], c[1], c[2])) continue;
        for (int a = 0; a < 3; a++) { lo[a] = min(lo[a], c[a]); hi[a] = max(hi[a], c[a]); }
    }
    // fold: lanes -> wave -> workgroup (LDS), then six atomics per workgroup that saw a point: all of an instance's go to the same six words
    __shared__ int red[4][6];
    const int w = threadIdx.x >> 6;
    for (int a = 0; a < 3; a++) {
        const int l = wave_min_i(lo[a]), h = wave_max_i(hi[a]);
        if ((threadIdx.x & 63) == 0) { red[w][a] = l; red[w][3 + a] = h; }
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int a = threadIdx.x;
        int32_t *b = box + 6 * (size_t)(S.kind_instance[z] >> 1);
        if (a < 3) {
            const int l = min(min(red[0][a], red[1][a]), min(red[2][a], red[3][a]));
            if (l != INT_MAX) atomicMin(b + a, l);
        } else {
            const int h = max(max(red[0][a], red[1][a]), max(red[2][a], red[3][a]));
            if (h != INT_MIN) atomicMax(b + a, h);
        }
    }
}

// (min, max) -> (min_b, dims); an instance without a surviving point gets six zeros.  A side of 2^31 or more cannot occur: |floor| < 2^30.
__global__ void __launch_bounds__(256) k_fuse_bounds_finish(int n_instances, int32_t *box)
{
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= n_instances) return;
    int32_t *q = box + 6 * (size_t)b;
    const bool empty = q[0] > q[3];
    for (int a = 0; a < 3; a++) {
        const int lo = q[a], hi = q[3 + a];
        q[a] = empty ? 0 : lo;
        q[3 + a] = empty ? 0 : hi - lo + 1;
    }
}

__global__ void __launch_bounds__(256) k_fuse_accumulate(int W, Mat4 Kinv, float inv_leaf, int require_normals, const FuseSegments S, const FusePlanes P,
                                                         int32_t *n_outside)
{
    const int z = blockIdx.y, n = S.n[z];
    const int mx = S.min_b[z][0], my = S.min_b[z][1], mz = S.min_b[z][2], dx = S.dims[z][0], dy = S.dims[z][1], dz = S.dims[z][2];
    const uchar4 *cmap = P.colour ? S.colour[z] : nullptr;
    int outside = 0;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < n; e += gridDim.x * 256) {
        float3 p, nrm;
        if (!fuse_point(S, z, e, W, Kinv, require_normals != 0, P.normal != nullptr, p, nrm)) continue;
        int cx, cy, cz;
        if (!fuse_cell(p, inv_leaf, cx, cy, cz)) { outside++; continue; }
        const long long ix = (long long)cx - mx, iy = (long long)cy - my, iz = (long long)cz - mz;
        if (ix < 0 || ix >= dx || iy < 0 || iy >= dy || iz < 0 || iz >= dz) { outside++; continue; }
        const size_t v = (size_t)S.vox_off[z] + (size_t)(ix + dx * (iy + dy * iz));
        atomicAdd(P.count + v, 1u);
        atomicAdd(P.xyz + v, (unsigned long long)__double2ll_rn((double)p.x * kFuseScale));
        atomicAdd(P.xyz + P.stride + v, (unsigned long long)__double2ll_rn((double)p.y * kFuseScale));
        atomicAdd(P.xyz + 2 * P.stride + v, (unsigned long long)__double2ll_rn((double)p.z * kFuseScale));
        if (P.normal) {
            atomicAdd(P.normal + v, (unsigned long long)__double2ll_rn((double)nrm.x * kFuseScale));
            atomicAdd(P.normal + P.stride + v, (unsigned long long)__double2ll_rn((double)nrm.y * kFuseScale));
            atomicAdd(P.normal + 2 * P.stride + v, (unsigned long long)__double2ll_rn((double)nrm.z * kFuseScale));
        }
        if (cmap) {
            const uchar4 c = cmap[e];
            atomicAdd(P.colour + v, (uint32_t)c.x);
            atomicAdd(P.colour + P.stride + v, (uint32_t)c.y);
            atomicAdd(P.colour + 2 * P.stride + v, (uint32_t)c.z);
        }
    }
    outside = wave_sum_i(outside);
    if ((threadIdx.x & 63) == 0 && outside) atomicAdd(n_outside + (S.kind_instance[z] >> 1), outside);
}

// qualifying voxels among the kFuseVoxelsPerThread consecutive ones of this thread (flags in the low bits of `mask`)
__device__ __forceinline__ int fuse_thread_voxels(const uint32_t *count, uint32_t first, int n_vox, int block, uint32_t min_points, unsigned &mask)
{
    const int base = block * kFuseBlockVoxels + (int)threadIdx.x * kFuseVoxelsPerThread;
    int q = 0;
    mask = 0;
    for (int k = 0; k < kFuseVoxelsPerThread; k++)
        if (base + k < n_vox && count[(size_t)first + base + k] >= min_points) { mask |= 1u << k; q++; }
    return q;
}

// exclusive rank of this thread's value among the workgroup's 256, and the workgroup's total; lds: 4 ints
__device__ __forceinline__ int fuse_block_rank(int q, int *lds, int &total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = q;
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(inc, o);
        if (lane >= o) inc += up;
    }
    if (lane == 63) lds[w] = inc;
    __syncthreads();
    int before = 0;
    total = 0;
    for (int k = 0; k < 4; k++) { if (k < w) before += lds[k]; total += lds[k]; }
    __syncthreads();
    return before + inc - q;
}

__global__ void __launch_bounds__(kFuseBlockThreads) k_fuse_block_counts(const FuseInstances I, const uint32_t *count, uint32_t min_points, uint32_t *block_counts)
{
    __shared__ int lds[4];
    const int b = blockIdx.y, n_vox = I.n_vox[b], block = blockIdx.x;
    if ((int64_t)block * kFuseBlockVoxels >= n_vox) return;      // (uniform)
    unsigned mask;
    int total;
    (void)fuse_block_rank(fuse_thread_voxels(count, I.vox_off[b], n_vox, block, min_points, mask), lds, total);
    if (threadIdx.x == 0) block_counts[(size_t)I.blk_off[b] + block] = (uint32_t)total;
}

// grid (instances of the chunk), 256 threads: the instance's block counts become exclusive offsets; n_out is their sum even beyond the capacity
__global__ void __launch_bounds__(256) k_fuse_scan(const FuseInstances I, int first_instance, uint32_t *block_counts, int capacity, int32_t *n_out, int32_t *status)
{
    __shared__ int lds[4];
    const int b = blockIdx.x;
    const int n_blk = (int)fuse_blocks(I.n_vox[b]);
    uint32_t *c = block_counts + I.blk_off[b];
    int running = 0;
    for (int k0 = 0; k0 < n_blk; k0 += 256) {
        const int k = k0 + (int)threadIdx.x;
        const int q = k < n_blk ? (int)c[k] : 0;
        int total;
        const int r = fuse_block_rank(q, lds, total);
        if (k < n_blk) c[k] = (uint32_t)(running + r);
        running += total;
    }
    if (threadIdx.x == 0) {
        n_out[first_instance + b] = running;
        status[first_instance + b] = running > capacity ? BTBA_FUSE_OVERFLOW : 0;
    }
}

__global__ void __launch_bounds__(kFuseBlockThreads) k_fuse_scatter(const FuseInstances I, int first_instance, const FusePlanes P, const uint32_t *block_counts,
                                                                    uint32_t min_points, int normalize_normals, const FuseOutputs O)
{
#pragma clang fp contract(off)
    __shared__ int lds[4];
    const int b = blockIdx.y, n_vox = I.n_vox[b], block = blockIdx.x;
    if ((int64_t)block * kFuseBlockVoxels >= n_vox) return;      // (uniform)
    unsigned mask;
    int total;
    int rank = fuse_block_rank(fuse_thread_voxels(P.count, I.vox_off[b], n_vox, block, min_points, mask), lds, total);
    rank += (int)block_counts[(size_t)I.blk_off[b] + block];
    const int base = block * kFuseBlockVoxels + (int)threadIdx.x * kFuseVoxelsPerThread;
    const size_t out0 = (size_t)(first_instance + b) * (size_t)O.capacity;
    for (int k = 0; k < kFuseVoxelsPerThread; k++) {
        if (!(mask >> k & 1u)) continue;
        const int slot = rank++;
        if (slot >= O.capacity) break;                            // later voxels of this thread rank higher still
        const size_t v = (size_t)I.vox_off[b] + base + k, o = out0 + slot;
        const uint32_t n = P.count[v];
        const double dn = (double)n;
        auto mean = [&](const unsigned long long *plane, int a) { return (float)((double)(long long)plane[a * P.stride + v] / kFuseScale / dn); };
        O.xyz[o] = make_float4(mean(P.xyz, 0), mean(P.xyz, 1), mean(P.xyz, 2), 1.0f);
        if (O.normal) {
            float nx = mean(P.normal, 0), ny = mean(P.normal, 1), nz = mean(P.normal, 2);
            if (normalize_normals) {
                const float l = sqrtf((nx * nx + ny * ny) + nz * nz);
                if (l > 0.0f) { nx = nx / l; ny = ny / l; nz = nz / l; }
                else nx = ny = nz = 0.0f;
            }
            O.normal[o] = make_float4(nx, ny, nz, 0.0f);
        }
        if (O.colour) {
            auto ch = [&](int a) { return (unsigned char)((2ull * P.colour[a * P.stride + v] + n) / (2ull * n)); };
            O.colour[o] = make_uchar4(ch(0), ch(1), ch(2), 0);
        }
        if (O.count) O.count[o] = n;
        if (O.lin) O.lin[o] = base + k;
    }
}

}  // namespace btba
