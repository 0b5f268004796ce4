// btba_fusion_layout.hpp -- voxel offsets, compaction blocks and scratch layout of keyframe fusion (btba_fuse_frames, include/btba.h).
// No HIP: the kernels (btba_fusion.hpp) index the planes with it, the host (btba_api_fusion.hip: btba_fuse_layout and the scratch of
// btba_fuse_frames) sizes them with it, and tests/cpp/fusion_host.cpp walks it under the host sanitizers.
//
// Instance b owns the voxels [vox_off[b], vox_off[b + 1]) of every plane; voxel (ix, iy, iz) of its box sits at
// vox_off[b] + ix + dims_x (iy + dims_y iz).  The planes are structure-of-arrays over all V voxels of the call, 64 bytes per voxel:
//   count   uint32 [V]          the plane compaction sweeps: 4 bytes per voxel
//   xyz     int64  [3][V]       sum llrint(p_a 2^20)
//   normal  int64  [3][V]       sum llrint(n_a 2^20)      (cleared and read only when a normal output is asked for)
//   colour  uint32 [3][V]       sum of each colour byte    (cleared and read only when a colour output is asked for)
// in that order, so the planes every call clears are one contiguous prefix.  Behind them: one uint32 per compaction block (a block is
// kFuseBlockVoxels consecutive voxels of ONE instance; instance b owns the blocks [blk_off[b], blk_off[b + 1])).
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define BTBA_FUSION_HD __host__ __device__
#else
#define BTBA_FUSION_HD
#endif

namespace btba {

constexpr int64_t kFuseMaxVoxels = (int64_t)1 << 24;      // BTBA_FUSE_MAX_VOXELS: 1 GiB of planes
constexpr int kFuseBlockThreads = 256, kFuseVoxelsPerThread = 4;
constexpr int kFuseBlockVoxels = kFuseBlockThreads * kFuseVoxelsPerThread;      // 1024

struct FuseLayout {
    int64_t voxels = 0, blocks = 0;                        // V and the number of compaction blocks of the call
    size_t count = 0, xyz = 0, normal = 0, colour = 0, block_counts = 0, total = 0;      // byte offsets, each a multiple of 256
    size_t plane_stride = 0;                               // voxels between two planes of a sum: V rounded up to 32 (256 bytes of int64)
};

// voxels of one box, in 64 bits; -1 for a negative side or a box that alone exceeds the cap (sides near 2^31 must not wrap)
inline int64_t fuse_box_voxels(const int32_t *dims)
{
    if (dims[0] < 0 || dims[1] < 0 || dims[2] < 0) return -1;
    if (dims[0] == 0 || dims[1] == 0 || dims[2] == 0) return 0;
    const int64_t xy = (int64_t)dims[0] * dims[1];         // < 2^62
    if (xy > kFuseMaxVoxels) return -1;
    const int64_t v = xy * dims[2];                        // <= 2^24 * 2^31
    return v > kFuseMaxVoxels ? -1 : v;
}

BTBA_FUSION_HD inline int64_t fuse_blocks(int64_t voxels) { return (voxels + kFuseBlockVoxels - 1) / kFuseBlockVoxels; }

// box: [n_instances][6] = (min_b[3], dims[3]).  vox_off / blk_off: [n_instances + 1], either may be null.  false: a negative side, or more
// than kFuseMaxVoxels voxels in all.
inline bool fuse_layout(int n_instances, const int32_t *box, int64_t *vox_off, int64_t *blk_off, FuseLayout *L)
{
    int64_t v = 0, nb = 0;
    for (int b = 0; b < n_instances; b++) {
        const int64_t vb = fuse_box_voxels(box + 6 * (size_t)b + 3);
        if (vb < 0) return false;
        if (vox_off) vox_off[b] = v;
        if (blk_off) blk_off[b] = nb;
        v += vb;
        nb += fuse_blocks(vb);
        if (v > kFuseMaxVoxels) return false;
    }
    if (vox_off) vox_off[n_instances] = v;
    if (blk_off) blk_off[n_instances] = nb;
    if (L) {
        auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
        L->voxels = v;
        L->blocks = nb;
        L->plane_stride = ((size_t)v + 31) & ~(size_t)31;
        L->count = 0;
        L->xyz = up(sizeof(uint32_t) * (size_t)v);
        L->normal = L->xyz + 3 * sizeof(int64_t) * L->plane_stride;
        L->colour = L->normal + 3 * sizeof(int64_t) * L->plane_stride;
        L->block_counts = L->colour + up(3 * sizeof(uint32_t) * L->plane_stride);
        L->total = L->block_counts + up(sizeof(uint32_t) * (size_t)nb);
    }
    return true;
}

}  // namespace btba
