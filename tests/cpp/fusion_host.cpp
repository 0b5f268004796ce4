// fusion_host.cpp -- voxel offsets, compaction blocks and the scratch layout of keyframe fusion (bundletrack_amd/csrc/btba_fusion_layout.hpp) on
// the CPU, for a sanitizer build (tests/test_fusion_layout.py):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined tests/cpp/fusion_host.cpp -o tests/cpp/fusion_host
// For every set of boxes: the instances' voxel ranges and block ranges are disjoint, in order and inside the totals; the planes are disjoint,
// 256-byte aligned and inside the stated size; instances with a zero side own nothing; the voxel cap is enforced per box and per call; sides
// near 2^31 are multiplied in 64 bits.  The scratch is allocated for real and every byte a kernel would touch is written, so an overrun is
// AddressSanitizer's to report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../bundletrack_amd/csrc/btba_fusion_layout.hpp"

static void fail(const char *what, long long a, long long b)
{
    std::printf("FAIL %s (%lld, %lld)\n", what, a, b);
    std::exit(1);
}

int main()
{
    using namespace btba;
    int checked = 0;
    const std::vector<std::vector<int32_t>> cases = {
        { 0, 0, 0, 1, 1, 1 },
        { -5, 3, 9, 7, 11, 13 },
        { 0, 0, 0, 32, 32, 1 },                                                      // exactly one block
        { 0, 0, 0, 1025, 1, 1 },                                                     // one voxel into the second block
        { 0, 0, 0, 0, 0, 0 },                                                        // an instance without a point
        { 1, 2, 3, 40, 0, 40 },                                                      // one zero side
        { 0, 0, 0, 17, 19, 23, 4, 4, 4, 0, 0, 0, -1, -1, -1, 33, 31, 3, 0, 0, 0, 5, 5, 0, 9, 9, 9, 1, 1, 2047 },
    };
    for (const auto &box : cases) {
        const int n = (int)box.size() / 6;
        std::vector<int64_t> vo(n + 1, -1), bo(n + 1, -1);
        FuseLayout L;
        if (!fuse_layout(n, box.data(), vo.data(), bo.data(), &L)) fail("a valid layout refused", n, 0);
        if (vo[0] != 0 || bo[0] != 0 || vo[n] != L.voxels || bo[n] != L.blocks) fail("totals", L.voxels, L.blocks);
        for (int b = 0; b < n; b++) {
            const int64_t v = (int64_t)box[6 * b + 3] * box[6 * b + 4] * box[6 * b + 5];
            if (vo[b + 1] - vo[b] != v) fail("voxels of an instance", b, v);
            if (bo[b + 1] - bo[b] != (v + kFuseBlockVoxels - 1) / kFuseBlockVoxels) fail("blocks of an instance", b, v);
            if (v == 0 && (vo[b + 1] != vo[b] || bo[b + 1] != bo[b])) fail("an empty instance owns something", b, 0);
        }
        for (size_t off : { L.count, L.xyz, L.normal, L.colour, L.block_counts, L.total })
            if (off % 256) fail("alignment", (long long)off, 0);
        if (L.plane_stride < (size_t)L.voxels || L.plane_stride % 32) fail("plane stride", (long long)L.plane_stride, L.voxels);
        // write what the kernels write: a counter per byte
        std::vector<unsigned char> scratch(L.total, 0);
        auto touch = [&](size_t off, size_t bytes) {
            for (size_t k = 0; k < bytes; k++) scratch[off + k]++;      // past L.total: AddressSanitizer
        };
        for (int b = 0; b < n; b++) {
            for (int64_t v = vo[b]; v < vo[b + 1]; v++) {
                touch(L.count + 4 * (size_t)v, 4);
                for (int a = 0; a < 3; a++) {
                    touch(L.xyz + 8 * (a * L.plane_stride + (size_t)v), 8);
                    touch(L.normal + 8 * (a * L.plane_stride + (size_t)v), 8);
                    touch(L.colour + 4 * (a * L.plane_stride + (size_t)v), 4);
                }
            }
            for (int64_t k = bo[b]; k < bo[b + 1]; k++) touch(L.block_counts + 4 * (size_t)k, 4);
            // every voxel of the instance lies in exactly one of its blocks, as the compaction kernels walk them
            const int64_t nv = vo[b + 1] - vo[b];
            int64_t seen = 0;
            for (int64_t blk = 0; blk < bo[b + 1] - bo[b]; blk++)
                for (int t = 0; t < kFuseBlockThreads; t++)
                    for (int k = 0; k < kFuseVoxelsPerThread; k++)
                        if (blk * kFuseBlockVoxels + (int64_t)t * kFuseVoxelsPerThread + k < nv) seen++;
            if (seen != nv) fail("voxels walked by the blocks", b, seen);
        }
        for (size_t k = 0; k < L.total; k++) if (scratch[k] > 1) fail("a byte with two owners", n, (long long)k);
        if (L.total < 64 * (size_t)L.voxels) fail("64 bytes per voxel", (long long)L.total, L.voxels);
        checked++;
    }
    // refused: a negative side, the cap per box and per call, sides whose 32-bit product would wrap to something small
    const std::vector<std::vector<int32_t>> refused = {
        { 0, 0, 0, -1, 1, 1 },
        { 0, 0, 0, 256, 256, 257 },
        { 0, 0, 0, 256, 256, 256, 0, 0, 0, 1, 1, 1 },
        { 0, 0, 0, 65536, 65536, 1 },                                                // 2^32: wraps to 0 in 32 bits
        { 0, 0, 0, 2147483647, 2147483647, 2147483647 },
        { 0, 0, 0, 2147483647, 2, 2 },                                               // 2^33 - 4
        { 0, 0, 0, 65536, 65537, 65536 },
    };
    for (const auto &box : refused) {
        FuseLayout L;
        if (fuse_layout((int)box.size() / 6, box.data(), nullptr, nullptr, &L)) fail("an invalid layout accepted", box[3], box[4]);
        checked++;
    }
    // the cap, reached exactly by two instances, is accepted (1 GiB of planes: sized here, not allocated)
    {
        const int32_t box[12] = { 0, 0, 0, 256, 256, 128, 0, 0, 0, 256, 128, 256 };
        int64_t vo[3];
        FuseLayout L;
        if (!fuse_layout(2, box, vo, nullptr, &L) || L.voxels != kFuseMaxVoxels || vo[1] != kFuseMaxVoxels / 2 || L.total < ((size_t)1 << 30))
            fail("the cap itself", L.voxels, (long long)L.total);
        checked++;
    }
    const int32_t near[3] = { 2147483647, 1, 0 };
    if (fuse_box_voxels(near) != 0) fail("a zero side", 0, 0);
    if (fuse_blocks(kFuseMaxVoxels) != kFuseMaxVoxels / kFuseBlockVoxels || fuse_blocks(1) != 1 || fuse_blocks(0) != 0) fail("fuse_blocks", 0, 0);
    std::printf("checked %d layouts\n", checked);
    return 0;
}
