// btba_sweep_layout.hpp -- the dynamic-LDS layout of a dense sweep item on the compact cache (btba_kernels.hpp: dense_block_zn, dense_block_pinhole),
// once, for the kernel that carves its pointers out of it and for the host that sizes the launch (btba_api.hip: solve_enqueue).
// No HIP in here (a constexpr constructor is callable on both sides): tests/cpp/sweep_layout_host.cpp compiles it with g++ and walks every cache size.
#pragma once
#include <cstddef>

namespace btba {

constexpr int kMaxBandBlocks = 1024;      // blocks of one band of the block walk: above it solve_enqueue falls back to row strips (the band's index arithmetic in pinhole_live_blocks relies on it)

// kinds of item: dense_block_zn (general K: the coordinate table only); dense_block_pinhole<0> / <1> (row strips, valid-pixel lists: + the rotated-ray
// tables); dense_block_pinhole<2> (8 x 8 block walk: + hull entries, wave totals and the list of live blocks)
enum SweepLdsKind { kSweepLdsGeneralK = 0, kSweepLdsStrips = 1, kSweepLdsBlocks = 2 };

// Offsets in BYTES from the start of the dynamic LDS of a cache of Wd x Hd pixels; band_blocks = blocks of one band of block rows (the largest one).
//   lut    (Wd + Hd) floats, padded to 16 bytes: the back-projection term of every cache column, then of every cache row
//   colA   Wd float4, rowB  Hd float4: the rotated rays (pinhole_fill_tables; rowB directly behind colA: the kernel addresses both through colA)
//   hull   8 floats per block column and block row: the entries of the dead-block test (btba_hull.hpp; five used)
//   hdr    8 ints: the wave totals of the list compaction
//   blist  band_blocks codes: the live blocks
// A region a kind does not use is empty.
struct SweepLayout {
    bool block_walk;                // kSweepLdsBlocks with a band the walk can index; false for a larger band: "no block walk", the layout is the strips'
    size_t lut, colA, rowB, hull, hdr, blist;
    size_t total;                   // bytes the launch asks for (the host adds its debug pad on top)

    constexpr SweepLayout(int Wd, int Hd, int band_blocks, int kind)
        : block_walk(kind == kSweepLdsBlocks && band_blocks <= kMaxBandBlocks), lut(0), colA(4 * (size_t)((Wd + Hd + 3) & ~3)),
          rowB(colA + (kind == kSweepLdsGeneralK ? 0 : 16 * (size_t)Wd)), hull(rowB + (kind == kSweepLdsGeneralK ? 0 : 16 * (size_t)Hd)),
          hdr(hull + (block_walk ? 32 * (size_t)((Wd >> 3) + (Hd >> 3)) : 0)), blist(hdr + (block_walk ? 32 : 0)),
          total(blist + (block_walk ? 4 * (size_t)band_blocks : 0)) {}
};

}  // namespace btba
