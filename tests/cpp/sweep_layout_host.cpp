// sweep_layout_host.cpp -- the dynamic-LDS layout of a dense sweep item (bundletrack_amd/csrc/btba_sweep_layout.hpp) on the CPU, for a
// sanitizer build: every cache the block walk accepts, against what the kernels and the host rely on.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined tests/cpp/sweep_layout_host.cpp -o tests/cpp/sweep_layout_host
// Prints one line per failed check and "checked <cases> layouts" at the end; exit status 0 only when every check held.
#include <cstddef>
#include <cstdio>

#include "../../bundletrack_amd/csrc/btba_sweep_layout.hpp"

using btba::SweepLayout;

static int failures = 0;
static void fail(const char *what, int Wd, int Hd, int tiles, int kind)
{
    std::printf("FAILED %s: Wd = %d, Hd = %d, tiles = %d, kind = %d\n", what, Wd, Hd, tiles, kind);
    failures++;
}

int main()
{
    long cases = 0;
    const int tile_counts[4] = { 1, 2, 3, 7 };
    const int kinds[3] = { btba::kSweepLdsGeneralK, btba::kSweepLdsStrips, btba::kSweepLdsBlocks };
    for (int Wd = 8; Wd <= 1016; Wd += 8)
        for (int Hd = 8; Wd + Hd <= 1024; Hd += 8)
            for (int tiles : tile_counts)
                for (int kind : kinds) {
                    const int bw = Wd / 8, bh = Hd / 8;
                    const size_t band_blocks = (size_t)((bh + tiles - 1) / tiles) * bw;
                    const SweepLayout L(Wd, Hd, (int)band_blocks, kind);
                    cases++;
                    const bool walk = kind == btba::kSweepLdsBlocks && band_blocks <= (size_t)btba::kMaxBandBlocks;
                    if (L.block_walk != walk) fail("block_walk", Wd, Hd, tiles, kind);      // a band beyond kMaxBandBlocks: no block walk
                    // the size as the host used to write it out: 4 ((Wd + Hd + 3) & ~3) + 16 (Wd + Hd) + 32 (bw + bh) + 32 + 4 band_blocks, each term only
                    // where the item has the region (a refused block walk is sized as the row strips it falls back to)
                    const size_t lut = 4 * (size_t)((Wd + Hd + 3) & ~3);
                    const size_t rays = kind == btba::kSweepLdsGeneralK ? 0 : 16 * (size_t)(Wd + Hd);
                    const size_t list = walk ? 32 * (size_t)(bw + bh) + 32 + 4 * band_blocks : 0;
                    if (L.total != lut + rays + list) fail("total", Wd, Hd, tiles, kind);
                    // the regions in address order, with their sizes: each starts exactly where the one before it ends, the last ends at the total
                    struct Region { const char *name; size_t off, size; bool read16; } regions[] = {
                        { "lut", L.lut, lut, false },
                        { "colA", L.colA, kind == btba::kSweepLdsGeneralK ? 0 : 16 * (size_t)Wd, true },      // float4 entries
                        { "rowB", L.rowB, kind == btba::kSweepLdsGeneralK ? 0 : 16 * (size_t)Hd, true },      // ... addressed through colA: directly behind it
                        { "hull", L.hull, walk ? 32 * (size_t)(bw + bh) : 0, true },                          // one float4 + one float per entry
                        { "hdr", L.hdr, walk ? 32 : 0, false },
                        { "blist", L.blist, walk ? 4 * band_blocks : 0, false },
                    };
                    size_t end = 0;
                    for (const Region &r : regions) {
                        if (r.off != end) fail(r.name, Wd, Hd, tiles, kind);                      // overlaps the region before it, or leaves a gap (an empty region sits where the next one starts)
                        if (r.read16 && r.size && r.off % 16 != 0) fail(r.name, Wd, Hd, tiles, kind);      // not 16-byte aligned
                        end = r.off + r.size;
                    }
                    if (end != L.total) fail("end is not the total", Wd, Hd, tiles, kind);
                    if (L.lut != 0) fail("lut does not start the LDS", Wd, Hd, tiles, kind);
                }
    // the band the block walk indexes: 1024 blocks are walked, 1025 are not
    if (!SweepLayout(256, 256, btba::kMaxBandBlocks, btba::kSweepLdsBlocks).block_walk) fail("1024 blocks refused", 256, 256, 1, btba::kSweepLdsBlocks);
    if (SweepLayout(256, 256, btba::kMaxBandBlocks + 1, btba::kSweepLdsBlocks).block_walk) fail("1025 blocks admitted", 256, 256, 1, btba::kSweepLdsBlocks);
    std::printf("checked %ld layouts\n", cases);
    return failures ? 1 : 0;
}
