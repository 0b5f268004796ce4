// objective_host.cpp -- the work split and scratch layout of the objective report (bundletrack_amd/csrc/btba_objective_layout.hpp) on the CPU, for a
// sanitizer build (tests/test_objective_layout.py):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined tests/cpp/objective_host.cpp -o tests/cpp/objective_host
// For every shape: tiles and chunks cover every pixel / entry exactly once and never reach past the end (cache sizes 117 and 1500 are no multiples of
// the workgroup, segments of 0 and 1 entries), the scratch regions are disjoint, 256-byte aligned and inside the stated size, every partial record has
// a slot of its own inside its region.  The scratch is allocated for real and every record written, so an overrun is AddressSanitizer's to report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../bundletrack_amd/csrc/btba_objective_layout.hpp"

static void fail(const char *what, int a, int b)
{
    std::printf("FAIL %s (%d, %d)\n", what, a, b);
    std::exit(1);
}

int main()
{
    using namespace btba;
    const int npixs[] = { 4, 117, 256, 768, 1024, 1025, 1500, 2200, 4800, 19200 };
    const uint32_t lens[] = { 0u, 1u, 63u, 64u, 65u, 255u, 256u, 257u, 513u, 1000u, 1023u, 1024u, 1025u, 2000u, 5000u };
    int checked = 0;
    // tiles: a partition of [0, npix), each tile at most kObjectiveTilePixels
    for (int npix : npixs) {
        const int tiles = objective_tiles(npix);
        std::vector<unsigned char> seen((size_t)npix, 0);
        for (int t = 0; t < tiles; t++) {
            const int lo = objective_tile_lo(npix, t), hi = objective_tile_hi(npix, t);
            if (lo < 0 || hi > npix || lo >= hi || hi - lo > kObjectiveTilePixels) fail("tile range", npix, t);
            // the walk of the kernels: lane tid visits lo + tid, lo + tid + 256, ... below hi
            for (int tid = 0; tid < kObjectiveBlock; tid++)
                for (int s = lo + tid; s < hi; s += kObjectiveBlock) seen[(size_t)s]++;
        }
        for (int s = 0; s < npix; s++) if (seen[(size_t)s] != 1) fail("pixel visited once", npix, s);
    }
    // chunks: for every call-wide maximum at least as long as the segment, the chunks partition the segment; chunks past its end are empty
    for (uint32_t mx : lens)
        for (uint32_t len : lens) {
            if (len > mx) continue;
            const int chunks = objective_chunks(mx);
            if (chunks < 1) fail("at least one chunk", (int)mx, (int)len);
            std::vector<unsigned char> seen((size_t)len, 0);
            for (int c = 0; c < chunks; c++) {
                const uint32_t lo = objective_chunk_lo(len, c), hi = objective_chunk_hi(len, c);
                if (lo > hi || hi > len || hi - lo > (uint32_t)kObjectiveChunkEntries) fail("chunk range", (int)len, c);
                if (lo % 64 != 0 && lo != len) fail("chunk starts on a 64-entry group", (int)len, c);
                for (uint32_t tid = 0; tid < (uint32_t)kObjectiveBlock; tid++)
                    for (uint32_t e = lo + tid; e < hi; e += kObjectiveBlock) seen[e]++;
            }
            for (uint32_t e = 0; e < len; e++) if (seen[e] != 1) fail("entry visited once", (int)mx, (int)e);
        }
    // scratch
    for (int B : { 1, 3 })
        for (int N : { 2, 3, 5, 15 })
            for (int npix : { 117, 1500, 19200 })
                for (int with_dense : { 0, 1 })
                    for (uint32_t mx : { 0u, 1u, 1000u, 1025u }) {
                        const int P = N * (N - 1) / 2, Pd = with_dense ? P + 1 : 0, Ps = mx ? P : 0;
                        const ObjectiveLayout L(B, N, npix, Pd, Ps, mx);
                        const size_t mat = 4 * 16 * (size_t)B * N, drec = (size_t)B * Pd * L.tiles, srec = (size_t)B * Ps * L.chunks;
                        if (L.T % 256 || L.Tinv % 256 || L.dense % 256 || L.sparse % 256 || L.total % 256) fail("alignment", N, npix);
                        if (L.T + mat > L.Tinv || L.Tinv + mat > L.dense || L.dense + kObjectiveRecordBytes * drec > L.sparse || L.sparse + kObjectiveRecordBytes * srec > L.total)
                            fail("regions disjoint and inside the total", N, npix);
                        std::vector<unsigned char> scratch(L.total, 0);
                        for (size_t k = 0; k < mat; k++) { scratch[L.T + k]++; scratch[L.Tinv + k]++; }
                        for (int b = 0; b < B; b++) {
                            for (int p = 0; p < Pd; p++)
                                for (int t = 0; t < L.tiles; t++) {
                                    const size_t r = L.dense_record(Pd, b, p, t);
                                    if (r >= drec) fail("dense record index", p, t);
                                    for (size_t k = 0; k < kObjectiveRecordBytes; k++) scratch[L.dense + kObjectiveRecordBytes * r + k]++;
                                }
                            for (int p = 0; p < Ps; p++)
                                for (int c = 0; c < L.chunks; c++) {
                                    const size_t r = L.sparse_record(Ps, b, p, c);
                                    if (r >= srec) fail("sparse record index", p, c);
                                    for (size_t k = 0; k < kObjectiveRecordBytes; k++) scratch[L.sparse + kObjectiveRecordBytes * r + k]++;
                                }
                        }
                        for (size_t k = 0; k < L.total; k++) if (scratch[k] > 1) fail("a byte with two owners", N, (int)k);
                        checked++;
                    }
    std::printf("checked %d layouts\n", checked);
    return 0;
}
