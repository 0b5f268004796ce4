// btba_objective_layout.hpp -- how btba_objective_batch_zn_aux cuts its work and lays out its scratch (btba_objective.hpp), once, for the
// kernels that index the partial records and for the host that sizes the buffer and the launches (btba_api_objective.hip).
// No HIP in here: tests/cpp/objective_host.cpp compiles it with g++ and walks the shapes.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define BTBA_OBJECTIVE_HD __host__ __device__
#else
#define BTBA_OBJECTIVE_HD
#endif

namespace btba {

constexpr int kObjectiveBlock = 256;               // lanes of a workgroup: four waves
constexpr int kObjectiveTilePixels = 1024;         // source pixels of a dense tile: four trips of a workgroup
constexpr int kObjectiveChunkEntries = 1024;       // correspondences of a sparse chunk: four trips (a multiple of the 64-entry groups of the 24-byte layout)
constexpr size_t kObjectiveRecordBytes = 40;       // one partial record = one btba_objective_pair (include/btba.h; asserted in btba_api_objective.hip)

// tiles of a dense pair: a function of the cache's pixel count alone
BTBA_OBJECTIVE_HD constexpr int objective_tiles(int npix) { return (npix + kObjectiveTilePixels - 1) / kObjectiveTilePixels; }
// chunks of a correspondence segment: a function of the call's longest segment alone.  Chunk c owns entries [c, c + 1) * kObjectiveChunkEntries of
// EVERY segment whatever that count is, and a chunk past a segment's end yields the empty record (+0.0 sums), so no sum depends on the count.
BTBA_OBJECTIVE_HD constexpr int objective_chunks(uint32_t max_corr_per_pair)
{
    return max_corr_per_pair == 0 ? 1 : (int)((max_corr_per_pair + (uint32_t)kObjectiveChunkEntries - 1) / (uint32_t)kObjectiveChunkEntries);
}
// pixels [lo, hi) of tile t; entries [lo, hi) of chunk c of a segment of len entries (relative to the segment's start)
BTBA_OBJECTIVE_HD constexpr int objective_tile_lo(int npix, int t) { return t * kObjectiveTilePixels < npix ? t * kObjectiveTilePixels : npix; }
BTBA_OBJECTIVE_HD constexpr int objective_tile_hi(int npix, int t) { return (t + 1) * kObjectiveTilePixels < npix ? (t + 1) * kObjectiveTilePixels : npix; }
BTBA_OBJECTIVE_HD constexpr uint32_t objective_chunk_lo(uint32_t len, int c)
{
    return (uint64_t)c * kObjectiveChunkEntries < len ? (uint32_t)c * (uint32_t)kObjectiveChunkEntries : len;
}
BTBA_OBJECTIVE_HD constexpr uint32_t objective_chunk_hi(uint32_t len, int c)
{
    return (uint64_t)(c + 1) * kObjectiveChunkEntries < len ? (uint32_t)(c + 1) * (uint32_t)kObjectiveChunkEntries : len;
}

// Offsets in BYTES into the call's scratch; every region starts on a 256-byte boundary.
//   T, Tinv   float [B][N][16]: k_prepare's matrices of the caller's poses
//   dense     record [B][Pd][tiles]   (empty when the call evaluates no dense term)
//   sparse    record [B][P][chunks]   (empty when it evaluates no sparse term)
struct ObjectiveLayout {
    int tiles, chunks;              // per dense pair, per correspondence segment
    size_t T, Tinv, dense, sparse;
    size_t total;                   // bytes the call asks the workspace for

    BTBA_OBJECTIVE_HD static constexpr size_t round256(size_t b) { return (b + 255) & ~(size_t)255; }
    // record index of (instance b, dense pair p, tile t) and of (instance b, segment p, chunk c)
    BTBA_OBJECTIVE_HD constexpr size_t dense_record(int Pd, int b, int p, int t) const { return ((size_t)b * (size_t)Pd + (size_t)p) * (size_t)tiles + (size_t)t; }
    BTBA_OBJECTIVE_HD constexpr size_t sparse_record(int P, int b, int p, int c) const { return ((size_t)b * (size_t)P + (size_t)p) * (size_t)chunks + (size_t)c; }

    // Pd, P: pairs the call evaluates (0: that term is absent)
    BTBA_OBJECTIVE_HD constexpr ObjectiveLayout(int B, int N, int npix, int Pd, int P, uint32_t max_corr_per_pair)
        : tiles(objective_tiles(npix)), chunks(objective_chunks(max_corr_per_pair)),
          T(0), Tinv(round256(4 * 16 * (size_t)B * (size_t)N)), dense(2 * round256(4 * 16 * (size_t)B * (size_t)N)),
          sparse(dense + round256(kObjectiveRecordBytes * (size_t)B * (size_t)Pd * (size_t)objective_tiles(npix))),
          total(sparse + round256(kObjectiveRecordBytes * (size_t)B * (size_t)P * (size_t)objective_chunks(max_corr_per_pair))) {}
};

}  // namespace btba
