// btba_register_layout.hpp -- point blocks, partial records and scratch layout of frame-to-model registration (btba_register_frames,
// include/btba.h).  No HIP: the kernels (btba_register.hpp) index the scratch with it, the host (btba_api_register.hip) sizes it with it, and
// tests/cpp/register_host.cpp walks it under the host sanitizers.
//
// An item's points are cut into blocks of kRegBlockPoints consecutive indices; block k of an item is summed by ONE workgroup into ONE partial
// record, whatever the batch looks like, so the summation tree of a point depends on its index within its segment alone.  Item i owns the
// partial records [part_off[i], part_off[i + 1]); an item without points owns none.  The scratch, every region a multiple of 256 bytes:
//   partials  double [blocks][kRegRecord]   slots 0 .. 20 H (lower triangle, row-major: (i, j) at i (i + 1) / 2 + j), 21 .. 26 g, 27 cost,
//                                           28 n_valid, 29 n_matched, 30 n_beyond (integers, exact in a double), 31 unused
//   poses     float  [n_items][12]          the current pose of every item
//   state     int32  [n_items][2]           (0 = running, 1 + status once stopped; iterations done)
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define BTBA_REGISTER_HD __host__ __device__
#else
#define BTBA_REGISTER_HD
#endif

namespace btba {

constexpr int kRegThreads = 256, kRegPointsPerThread = 8;
constexpr int kRegBlockPoints = kRegThreads * kRegPointsPerThread;      // 2048
constexpr int kRegRecord = 32;                                           // doubles per partial record: 256 bytes
constexpr int kRegSlotG = 21, kRegSlotCost = 27, kRegSlotValid = 28, kRegSlotMatched = 29, kRegSlotBeyond = 30;
constexpr int64_t kRegMaxBlocks = (int64_t)1 << 22;                      // partial records of one call: 1 GiB
constexpr int64_t kRegMaxPoints = (int64_t)1 << 30;                      // points of one item (the segment record's limit)

struct RegisterLayout {
    int64_t blocks = 0;                                                  // partial records of the call
    size_t partials = 0, poses = 0, state = 0, total = 0;                // byte offsets, each a multiple of 256
};

BTBA_REGISTER_HD inline int64_t register_blocks(int64_t n_points) { return (n_points + kRegBlockPoints - 1) / kRegBlockPoints; }

// n_points: [n_items].  part_off: [n_items + 1] or null.  false: a count outside 0 .. kRegMaxPoints, or more than kRegMaxBlocks records in all.
inline bool register_layout(int n_items, const int64_t *n_points, int64_t *part_off, RegisterLayout *L)
{
    int64_t nb = 0;
    for (int i = 0; i < n_items; i++) {
        if (n_points[i] < 0 || n_points[i] > kRegMaxPoints) return false;
        if (part_off) part_off[i] = nb;
        nb += register_blocks(n_points[i]);
        if (nb > kRegMaxBlocks) return false;
    }
    if (part_off) part_off[n_items < 0 ? 0 : n_items] = nb;
    if (L) {
        auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
        const size_t n = n_items < 0 ? 0 : (size_t)n_items;
        L->blocks = nb;
        L->partials = 0;
        L->poses = up(sizeof(double) * kRegRecord * (size_t)nb);
        L->state = L->poses + up(sizeof(float) * 12 * n);
        L->total = L->state + up(sizeof(int32_t) * 2 * n);
    }
    return true;
}

}  // namespace btba
