// register_host.cpp -- point blocks, partial records and the scratch layout of frame-to-model registration
// (bundletrack_amd/csrc/btba_register_layout.hpp) on the CPU, for a sanitizer build (tests/test_register_layout.py):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined tests/cpp/register_host.cpp -o tests/cpp/register_host
// For every set of items: the items' record ranges are disjoint, in order and inside the total; an item without points owns none; every point
// of an item lies in exactly one (block, thread, slot) of the accumulate kernel's walk; the regions are disjoint, 256-byte aligned and inside
// the stated size; the caps on points per item and on records per call hold.  The scratch is allocated for real and every byte a kernel would
// touch is written, so an overrun is AddressSanitizer's to report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../bundletrack_amd/csrc/btba_register_layout.hpp"

static void fail(const char *what, long long a, long long b)
{
    std::printf("FAIL %s (%lld, %lld)\n", what, a, b);
    std::exit(1);
}

int main()
{
    using namespace btba;
    int checked = 0;
    const std::vector<std::vector<int64_t>> cases = {
        { 1 },
        { 0 },
        { 35 },                                                                      // a 7 x 5 frame: less than a wave
        { 2048 },                                                                    // exactly one block
        { 2049 },                                                                    // one point into the second block
        { 48 * 64, 0, 65, 5000, 1, 480 * 640 },
        std::vector<int64_t>(33, 3072),                                              // more than one chunk of items
    };
    for (const auto &n : cases) {
        const int items = (int)n.size();
        std::vector<int64_t> po(items + 1, -1);
        RegisterLayout L;
        if (!register_layout(items, n.data(), po.data(), &L)) fail("a valid layout refused", items, 0);
        if (po[0] != 0 || po[items] != L.blocks) fail("totals", po[items], L.blocks);
        for (size_t off : { L.partials, L.poses, L.state, L.total })
            if (off % 256) fail("alignment", (long long)off, 0);
        std::vector<unsigned char> scratch(L.total, 0);
        auto touch = [&](size_t off, size_t bytes) {
            for (size_t k = 0; k < bytes; k++) scratch[off + k]++;      // past L.total: AddressSanitizer
        };
        for (int i = 0; i < items; i++) {
            const int64_t nb = po[i + 1] - po[i];
            if (nb != register_blocks(n[i]) || nb != (n[i] + kRegBlockPoints - 1) / kRegBlockPoints) fail("blocks of an item", i, nb);
            if (n[i] == 0 && nb != 0) fail("an empty item owns a record", i, nb);
            // the accumulate kernel's walk: block b, slot j, thread t takes element b * 2048 + j * 256 + t
            int64_t seen = 0, last = -1;
            for (int64_t b = 0; b < nb; b++) {
                for (int t = 0; t < kRegThreads; t++)
                    for (int j = 0; j < kRegPointsPerThread; j++) {
                        const int64_t e = b * kRegBlockPoints + (int64_t)j * kRegThreads + t;
                        if (e < n[i]) { seen++; if (e > last) last = e; }
                    }
                touch(L.partials + sizeof(double) * kRegRecord * (size_t)(po[i] + b), sizeof(double) * kRegRecord);
            }
            if (seen != n[i] || (n[i] > 0 && last != n[i] - 1)) fail("points walked by the blocks", i, seen);
            touch(L.poses + sizeof(float) * 12 * (size_t)i, sizeof(float) * 12);
            touch(L.state + sizeof(int32_t) * 2 * (size_t)i, sizeof(int32_t) * 2);
        }
        for (size_t k = 0; k < L.total; k++) if (scratch[k] > 1) fail("a byte with two owners", items, (long long)k);
        if (kRegSlotG != 21 || kRegSlotCost != 27 || kRegSlotBeyond >= kRegRecord || kRegBlockPoints != 2048) fail("record slots", 0, 0);
        checked++;
    }
    // refused: a negative count, more than 2^30 points in an item, more than 2^22 records in a call
    const std::vector<std::vector<int64_t>> refused = {
        { -1 },
        { 5, ((int64_t)1 << 30) + 1 },
        std::vector<int64_t>(9, (int64_t)1 << 30),                                   // 9 * 2^19 records
    };
    for (const auto &n : refused) {
        RegisterLayout L;
        if (register_layout((int)n.size(), n.data(), nullptr, &L)) fail("an invalid layout accepted", (long long)n.size(), n[0]);
        checked++;
    }
    // the cap itself, reached exactly by eight items of 2^30 points, is accepted (1 GiB of records: sized here, not allocated)
    {
        const std::vector<int64_t> n(8, (int64_t)1 << 30);
        std::vector<int64_t> po(9);
        RegisterLayout L;
        if (!register_layout(8, n.data(), po.data(), &L) || L.blocks != kRegMaxBlocks || po[1] != ((int64_t)1 << 19) || L.total < ((size_t)1 << 30))
            fail("the cap itself", L.blocks, (long long)L.total);
        checked++;
    }
    if (register_blocks(0) != 0 || register_blocks(1) != 1 || register_blocks(2048) != 1 || register_blocks(2049) != 2) fail("register_blocks", 0, 0);
    // no items: nothing but the (empty, aligned) regions
    {
        RegisterLayout L;
        int64_t po[1] = { -1 };
        if (!register_layout(0, nullptr, po, &L) || L.blocks != 0 || po[0] != 0 || L.total != 0) fail("no items", L.blocks, (long long)L.total);
        checked++;
    }
    std::printf("checked %d layouts\n", checked);
    return 0;
}
