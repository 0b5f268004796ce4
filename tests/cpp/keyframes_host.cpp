// keyframes_host.cpp -- the pool records and the select kernel's LDS layout of the device keyframe memory
// (bundletrack_amd/csrc/btba_keyframes_layout.hpp) on the CPU, for a sanitizer build (tests/test_keyframes_layout.py):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined tests/cpp/keyframes_host.cpp -o keyframes_host
// For every (sessions, capacity, max_BA): the pool's regions are disjoint, 256-byte aligned and inside the stated size; the LDS regions are
// disjoint, 16-byte aligned and inside the stated size, which is inside the LDS limit; sizes outside the limits are refused.  Both blocks are
// allocated for real and every byte a kernel would touch is written, so an overrun is AddressSanitizer's to report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../bundletrack_amd/csrc/btba_keyframes_layout.hpp"

static void fail(const char *what, long long a, long long b)
{
    std::printf("FAIL %s (%lld, %lld)\n", what, a, b);
    std::exit(1);
}

int main()
{
    using namespace btba;
    int checked = 0;
    struct Case { int S, C, B; };
    const std::vector<Case> cases = { { 1, 1, 2 }, { 4, 320, 6 }, { 32, 100, 15 }, { 3, 1000, 15 }, { 1, 1024, 32 }, { 2, 479, 85 }, { 1, 20000, 2 }, { 7, 33, 85 } };
    for (const Case &c : cases) {
        KeyframesPool P;
        KeyframesLds L;
        if (!keyframes_pool_layout(c.S, c.C, &P) || !keyframes_lds_layout(c.C, c.B, &L)) fail("a valid layout refused", c.C, c.B);
        for (size_t off : { P.poses, P.frame_id, P.frame_key, P.count, P.overflow, P.total })
            if (off % 256) fail("pool alignment", (long long)off, 0);
        for (size_t off : { L.table, L.member, L.order, L.red_cum, L.red_slot, L.pick, L.total })
            if (off % 16) fail("LDS alignment", (long long)off, 0);
        if (L.total > kKfLdsLimit) fail("LDS limit", (long long)L.total, (long long)kKfLdsLimit);
        std::vector<unsigned char> pool(P.total, 0), lds(L.total, 0);
        auto touch = [](std::vector<unsigned char> &m, size_t off, size_t bytes) {
            for (size_t k = 0; k < bytes; k++) m[off + k]++;            // past the end: AddressSanitizer
        };
        for (int s = 0; s < c.S; s++) {
            for (int k = 0; k < c.C; k++) {
                const size_t slot = (size_t)s * c.C + k;
                touch(pool, P.poses + sizeof(float) * 16 * slot, sizeof(float) * 16);
                touch(pool, P.frame_id + sizeof(int32_t) * slot, sizeof(int32_t));
                touch(pool, P.frame_key + sizeof(uint64_t) * slot, sizeof(uint64_t));
            }
            touch(pool, P.count + sizeof(int32_t) * s, sizeof(int32_t));
            touch(pool, P.overflow + sizeof(int32_t) * s, sizeof(int32_t));
        }
        for (size_t k = 0; k < P.total; k++) if (pool[k] > 1) fail("a pool byte with two owners", c.S, (long long)k);
        for (int j = 0; j < c.B; j++) {
            for (int k = 0; k < c.C; k++) touch(lds, L.table + sizeof(float) * ((size_t)j * c.C + k), sizeof(float));      // the kernel's index: column j at j * C
            touch(lds, L.member + sizeof(int32_t) * j, sizeof(int32_t));
            touch(lds, L.order + sizeof(int32_t) * j, sizeof(int32_t));
        }
        for (int w = 0; w < kKfSelectWaves; w++) {
            touch(lds, L.red_cum + sizeof(float) * w, sizeof(float));
            touch(lds, L.red_slot + sizeof(int32_t) * w, sizeof(int32_t));
        }
        touch(lds, L.pick, sizeof(int32_t));
        for (size_t k = 0; k < L.total; k++) if (lds[k] > 1) fail("an LDS byte with two owners", c.C, (long long)k);
        checked++;
    }
    // refused: max_BA outside 2 .. 85, no capacity, no session, a table past the LDS limit, more than 2^24 slots
    const std::vector<Case> refused = { { 1, 10, 1 }, { 1, 10, 86 }, { 1, 0, 6 }, { 0, 10, 6 }, { 1, 1024, 40 }, { 1, 1281, 32 }, { 1, 482, 85 }, { 1 << 13, (1 << 11) + 1, 2 } };
    for (const Case &c : refused) {
        if (keyframes_pool_layout(c.S, c.C, nullptr) && keyframes_lds_layout(c.C, c.B, nullptr)) fail("an invalid layout accepted", c.C, c.B);
        checked++;
    }
    // about 1024 keyframes at max_BA_frames <= 32
    if (!keyframes_lds_layout(1024, 32, nullptr) || !keyframes_lds_layout(1270, 32, nullptr)) fail("the stated reach", 1024, 32);
    if (kKfSelectThreads != 256 || kKfSelectWaves != 4 || kKfMinBA != 2 || kKfMaxBA != 85) fail("constants", 0, 0);
    std::printf("checked %d layouts\n", checked);
    return 0;
}
