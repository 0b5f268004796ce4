// marginals_host.cpp -- the LDS layout of k_pose_covariances (bundletrack_amd/csrc/btba_marginals_layout.hpp) on the CPU, for a sanitizer
// build: every window size the kernel serves, against what the kernel and the host rely on.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined tests/cpp/marginals_host.cpp -o tests/cpp/marginals_host
// Prints one line per failed check and "checked <cases> layouts" at the end; exit status 0 only when every check held.
#include <cstddef>
#include <cstdio>
#include <vector>

#include "../../bundletrack_amd/csrc/btba_marginals_layout.hpp"

using btba::MarginalsLayout;

static int failures = 0;
static void fail(const char *what, int N)
{
    std::printf("FAILED %s: N = %d\n", what, N);
    failures++;
}

int main()
{
    long cases = 0;
    for (int N = 2; N <= btba::kMarginalsMaxFrames; N++) {
        const MarginalsLayout L(N);
        cases++;
        const size_t na = 6 * (size_t)(N - 1);
        if ((size_t)L.na != na || btba::marginals_unknowns(N) != (int)na) fail("na", N);
        if (na > (size_t)btba::kMarginalsBlock) fail("more unknowns than lanes", N);
        // the regions in address order, with their sizes in bytes: each starts where the one before it ends, on an 8-byte boundary
        struct Region { const char *name; size_t off, size; } regions[] = {
            { "tri", L.tri, 8 * (na * (na + 1) / 2) }, { "col", L.col, 8 * 2 * na }, { "pivot", L.pivot, 8 * na }, { "diag", L.diag, 8 * na },
        };
        size_t end = 0;
        for (const Region &r : regions) {
            if (r.off != end) fail(r.name, N);                                  // overlaps the region before it, or leaves a gap
            if (r.off % 8 != 0) fail(r.name, N);
            end = r.off + r.size;
        }
        if (end != L.total) fail("total", N);
        if (L.total != btba::marginals_lds_bytes(N)) fail("marginals_lds_bytes", N);
        if (L.total > btba::kMarginalsLdsLimit) fail("beyond the LDS of a compute unit", N);
        // the packed triangle: every (i, j), j <= i, has a slot of its own inside the region, rows back to back
        std::vector<unsigned char> seen(na * (na + 1) / 2, 0);
        for (size_t i = 0; i < na; i++)
            for (size_t j = 0; j <= i; j++) {
                const size_t e = btba::marginals_tri_index((int)i, (int)j);
                if (e >= seen.size() || seen[e]) { fail("tri_index", N); i = na; break; }
                seen[e] = 1;
            }
        // what makes column accesses of the lanes' own rows conflict-free: the row starts of any aligned run of 32 lanes fall into 32 different
        // 8-byte bank pairs (i (i + 1) / 2 modulo 32 is a permutation there)
        for (size_t i0 = 0; i0 + 32 <= ((na + 31) & ~(size_t)31); i0 += 32) {
            unsigned hit = 0;
            for (size_t i = i0; i < i0 + 32; i++) hit |= 1u << (btba::marginals_tri_index((int)i, 0) % 32);
            if (hit != 0xFFFFFFFFu) fail("row starts share a bank pair", N);
        }
    }
    if (btba::marginals_lds_bytes(31) != 130320 + 8 * 4 * 180) fail("31 frames: 130 320 bytes of triangle + vectors", 31);
    if (!(8 * (size_t)180 * 180 > btba::kMarginalsLdsLimit)) fail("the full square of 31 frames was expected not to fit", 31);
    std::printf("checked %ld layouts\n", cases);
    return failures ? 1 : 0;
}
