// solve_layout_host.cpp -- the LDS layout of the general system solve (bundletrack_amd/csrc/btba_solve_layout.hpp) on the CPU, for a
// sanitizer build: every window size and pair-list size the solve accepts, against what the kernel and the host rely on.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined tests/cpp/solve_layout_host.cpp -o tests/cpp/solve_layout_host
// Prints one line per failed check and "checked <cases> layouts" at the end; exit status 0 only when every check held.
#include <cstddef>
#include <cstdio>

#include "../../bundletrack_amd/csrc/btba_solve_layout.hpp"

using btba::SolveLayout;

static int failures = 0;
static void fail(const char *what, int N, int Pd, bool a_in_global)
{
    std::printf("FAILED %s: N = %d, Pd = %d, a_in_global = %d\n", what, N, Pd, (int)a_in_global);
    failures++;
}

static size_t round4(size_t v) { return (v + 3) & ~(size_t)3; }

int main()
{
    long cases = 0;
    for (int N = 2; N <= 85; N++) {
        const int P = N * (N - 1) / 2, n = 6 * N;
        const int pds[4] = { 0, 1, P, 2 * P };
        for (int Pd : pds)
            for (int variant = 0; variant < 2; variant++) {
                const bool a_in_global = variant > 0;
                const SolveLayout L(N, Pd, a_in_global);
                cases++;
                const size_t ld = 4 * (size_t)(((n + 3) / 4) | 1);
                if ((size_t)L.ld != ld || L.ld != btba::solve_row_floats(N)) fail("ld", N, Pd, a_in_global);
                // the size of everything but the matrix, as the host used to write it out
                const size_t rest = 6 * ld + 16 + 16 * (size_t)N + 4 * (size_t)Pd + (size_t)N + 1 + (size_t)P + 288 + round4((size_t)P) + round4(6 * (size_t)N);
                if (L.rest_floats != rest) fail("rest_floats", N, Pd, a_in_global);
                const size_t a_floats = a_in_global ? 0 : (size_t)n * ld;
                if (L.total != a_floats + rest) fail("total", N, Pd, a_in_global);
                // the regions in address order, with their sizes: each starts exactly where the one before it ends -- no overlap, and no gap that would move the
                // footprint; the last ends inside the total
                struct Region { const char *name; size_t off, size; bool read16; } regions[] = {
                    { "A", (size_t)L.A, a_floats, true },                         // float4 rows (the one-wave mat-vec, the load of a pre-assembled matrix)
                    { "vb", (size_t)L.vb, ld, true }, { "vM", (size_t)L.vM, ld, true }, { "unused", (size_t)L.unused, ld, false },
                    { "vp", (size_t)L.vp, ld, true },                              // float4 / float2 chunks of p
                    { "vAp", (size_t)L.vAp, ld, true }, { "vd", (size_t)L.vd, ld, true },
                    { "scratch", (size_t)L.scratch, 16, true },
                    { "vT", (size_t)L.vT, 16 * (size_t)N, true },                  // load_mat4: four float4 per frame
                    { "dense_pairs", (size_t)L.dense_pairs, 2 * (size_t)Pd, false },
                    { "adj_off", (size_t)L.adj_off, (size_t)N + 1, false },
                    { "adj", (size_t)L.adj, 2 * (size_t)Pd, false },
                    { "pair_ij", (size_t)L.pair_ij, (size_t)P, false },
                    { "entry_lut", (size_t)L.entry_lut, 288, false },
                    { "cross", (size_t)L.cross, round4((size_t)P), false },
                    { "x", (size_t)L.x, round4(6 * (size_t)N), false },
                };
                size_t end = 0;
                for (const Region &r : regions) {
                    if (r.size == 0) continue;                                            // (not part of this variant)
                    if (r.off != end) fail(r.name, N, Pd, a_in_global);      // overlaps the region before it, or leaves a gap
                    if (r.read16 && r.off % 4 != 0) fail(r.name, N, Pd, a_in_global);      // not 16-byte aligned
                    end = r.off + r.size;
                }
                if (end > L.total) fail("end beyond total", N, Pd, a_in_global);
                if (L.ld % 8 != 4) fail("ld is not an odd multiple of 4", N, Pd, a_in_global);
                // the staged pair sums start at `total`: directly behind x
                if (L.total != (size_t)L.x + round4(6 * (size_t)N)) fail("pair sums do not follow x", N, Pd, a_in_global);
            }
    }
    std::printf("checked %ld layouts\n", cases);
    return failures ? 1 : 0;
}
