// btba_solve_layout.hpp -- the dynamic-LDS layout of the general system solve (btba_solve_general.hpp: system_solve_body), once, for the
// kernel that carves its pointers out of it and for the host that sizes the launch (btba_api.hip: solve_enqueue).
// No HIP in here: tests/cpp/solve_layout_host.cpp compiles it with g++ and walks every window size.
#pragma once
#include <cstddef>

#if defined(__HIPCC__)
#define BTBA_LAYOUT_HD __host__ __device__
#else
#define BTBA_LAYOUT_HD
#endif

namespace btba {

constexpr int kLayoutSparseVals = 44;      // = kSparseVals (btba_kernels.hpp; asserted in btba_solve_general.hpp)

// row length of A and stride of the vectors: an odd multiple of 4 floats -- 16-byte rows, conflict-free ds_read_b128
BTBA_LAYOUT_HD constexpr int solve_row_floats(int n_frames) { return 4 * (((6 * n_frames + 3) / 4) | 1); }

// Offsets in floats from the start of the dynamic LDS (the int tables count one float per int).
//   a_in_global: the matrix lives in a global scratch (windows beyond BTBA_MAX_FRAMES_LDS frames), not in front of the vectors
// The reduced pair sums, when the host stages them in LDS (SolveDims::pairsum_in_lds), start at `total` and are sized by the host.
struct SolveLayout {
    int ld;                         // solve_row_floats(N)
    int A;                          // A[n][ld] (nothing when a_in_global; its pad columns n..ld-1 stay 0)
    int vb, vM, unused, vp, vAp, vd;      // ld floats each, 16-B aligned, zero padded: rhs / residual r, M^-1, (padding nobody touches: it keeps the footprint, and with it occupancy, where it was), p, A p, delta
    int scratch;                    // 16 floats: the workgroup sums' wave totals
    int vT;                         // this iterate's T[N][16]
    int dense_pairs;                // ints: (target, source) of every dense pair, 2 Pd
    int adj_off, adj;               // ints: the dense adjacency, N + 1 offsets and 2 Pd entries
    int pair_ij;                    // ints: canonical pair p -> (i << 8 | j), P
    // ints, 72 x 4: every entry of a sparse 6x6 block is  c1 rec[i1 + e es] + c2 rec[i2 + e es]  of the pair's 44 moment sums (e = which
    // end of the pair): 36 descriptors for diagonal blocks + 36 for cross blocks, so the assembly loops are branch-free
    int entry_lut;
    int cross;                      // ints: canonical pair -> the dense pair whose cross block it carries (or -1): P, padded to 16 bytes
    int x;                          // this iterate's x (phase D would otherwise start with a fabric-latency load): 6 N floats, padded to 16 bytes
    size_t rest_floats;             // everything but A
    size_t total;                   // floats the launch asks for (without the staged pair sums)

    BTBA_LAYOUT_HD SolveLayout(int N, int Pd, bool a_in_global)
    {
        const int n = 6 * N, P = N * (N - 1) / 2;
        ld = solve_row_floats(N);
        A = 0;
        vb = a_in_global ? 0 : n * ld;
        vM = vb + ld; unused = vM + ld; vp = unused + ld; vAp = vp + ld; vd = vAp + ld;
        scratch = vd + ld;
        vT = scratch + 16;
        dense_pairs = vT + 16 * N;
        adj_off = dense_pairs + 2 * Pd; adj = adj_off + (N + 1);
        pair_ij = adj + 2 * Pd;
        entry_lut = pair_ij + P;
        cross = entry_lut + 288;
        x = cross + ((P + 3) & ~3);
        const int end = x + ((n + 3) & ~3);
        rest_floats = (size_t)(end - vb);
        total = (size_t)end;
    }
};

}  // namespace btba
