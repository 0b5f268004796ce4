// btba_marginals_layout.hpp -- the dynamic-LDS layout of k_pose_covariances (btba_marginals.hpp), once, for the kernel that carves its
// pointers out of it and for the host that sizes the launch (btba_api_marginals.hip: btba_pose_covariances).
// No HIP in here: tests/cpp/marginals_host.cpp compiles it with g++ and walks every window size.
#pragma once
#include <cstddef>

#if defined(__HIPCC__)
#define BTBA_MARGINALS_HD __host__ __device__
#else
#define BTBA_MARGINALS_HD
#endif

namespace btba {

constexpr int kMarginalsMaxFrames = 31;                              // = BTBA_MAX_FRAMES_LDS (include/btba.h; asserted in btba_api_marginals.hip)
constexpr int kMarginalsBlock = 256;                                 // lanes of a workgroup: one per unknown (na <= 180) while factorising, all of them for the products
constexpr size_t kMarginalsLdsLimit = 160 * 1024;                    // bytes of LDS of one compute unit

// unknowns of a window: frame 0 is fixed
BTBA_MARGINALS_HD constexpr int marginals_unknowns(int n_frames) { return 6 * (n_frames - 1); }
// entry (i, j), j <= i, of the packed lower triangle, row by row
BTBA_MARGINALS_HD constexpr size_t marginals_tri_index(int i, int j) { return (size_t)i * (size_t)(i + 1) / 2 + (size_t)j; }

// bytes of dynamic LDS of a window: the packed triangle, and four vectors of na doubles (= MarginalsLayout::total)
BTBA_MARGINALS_HD constexpr size_t marginals_lds_bytes(int n_frames)
{
    return 8 * ((size_t)marginals_unknowns(n_frames) * (size_t)(marginals_unknowns(n_frames) + 1) / 2 + 4 * (size_t)marginals_unknowns(n_frames));
}

// Offsets in BYTES from the start of the dynamic LDS; every region holds doubles and is 8-byte aligned.  The full square of a 31-frame
// window (180 x 180 x 8 = 259 200 bytes) does not fit a compute unit's LDS; its packed lower triangle (130 320 bytes) does.
struct MarginalsLayout {
    int na;                         // unknowns
    size_t tri;                     // double [na (na + 1) / 2]: H, then L, then L^-1, packed row by row
    size_t col;                     // double [2][na]: the column of L the inversion is about to overwrite, double-buffered
    size_t pivot;                   // double [na]: d_j, the pivot of unknown j before its square root
    size_t diag;                    // double [na]: H_jj as given
    size_t total;                   // bytes the launch asks for

    BTBA_MARGINALS_HD explicit MarginalsLayout(int n_frames)
    {
        na = marginals_unknowns(n_frames);
        const size_t n = (size_t)na;
        tri = 0;
        col = tri + 8 * (n * (n + 1) / 2);
        pivot = col + 8 * 2 * n;
        diag = pivot + 8 * n;
        total = diag + 8 * n;
    }
};

}  // namespace btba
