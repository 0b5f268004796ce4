// btba_mask.hpp -- foreground-mask segmentation (btba_apply_masks, include/btba.h)
//   Frame::segmentationByMaskFile   src/Frame.cpp:236-317  (NOCS: largest 8-connected component -> convex hull -> fill; 5 x 5 dilate)
//   Frame::invalidatePixelsByMask   src/Frame.cpp:339-373  (zero colour / depth / normals outside the mask, the mask's ROI)
// The reference does this on the host with OpenCV and uploads the three maps again.  Here, per chunk of up to kMaskChunk frames
// (their pointers travel as kernel arguments, so an asynchronous call keeps no host memory alive):
//   plain path (YCBInEOAT):  k_mask_apply<false>   one launch: mask tile + halo in LDS, separable max, zero stores, ROI
//   hull path (NOCS):        k_mask_label_local    union-find per 16 x 16 tile in LDS, roots at the minimum linear index
//                            k_mask_label_merge    unions across tile borders: device-scope atomicMin on the global forest
//                            k_mask_label_count    flatten + component sizes per tile in an LDS hash, one add per (tile, root)
//                            k_mask_argmax         max over (count << 32) | ~root: largest, ties to the first in raster order
//                            k_mask_rows           one wave per row: the winner's leftmost and rightmost pixel
//                            k_mask_hull           one workgroup per frame: the two halves of the monotone chain over those
//                                                  <= 2H points on two waves (int64 cross products), then every row's
//                                                  [lo, hi] span of the closed hull
//                            k_mask_apply<true>    as the plain path, with M0 read from the spans
// Kernel boundaries give every cross-workgroup step its visibility: there is no spin-wait anywhere.  All of it is integer
// logic: the outputs equal a CPU restatement exactly (tests/mask_ref.py).
#pragma once
#include <hip/hip_runtime.h>
#include <climits>
#include <cstdint>

namespace btba {

constexpr int kMaskChunk = 32;                 // frames per launch
constexpr int kMaskTileW = 64, kMaskTileH = 16;   // apply: 64 x 4 threads, four rows each
constexpr int kMaskMaxR = 7;                   // dilate <= 15
constexpr int kLabelTile = 16;                 // labelling: 16 x 16 pixels, one per thread
constexpr int kHullLdsMaxH = 1536;             // k_mask_hull keeps rows and stack in LDS (40 H + 16 bytes) up to this height

struct MaskFrames {
    const uint8_t *mask[kMaskChunk];
    float *depth[kMaskChunk];
    float4 *normal[kMaskChunk];
    uchar4 *color[kMaskChunk];                 // entries may be null
    uint8_t *mask_out[kMaskChunk];             // entries may be null
};

template <class T> __device__ __forceinline__ T ld_relaxed(T *p, int scope)
{
    return scope == 0 ? __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
                      : __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// union-find on a forest whose parents never exceed their child (roots: the minimum index of the component).  The other
// threads of the same launch move parents concurrently, only ever downwards, so every load is an atomic one.
__device__ __forceinline__ int uf_find(int *P, int x, int scope)
{
    int p = ld_relaxed(P + x, scope);
    while (p != x) { x = p; p = ld_relaxed(P + x, scope); }
    return x;
}
__device__ __forceinline__ void uf_union(int *P, int a, int b, int scope)
{
    for (;;) {
        a = uf_find(P, a, scope);
        b = uf_find(P, b, scope);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }              // hang the larger root a under b
        const int old = atomicMin(P + a, b);
        if (old == a) return;
        a = old;                                                   // a was re-parented meanwhile: retry from there
    }
}

// grid (ceil(W / 16), ceil(H / 16), frames), 16 x 16.  labels: root's linear index (-1 off the mask); counts zeroed; best zeroed.
__global__ void __launch_bounds__(256) k_mask_label_local(int W, int H, const MaskFrames F, int *__restrict__ labels, int *__restrict__ counts,
                                                          unsigned long long *__restrict__ best)
{
    __shared__ int P[kLabelTile * kLabelTile];
    const int z = blockIdx.z, tx = threadIdx.x, ty = threadIdx.y, li = ty * kLabelTile + tx;
    const int x0 = blockIdx.x * kLabelTile, y0 = blockIdx.y * kLabelTile, x = x0 + tx, y = y0 + ty;
    const bool in = x < W && y < H;
    const size_t HW = (size_t)W * H, idx = (size_t)y * W + x;
    const bool fg = in && F.mask[z][idx] != 0;
    P[li] = fg ? li : -1;
    if (blockIdx.x == 0 && blockIdx.y == 0 && li == 0) best[z] = 0;
    __syncthreads();
    if (fg) {                                                      // backward neighbours inside the tile: W, NW, N, NE
        if (tx > 0 && ld_relaxed(P + li - 1, 0) >= 0) uf_union(P, li, li - 1, 0);
        if (ty > 0) {
            if (tx > 0 && ld_relaxed(P + li - kLabelTile - 1, 0) >= 0) uf_union(P, li, li - kLabelTile - 1, 0);
            if (ld_relaxed(P + li - kLabelTile, 0) >= 0) uf_union(P, li, li - kLabelTile, 0);
            if (tx < kLabelTile - 1 && ld_relaxed(P + li - kLabelTile + 1, 0) >= 0) uf_union(P, li, li - kLabelTile + 1, 0);
        }
    }
    __syncthreads();
    if (!in) return;
    int lab = -1;
    if (fg) {                                                      // local raster order is global raster order within a tile
        const int r = uf_find(P, li, 0);
        lab = (y0 + r / kLabelTile) * W + x0 + r % kLabelTile;
    }
    labels[z * HW + idx] = lab;
    counts[z * HW + idx] = 0;
}

// same grid: every union between a pixel and a backward neighbour (W, NW, N, NE) in another tile
__global__ void __launch_bounds__(256) k_mask_label_merge(int W, int H, int *__restrict__ labels)
{
    const int z = blockIdx.z, tx = threadIdx.x, ty = threadIdx.y;
    const int x = blockIdx.x * kLabelTile + tx, y = blockIdx.y * kLabelTile + ty;
    if (x >= W || y >= H || (tx != 0 && ty != 0 && tx != kLabelTile - 1)) return;
    int *L = labels + (size_t)z * W * H;
    const int i = y * W + x;
    if (L[i] < 0) return;
    if (tx == 0 && x > 0 && L[i - 1] >= 0) uf_union(L, i, i - 1, 1);
    if (y > 0) {
        if ((tx == 0 || ty == 0) && x > 0 && L[i - W - 1] >= 0) uf_union(L, i, i - W - 1, 1);
        if (ty == 0 && L[i - W] >= 0) uf_union(L, i, i - W, 1);
        if ((ty == 0 || tx == kLabelTile - 1) && x + 1 < W && L[i - W + 1] >= 0) uf_union(L, i, i - W + 1, 1);
    }
}

// same grid: labels := root; sizes summed per tile by root in an LDS hash (<= 256 keys in 256 slots), one global add per root
__global__ void __launch_bounds__(256) k_mask_label_count(int W, int H, int *__restrict__ labels, int *__restrict__ counts)
{
    __shared__ int key[256], cnt[256];
    const int z = blockIdx.z, tx = threadIdx.x, ty = threadIdx.y, li = ty * kLabelTile + tx;
    const int x = blockIdx.x * kLabelTile + tx, y = blockIdx.y * kLabelTile + ty;
    const size_t HW = (size_t)W * H;
    key[li] = -1;
    cnt[li] = 0;
    __syncthreads();
    if (x < W && y < H) {
        int *L = labels + z * HW;
        const int i = y * W + x;
        if (L[i] >= 0) {
            const int r = uf_find(L, i, 1);
            __hip_atomic_store(L + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // others may walk through i: r is still an ancestor
            unsigned h = ((unsigned)r * 2654435761u) >> 24;
            for (;;) {
                const int old = atomicCAS(key + h, -1, r);
                if (old == -1 || old == r) { atomicAdd(cnt + h, 1); break; }
                h = (h + 1) & 255;
            }
        }
    }
    __syncthreads();
    if (key[li] >= 0) atomicAdd(counts + z * HW + key[li], cnt[li]);
}

// grid (ceil(HW / 256), frames): best[z] = max over roots of (count << 32) | ~root
__global__ void __launch_bounds__(256) k_mask_argmax(int HW, const int *__restrict__ counts, unsigned long long *__restrict__ best)
{
    __shared__ unsigned long long part[4];
    const int z = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    unsigned long long k = 0;
    if (i < HW) {
        const int c = counts[(size_t)z * HW + i];
        if (c > 0) k = ((unsigned long long)c << 32) | (unsigned)~(unsigned)i;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const unsigned long long t = __shfl_xor(k, o, 64); k = t > k ? t : k; }
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = k;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; w++) k = part[w] > k ? part[w] : k;
        if (k) atomicMax(best + z, k);
    }
}

// grid (ceil(H / 4), frames), 256: one wave per row; rows[z H + y] = (leftmost, rightmost) x of the winner, (INT_MAX, -1) if none
__global__ void __launch_bounds__(256) k_mask_rows(int W, int H, const int *__restrict__ labels, const unsigned long long *__restrict__ best, int2 *__restrict__ rows)
{
    const int z = blockIdx.y, y = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (y >= H) return;
    const unsigned long long b = best[z];
    int lo = INT_MAX, hi = -1;
    if (b >> 32) {
        const int R = (int)~(unsigned)b;
        const int *L = labels + (size_t)z * W * H + (size_t)y * W;
        for (int x = lane; x < W; x += 64)
            if (L[x] == R) { lo = min(lo, x); hi = max(hi, x); }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { lo = min(lo, __shfl_xor(lo, o, 64)); hi = max(hi, __shfl_xor(hi, o, 64)); }
    if (lane == 0) rows[(size_t)z * H + y] = make_int2(lo, hi);
}

__device__ __forceinline__ long long floor_div(long long a, long long b)      // b > 0
{
    return a >= 0 ? a / b : -((-a + b - 1) / b);
}

// cross product in (u, v) = (y, x): Andrew's chain over points sorted by (y, x) is counter-clockwise in (u, v)
__device__ __forceinline__ long long cross_uv(int2 o, int2 a, int2 b)
{
    return (long long)(a.y - o.y) * (b.x - o.x) - (long long)(a.x - o.x) * (b.y - o.y);
}

// One half of Andrew's monotone chain over the points in (y, x) order -- each row's leftmost, then its rightmost when different (the
// hull of the component is the hull of these) -- forwards (the lower chain in (u, v)) or backwards (the upper chain), on the stack S.
// The top two entries stay in registers: a thread walking the chain alone waits on LDS only for the row it reads and for pops.
__device__ __forceinline__ int hull_chain(const int2 *rw, int H, bool fwd, int2 *S)
{
    int k = 0;
    int2 a = make_int2(0, 0), b = make_int2(0, 0);                  // S[k - 2], S[k - 1]
    for (int i = 0; i < H; i++) {
        const int y = fwd ? i : H - 1 - i;
        const int2 r = rw[y];
        if (r.y < 0) continue;
        const int ns = r.x != r.y ? 2 : 1;
        for (int s = 0; s < ns; s++) {
            const int2 p = make_int2((s == 0) == fwd ? r.x : r.y, y);
            while (k >= 2 && cross_uv(a, b, p) <= 0) {
                k--;
                b = a;
                if (k >= 2) a = S[k - 2];
            }
            S[k++] = p;
            a = b;
            b = p;
        }
    }
    return k;
}

// grid (frames), 256; dynamic LDS 40 H + 16 bytes when H <= kHullLdsMaxH, else none (rows and stacks stay in global scratch).
// spans[z H + y] = (lo, hi): the lattice points of row y inside the closed hull (empty when lo > hi).
__global__ void __launch_bounds__(256) k_mask_hull(int W, int H, const int2 *__restrict__ rows_g, int2 *__restrict__ stack_g, int2 *__restrict__ spans)
{
    extern __shared__ int2 sm[];
    __shared__ int n_chain[2], bb[4];
    const int z = blockIdx.x, tid = threadIdx.x;
    const bool lds = H <= kHullLdsMaxH;
    const int2 *rw = rows_g + (size_t)z * H;
    int2 *stk = stack_g + (size_t)z * (4 * (size_t)H + 2);
    if (lds) {
        for (int y = tid; y < H; y += 256) sm[y] = rw[y];
        rw = sm;
        stk = sm + H;
        __syncthreads();
    }
    int2 *lower = stk, *upper = stk + 2 * (size_t)H + 1;              // <= 2H points each
    if (tid == 0) n_chain[0] = hull_chain(rw, H, true, lower);          // the two chains on two waves, at the same time
    if (tid == 64) n_chain[1] = hull_chain(rw, H, false, upper);
    __syncthreads();
    // the hull counter-clockwise in (u, v): lower[0 .. kl - 2], upper[0 .. ku - 2]; a single point is lower[0]
    const int kl = n_chain[0], ku = n_chain[1];
    const int nl = kl > 1 ? kl - 1 : kl, hn = kl > 1 ? nl + ku - 1 : kl;
    auto vert = [&](int e) { return e < nl ? lower[e] : upper[e - nl]; };
    if (tid == 0) {
        int xmin = INT_MAX, xmax = -1, ymin = INT_MAX, ymax = -1;
        for (int e = 0; e < hn; e++) {
            const int2 v = vert(e);
            xmin = min(xmin, v.x); xmax = max(xmax, v.x);
            ymin = min(ymin, v.y); ymax = max(ymax, v.y);
        }
        bb[0] = xmin; bb[1] = xmax; bb[2] = ymin; bb[3] = ymax;
    }
    __syncthreads();
    for (int y = tid; y < H; y += 256) {
        long long lo = bb[0], hi = bb[1];
        if (hn == 0 || y < bb[2] || y > bb[3]) { lo = 1; hi = 0; }
        // every edge a -> b keeps the points p with cross_uv(a, b, p) = du (x - ax) - dv (y - ay) >= 0
        for (int e = 0; e < hn && lo <= hi; e++) {
            const int2 a = vert(e), b = vert(e + 1 < hn ? e + 1 : 0);
            const long long du = b.y - a.y, dv = b.x - a.x, c = dv * (long long)(y - a.y);
            if (du > 0) lo = max(lo, a.x - floor_div(-c, du));              // x - ax >= ceil(c / du)
            else if (du < 0) hi = min(hi, a.x + floor_div(-c, -du));       // x - ax <= floor(c / du)
            else if (c > 0) { lo = 1; hi = 0; }
        }
        spans[(size_t)z * H + y] = lo <= hi ? make_int2((int)lo, (int)hi) : make_int2(1, 0);
    }
}

// grid (ceil(W / 64), ceil(H / 16), frames), 64 x 4.  M0 from the mask bytes (plain) or the spans (hull); M = OR of M0 over the
// (2r + 1)^2 square; mask_out = M; depth, normal, colour := 0 where M = 0 (nothing is read from them); roi (when not null,
// frame f at roi + 4 (base + z), zero-initialised) collects max(9999 - x), max x, max(9999 - y), max y over M = 1, which
// decodes to the reference's (min(9999, umin), max(0, umax), ...) from a zero start.
template <bool HULL>
__global__ void __launch_bounds__(256) k_mask_apply(int W, int H, int r, const MaskFrames F, const int2 *__restrict__ spans, int *__restrict__ roi, int base)
{
    constexpr int LWM = kMaskTileW + 2 * kMaskMaxR, LHM = kMaskTileH + 2 * kMaskMaxR;
    __shared__ uint8_t m0[LHM * LWM];
    __shared__ uint8_t mh[LHM * kMaskTileW];
    __shared__ int2 sp[LHM];
    __shared__ int part[4][4];
    const int z = blockIdx.z, tx = threadIdx.x, ty = threadIdx.y, tid = ty * kMaskTileW + tx;
    const int x0 = blockIdx.x * kMaskTileW, y0 = blockIdx.y * kMaskTileH;
    const int LW = kMaskTileW + 2 * r, LH = kMaskTileH + 2 * r;
    if (HULL) {
        if (tid < LH) {
            const int gy = y0 - r + tid;
            sp[tid] = (gy >= 0 && gy < H) ? spans[(size_t)z * H + gy] : make_int2(1, 0);
        }
        __syncthreads();
    }
    const uint8_t *mk = F.mask[z];
    for (int e = tid; e < LW * LH; e += 256) {
        const int lx = e % LW, ly = e / LW, gx = x0 - r + lx, gy = y0 - r + ly;
        uint8_t v = 0;
        if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
            if (HULL) v = sp[ly].x <= gx && gx <= sp[ly].y;
            else v = mk[(size_t)gy * W + gx] != 0;
        }
        m0[ly * LW + lx] = v;
    }
    __syncthreads();
    for (int e = tid; e < kMaskTileW * LH; e += 256) {
        const int lx = e % kMaskTileW, ly = e / kMaskTileW;
        uint8_t v = 0;
        for (int d = 0; d <= 2 * r; d++) v |= m0[ly * LW + lx + d];
        mh[ly * kMaskTileW + lx] = v;
    }
    __syncthreads();
    int a0 = 0, a1 = 0, a2 = 0, a3 = 0;              // the ROI encoding above: 0 is the empty value of all four
    const int gx = x0 + tx;
    float *dep = F.depth[z];
    float4 *nrm = F.normal[z];
    uchar4 *col = F.color[z];
    uint8_t *mo = F.mask_out[z];
    for (int j = 0; j < kMaskTileH / 4; j++) {
        const int ly = ty + 4 * j, gy = y0 + ly;
        if (gx >= W || gy >= H) continue;
        uint8_t v = 0;
        for (int d = 0; d <= 2 * r; d++) v |= mh[(ly + d) * kMaskTileW + tx];
        const size_t idx = (size_t)gy * W + gx;
        if (mo) mo[idx] = v;
        if (!v) {
            dep[idx] = 0.0f;
            nrm[idx] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (col) col[idx] = make_uchar4(0, 0, 0, 0);
        } else {
            a0 = max(a0, 9999 - gx); a1 = max(a1, gx); a2 = max(a2, 9999 - gy); a3 = max(a3, gy);
        }
    }
    if (!roi) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a0 = max(a0, __shfl_xor(a0, o, 64)); a1 = max(a1, __shfl_xor(a1, o, 64));
        a2 = max(a2, __shfl_xor(a2, o, 64)); a3 = max(a3, __shfl_xor(a3, o, 64));
    }
    if (tx == 0) { part[ty][0] = a0; part[ty][1] = a1; part[ty][2] = a2; part[ty][3] = a3; }
    __syncthreads();
    if (tid < 4) {                                    // one atomic per slot and workgroup; a workgroup with nothing on the mask adds none
        const int q = tid, m = max(max(part[0][q], part[1][q]), max(part[2][q], part[3][q]));
        if (m > 0) atomicMax(roi + 4 * (base + z) + q, m);
    }
}

}  // namespace btba
