// btba_fusion_point.hpp -- the per-point device functions of keyframe fusion (btba_fusion.hpp) that frame-to-model registration
// (btba_register.hpp) shares: how a segment's element is taken or dropped, its bit-exact p = T x and rotated normal, the voxel rule, and the
// integer wave folds.  Functions only, no kernel: both translation units include it.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/btba.h"
#include "btba_image.hpp"

namespace btba {

constexpr int kFuseChunk = BTBA_FUSE_CHUNK;            // segments (accumulate, bounds), instances (compaction) or registration items per launch
constexpr float kFuseMaxCoord = 65536.0f;              // |p_a| >= 2^16 m: outside

__device__ __forceinline__ int wave_min_i(int v)
{
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ int wave_max_i(int v)
{
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ int wave_sum_i(int v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// The model-frame point (and normal) of element e of a segment given by its parts, by the header's rules.  false: the element is dropped without
// being counted (no depth, a zero normal under require_normals, a non-finite coordinate).
__device__ __forceinline__ bool fuse_point_at(bool frame, const void *geom, const float4 *nmap, const float *T, int e, int W, const Mat4 &Kinv,
                                              bool require_normals, bool want_normal, float3 &p, float3 &nrm)
{
#pragma clang fp contract(off)
    float3 c;
    float4 nq = make_float4(0.f, 0.f, 0.f, 0.f);
    if (frame) {
        const float d = static_cast<const float *>(geom)[e];
        if (!((double)d >= 0.1)) return false;
        const bool test_normal = require_normals && nmap;
        if (test_normal || (want_normal && nmap)) nq = nmap[e];
        if (test_normal && nq.x == 0.0f && nq.y == 0.0f && nq.z == 0.0f) return false;
        const int y = e / W, x = e - y * W;
        c = backproject(Kinv.m, x, y, d);
    } else {
        const float4 q = static_cast<const float4 *>(geom)[e];
        if (!(fabsf(q.x) < INFINITY && fabsf(q.y) < INFINITY && fabsf(q.z) < INFINITY)) return false;
        c = make_float3(q.x, q.y, q.z);
        if (want_normal && nmap) nq = nmap[e];
    }
    p.x = ((T[0] * c.x + T[1] * c.y) + T[2] * c.z) + T[3];
    p.y = ((T[4] * c.x + T[5] * c.y) + T[6] * c.z) + T[7];
    p.z = ((T[8] * c.x + T[9] * c.y) + T[10] * c.z) + T[11];
    nrm.x = (T[0] * nq.x + T[1] * nq.y) + T[2] * nq.z;
    nrm.y = (T[4] * nq.x + T[5] * nq.y) + T[6] * nq.z;
    nrm.z = (T[8] * nq.x + T[9] * nq.y) + T[10] * nq.z;
    if (!(fabsf(nrm.x) < kFuseMaxCoord && fabsf(nrm.y) < kFuseMaxCoord && fabsf(nrm.z) < kFuseMaxCoord)) nrm = make_float3(0.f, 0.f, 0.f);
    return true;
}

// floorf(p_a inv_leaf) as integers; false when |p_a| >= 2^16 (or NaN).  inv_leaf <= 2^14 (the host's check), so the floor is below 2^30.
__device__ __forceinline__ bool fuse_cell(const float3 &p, float inv_leaf, int &cx, int &cy, int &cz)
{
#pragma clang fp contract(off)
    if (!(fabsf(p.x) < kFuseMaxCoord && fabsf(p.y) < kFuseMaxCoord && fabsf(p.z) < kFuseMaxCoord)) return false;
    cx = (int)floorf(p.x * inv_leaf);
    cy = (int)floorf(p.y * inv_leaf);
    cz = (int)floorf(p.z * inv_leaf);
    return true;
}

}  // namespace btba
