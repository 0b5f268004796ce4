// btba_api_fusion.hip -- host side of libbtba.so: keyframe fusion and voxel-grid downsampling (btba_fusion.hpp).
#include "btba_host_common.hpp"
#include "btba_fusion.hpp"

#include <algorithm>
#include <limits>

namespace btba_host {

// Everything btba_fuse_bounds and btba_fuse_frames share (and btba_api_register.hip takes over): the checks of params and segments, decided
// before any HIP call.
bool fuse_segments_ok(const btba_fuse_params *prm, int n_instances, int n_segments, const btba_fuse_segment *seg, int H, int W, const float *K,
                      bool need_colour)
{
    if (!prm || n_instances < 1 || n_segments < 0 || (n_segments > 0 && !seg)) return false;
    if (!(prm->leaf >= 0.00006103515625f) || !(prm->leaf < std::numeric_limits<float>::infinity()) || prm->min_points < 1) return false;      // 2^-14
    for (int s = 0; s < n_segments; s++) {
        const btba_fuse_segment &g = seg[s];
        if (g.instance < 0 || g.instance >= n_instances || misaligned(g.normal, 16) || misaligned(g.colour, 4)) return false;
        if (g.kind == BTBA_FUSE_FRAME) {
            if (H < 1 || W < 1 || (int64_t)H * W > ((int64_t)1 << 30) || !K || !g.geom || misaligned(g.geom, 4)) return false;
            if ((prm->require_normals && !g.normal) || (need_colour && !g.colour)) return false;
        } else if (g.kind == BTBA_FUSE_POINTS) {
            if (g.n < 0 || g.n > ((int64_t)1 << 30) || misaligned(g.geom, 16)) return false;
            if (g.n > 0 && (!g.geom || (need_colour && !g.colour))) return false;      // an empty list needs no arrays
        } else {
            return false;
        }
    }
    return true;
}

bool fuse_has_frames(int n_segments, const btba_fuse_segment *seg)
{
    for (int s = 0; s < n_segments; s++) if (seg[s].kind == BTBA_FUSE_FRAME) return true;
    return false;
}

}  // namespace btba_host

namespace {

// chunk [s0, s0 + ns) of the segments as the kernels take it; the box and first voxel of each segment's instance when box is given.
// Returns the largest element count of the chunk.
int fuse_chunk(const btba_fuse_segment *seg, int s0, int ns, int H, int W, const int32_t *box, const int64_t *vox_off, FuseSegments &S)
{
    int n_max = 0;
    for (int z = 0; z < ns; z++) {
        const btba_fuse_segment &g = seg[s0 + z];
        S.geom[z] = g.geom;
        S.normal[z] = static_cast<const float4 *>(g.normal);
        S.colour[z] = static_cast<const uchar4 *>(g.colour);
        std::memcpy(S.pose[z], g.pose, sizeof(float) * 12);
        S.n[z] = g.kind == BTBA_FUSE_FRAME ? H * W : (int)g.n;
        S.kind_instance[z] = g.instance * 2 + g.kind;
        if (box) {
            for (int a = 0; a < 3; a++) { S.min_b[z][a] = box[6 * (size_t)g.instance + a]; S.dims[z][a] = box[6 * (size_t)g.instance + 3 + a]; }
            S.vox_off[z] = (uint32_t)vox_off[g.instance];
        }
        n_max = std::max(n_max, S.n[z]);
    }
    return n_max;
}

constexpr int kFuseMaxGridX = 1024;                     // blocks per segment: the kernels stride over the rest
constexpr int kFuseBoundsGridX = 64;                    // ... of the bounds pass: every workgroup ends in six atomics on its instance's six words, so few, long-striding ones

}  // namespace

extern "C" {

void btba_fuse_params_default(btba_fuse_params *p)
{
    if (!p) return;
    p->leaf = 0.005f;
    p->min_points = 1;
    p->require_normals = 1;
    p->normalize_normals = 0;
}

int btba_fuse_layout(int n_instances, const int32_t *box, int64_t *voxel_offsets_out, int64_t *scratch_bytes_out)
{
    if (n_instances < 1 || !box) return BTBA_EINVAL;
    FuseLayout L;
    if (!fuse_layout(n_instances, box, voxel_offsets_out, nullptr, &L)) return BTBA_EINVAL;
    if (scratch_bytes_out) *scratch_bytes_out = (int64_t)L.total;
    return BTBA_OK;
}

int btba_fuse_bounds(btba_workspace *ws, const btba_fuse_params *prm, int n_instances, int n_segments, const btba_fuse_segment *segments,
                     int H, int W, const float *K, int32_t *box_out_dev)
{
    // every argument is checked before the first HIP call
    if (!ws || !box_out_dev || misaligned(box_out_dev, 4) || !fuse_segments_ok(prm, n_instances, n_segments, segments, H, W, K, false)) return BTBA_EINVAL;
    DeviceGuard device_guard(ws);
    Mat4 Kinv{};
    float intr[4];
    if (fuse_has_frames(n_segments, segments)) scaled_intrinsics(H, W, H, W, K, intr, &Kinv);      // btba_depth_to_normals' inverse
    const float inv_leaf = 1.0f / prm->leaf;
    k_fuse_bounds_init<<<(6 * n_instances + 255) / 256, 256, 0, ws->stream>>>(n_instances, box_out_dev);
    HIP_TRY(hipGetLastError());
    for (int s0 = 0; s0 < n_segments; s0 += kFuseChunk) {
        const int ns = std::min(kFuseChunk, n_segments - s0);
        FuseSegments S{};
        const int n_max = fuse_chunk(segments, s0, ns, H, W, nullptr, nullptr, S);
        if (n_max == 0) continue;
        k_fuse_bounds<<<dim3(std::min((n_max + 255) / 256, kFuseBoundsGridX), ns), 256, 0, ws->stream>>>(W, Kinv, inv_leaf, prm->require_normals, S, box_out_dev);
        HIP_TRY(hipGetLastError());
    }
    k_fuse_bounds_finish<<<(n_instances + 255) / 256, 256, 0, ws->stream>>>(n_instances, box_out_dev);
    HIP_TRY(hipGetLastError());
    return BTBA_OK;
}

int btba_fuse_frames(btba_workspace *ws, const btba_fuse_params *prm, int n_instances, int n_segments, const btba_fuse_segment *segments,
                     int H, int W, const float *K, const int32_t *box, int capacity, float *xyz_out_dev, float *normal_out_dev,
                     uint8_t *colour_out_dev, uint32_t *count_out_dev, int32_t *lin_out_dev, int32_t *n_out_dev, int32_t *n_outside_dev,
                     int32_t *status_dev)
{
    // every argument is checked before the first HIP call
    if (!ws || !box || capacity < 0 || !xyz_out_dev || !n_out_dev || !n_outside_dev || !status_dev) return BTBA_EINVAL;
    if (misaligned(xyz_out_dev, 16) || misaligned(normal_out_dev, 16) || misaligned(colour_out_dev, 4) || misaligned(count_out_dev, 4) ||
        misaligned(lin_out_dev, 4) || misaligned(n_out_dev, 4) || misaligned(n_outside_dev, 4) || misaligned(status_dev, 4))
        return BTBA_EINVAL;
    if (!fuse_segments_ok(prm, n_instances, n_segments, segments, H, W, K, colour_out_dev != nullptr)) return BTBA_EINVAL;
    if ((int64_t)n_instances * capacity > (int64_t)std::numeric_limits<int32_t>::max()) return BTBA_EINVAL;
    for (int b = 0; b < n_instances; b++)
        for (int a = 0; a < 3; a++)
            if (box[6 * (size_t)b + a] > (1 << 30) || box[6 * (size_t)b + a] < -(1 << 30)) return BTBA_EINVAL;
    std::vector<int64_t> vox_off((size_t)n_instances + 1), blk_off((size_t)n_instances + 1);
    FuseLayout L;
    if (!fuse_layout(n_instances, box, vox_off.data(), blk_off.data(), &L)) return BTBA_EINVAL;

    DeviceGuard device_guard(ws);
    if (int rc = ws->fusion.ensure(std::max(L.total, (size_t)256))) return rc;
    unsigned char *base = ws->fusion.as<unsigned char>();
    FusePlanes P{};
    P.count = reinterpret_cast<uint32_t *>(base + L.count);
    P.xyz = reinterpret_cast<unsigned long long *>(base + L.xyz);
    P.normal = normal_out_dev ? reinterpret_cast<unsigned long long *>(base + L.normal) : nullptr;
    P.colour = colour_out_dev ? reinterpret_cast<uint32_t *>(base + L.colour) : nullptr;
    P.stride = L.plane_stride;
    uint32_t *block_counts = reinterpret_cast<uint32_t *>(base + L.block_counts);
    // clear: only the planes that will be read -- count and position (one prefix, with the normal sums behind them when wanted), colour
    if (L.voxels > 0) {
        HIP_TRY(hipMemsetAsync(base, 0, normal_out_dev ? L.colour : L.normal, ws->stream));
        if (colour_out_dev) HIP_TRY(hipMemsetAsync(base + L.colour, 0, L.block_counts - L.colour, ws->stream));
    }
    HIP_TRY(hipMemsetAsync(n_outside_dev, 0, sizeof(int32_t) * (size_t)n_instances, ws->stream));

    Mat4 Kinv{};
    float intr[4];
    if (fuse_has_frames(n_segments, segments)) scaled_intrinsics(H, W, H, W, K, intr, &Kinv);      // btba_depth_to_normals' inverse
    const float inv_leaf = 1.0f / prm->leaf;
    for (int s0 = 0; s0 < n_segments; s0 += kFuseChunk) {
        const int ns = std::min(kFuseChunk, n_segments - s0);
        FuseSegments S{};
        const int n_max = fuse_chunk(segments, s0, ns, H, W, box, vox_off.data(), S);
        if (n_max == 0) continue;
        k_fuse_accumulate<<<dim3(std::min((n_max + 255) / 256, kFuseMaxGridX), ns), 256, 0, ws->stream>>>(W, Kinv, inv_leaf, prm->require_normals, S, P, n_outside_dev);
        HIP_TRY(hipGetLastError());
    }

    FuseOutputs O{};
    O.xyz = reinterpret_cast<float4 *>(xyz_out_dev);
    O.normal = reinterpret_cast<float4 *>(normal_out_dev);
    O.colour = reinterpret_cast<uchar4 *>(colour_out_dev);
    O.count = count_out_dev;
    O.lin = lin_out_dev;
    O.n_out = n_out_dev;
    O.status = status_dev;
    O.capacity = capacity;
    for (int b0 = 0; b0 < n_instances; b0 += kFuseChunk) {
        const int nb = std::min(kFuseChunk, n_instances - b0);
        FuseInstances I{};
        int64_t blocks_max = 0;
        for (int z = 0; z < nb; z++) {
            I.vox_off[z] = (uint32_t)vox_off[b0 + z];
            I.blk_off[z] = (uint32_t)blk_off[b0 + z];
            I.n_vox[z] = (int32_t)(vox_off[b0 + z + 1] - vox_off[b0 + z]);
            blocks_max = std::max(blocks_max, blk_off[b0 + z + 1] - blk_off[b0 + z]);
        }
        if (blocks_max > 0) {
            k_fuse_block_counts<<<dim3((unsigned)blocks_max, nb), kFuseBlockThreads, 0, ws->stream>>>(I, P.count, (uint32_t)prm->min_points, block_counts);
            HIP_TRY(hipGetLastError());
        }
        k_fuse_scan<<<nb, 256, 0, ws->stream>>>(I, b0, block_counts, capacity, n_out_dev, status_dev);
        HIP_TRY(hipGetLastError());
        if (blocks_max > 0 && capacity > 0) {
            k_fuse_scatter<<<dim3((unsigned)blocks_max, nb), kFuseBlockThreads, 0, ws->stream>>>(I, b0, P, block_counts, (uint32_t)prm->min_points,
                                                                                                 prm->normalize_normals, O);
            HIP_TRY(hipGetLastError());
        }
    }
    return BTBA_OK;
}

int btba_voxel_downsample(btba_workspace *ws, const btba_fuse_params *prm, int n_instances, const float *const *xyz_dev,
                          const float *const *normal_dev, const uint8_t *const *colour_dev, const int64_t *n_points, const int32_t *box,
                          int capacity, float *xyz_out_dev, float *normal_out_dev, uint8_t *colour_out_dev, uint32_t *count_out_dev,
                          int32_t *lin_out_dev, int32_t *n_out_dev, int32_t *n_outside_dev, int32_t *status_dev)
{
    if (n_instances < 1 || !xyz_dev || !n_points) return BTBA_EINVAL;
    std::vector<btba_fuse_segment> seg((size_t)n_instances);
    for (int b = 0; b < n_instances; b++) {
        btba_fuse_segment &g = seg[b];
        g = btba_fuse_segment{};
        g.kind = BTBA_FUSE_POINTS;
        g.instance = b;
        g.n = n_points[b];
        g.geom = xyz_dev[b];
        g.normal = normal_dev ? normal_dev[b] : nullptr;
        g.colour = colour_dev ? colour_dev[b] : nullptr;
        g.pose[0] = g.pose[5] = g.pose[10] = g.pose[15] = 1.0f;
    }
    return btba_fuse_frames(ws, prm, n_instances, n_instances, seg.data(), 0, 0, nullptr, box, capacity, xyz_out_dev, normal_out_dev, colour_out_dev,
                            count_out_dev, lin_out_dev, n_out_dev, n_outside_dev, status_dev);
}

}  // extern "C"
