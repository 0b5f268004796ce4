// btba_api_register.hip -- host side of libbtba.so: frame-to-model registration against the fused cloud (btba_register.hpp).
#include "btba_host_common.hpp"
#include "btba_fusion_layout.hpp"
#include "btba_register.hpp"

#include <algorithm>
#include <limits>

namespace {

constexpr int kRegAssociateGridX = 1024;                // blocks per item of the association pass: the kernel strides over the rest

// What btba_register_frames and btba_register_associate share, all of it decided before any HIP call: the argument checks, the device form of
// the parameters, the instances' first cells and the items' first partial records.
struct RegisterCall {
    RegParams P{};
    std::vector<int64_t> vox_off, part_off;
    RegisterLayout L;
};

bool model_ok(int n_instances, const int32_t *box, int capacity, std::vector<int64_t> &vox_off)
{
    if (n_instances < 1 || !box || capacity < 0 || (int64_t)n_instances * capacity > (int64_t)std::numeric_limits<int32_t>::max()) return false;
    for (int b = 0; b < n_instances; b++)
        for (int a = 0; a < 3; a++)
            if (box[6 * (size_t)b + a] > (1 << 30) || box[6 * (size_t)b + a] < -(1 << 30)) return false;
    vox_off.assign((size_t)n_instances + 1, 0);
    return fuse_layout(n_instances, box, vox_off.data(), nullptr, nullptr);
}

bool register_call_ok(const btba_register_params *prm, int n_instances, int n_items, const btba_fuse_segment *seg, int H, int W, const float *K,
                      const int32_t *box, int capacity, const float *xyz, const float *normal, const int32_t *cell, RegisterCall &c)
{
    const float inf = std::numeric_limits<float>::infinity();
    if (!prm || !xyz || !normal || !cell || misaligned(xyz, 16) || misaligned(normal, 16) || misaligned(cell, 4)) return false;
    if (prm->search_radius < 0 || prm->search_radius > 2 || prm->n_iters < 0 || prm->n_iters > BTBA_REG_MAX_ITERATIONS || prm->min_matches < 0) return false;
    if (!(prm->max_dist >= 0.0f) || !(prm->max_dist < inf) || !(prm->huber_delta > 0.0f) || !(prm->huber_delta < inf) || prm->min_cos != prm->min_cos) return false;
    if (!(prm->eps_rot >= 0.0f) || !(prm->eps_trans >= 0.0f)) return false;
    btba_fuse_params fp{};
    fp.leaf = prm->leaf;
    fp.min_points = 1;
    fp.require_normals = prm->require_normals;
    if (!fuse_segments_ok(&fp, n_instances, n_items, seg, H, W, K, false)) return false;
    if (!model_ok(n_instances, box, capacity, c.vox_off)) return false;
    std::vector<int64_t> n_points((size_t)n_items);
    for (int i = 0; i < n_items; i++) n_points[i] = seg[i].kind == BTBA_FUSE_FRAME ? (int64_t)H * W : seg[i].n;
    c.part_off.assign((size_t)n_items + 1, 0);
    if (!register_layout(n_items, n_points.data(), c.part_off.data(), &c.L)) return false;
    c.P.inv_leaf = 1.0f / prm->leaf;
    c.P.max_dist2 = prm->max_dist * prm->max_dist;
    c.P.min_cos = prm->min_cos;
    c.P.delta = prm->huber_delta;
    c.P.radius = prm->search_radius;
    c.P.require_normals = prm->require_normals;
    c.P.min_matches = prm->min_matches;
    c.P.n_iters = prm->n_iters;
    c.P.eps_rot = (double)prm->eps_rot;
    c.P.eps_trans = (double)prm->eps_trans;
    return true;
}

// chunk [s0, s0 + ns) of the items as the kernels take it; returns the largest element count of the chunk
int register_chunk(const btba_fuse_segment *seg, int s0, int ns, int H, int W, const int32_t *box, const RegisterCall &c, RegItems &S, RegPoses &Q)
{
    int n_max = 0;
    S.first = s0;
    for (int z = 0; z < ns; z++) {
        const btba_fuse_segment &g = seg[s0 + z];
        S.geom[z] = g.geom;
        S.normal[z] = static_cast<const float4 *>(g.normal);
        S.n[z] = g.kind == BTBA_FUSE_FRAME ? H * W : (int)g.n;
        S.kind_instance[z] = g.instance * 2 + g.kind;
        for (int a = 0; a < 3; a++) { S.min_b[z][a] = box[6 * (size_t)g.instance + a]; S.dims[z][a] = box[6 * (size_t)g.instance + 3 + a]; }
        S.vox_off[z] = (uint32_t)c.vox_off[g.instance];
        S.part_off[z] = (uint32_t)c.part_off[s0 + z];
        std::memcpy(Q.pose[z], g.pose, sizeof(float) * 12);
        n_max = std::max(n_max, S.n[z]);
    }
    return n_max;
}

}  // namespace

extern "C" {

void btba_register_params_default(btba_register_params *p)
{
    if (!p) return;
    p->leaf = 0.0f;                       // no default: the model's
    p->search_radius = 1;
    p->max_dist = 0.02f;
    p->min_cos = 0.70710678118654752f;
    p->huber_delta = 0.005f;
    p->n_iters = 10;
    p->eps_rot = 1e-5f;
    p->eps_trans = 1e-6f;
    p->min_matches = 6;
    p->require_normals = 1;
    p->reserved = 0;
}

int btba_register_index(btba_workspace *ws, int n_instances, const int32_t *box, int capacity, const int32_t *lin_dev, const int32_t *n_out_dev,
                        int32_t *cell_index_dev)
{
    // every argument is checked before the first HIP call
    if (!ws || !lin_dev || !n_out_dev || !cell_index_dev || misaligned(lin_dev, 4) || misaligned(n_out_dev, 4) || misaligned(cell_index_dev, 4)) return BTBA_EINVAL;
    std::vector<int64_t> vox_off;
    if (!model_ok(n_instances, box, capacity, vox_off)) return BTBA_EINVAL;
    DeviceGuard device_guard(ws);
    const int64_t V = vox_off[n_instances];
    if (V > 0) HIP_TRY(hipMemsetAsync(cell_index_dev, 0xFF, sizeof(int32_t) * (size_t)V, ws->stream));      // -1
    if (V == 0 || capacity == 0) return BTBA_OK;
    for (int b0 = 0; b0 < n_instances; b0 += kFuseChunk) {
        const int nb = std::min(kFuseChunk, n_instances - b0);
        RegIndexInstances I{};
        for (int z = 0; z < nb; z++) {
            I.vox_off[z] = (uint32_t)vox_off[b0 + z];
            I.n_vox[z] = (int32_t)(vox_off[b0 + z + 1] - vox_off[b0 + z]);
        }
        k_register_index<<<dim3((capacity + 255) / 256, nb), 256, 0, ws->stream>>>(I, b0, capacity, lin_dev, n_out_dev, cell_index_dev);
        HIP_TRY(hipGetLastError());
    }
    return BTBA_OK;
}

int btba_register_frames(btba_workspace *ws, const btba_register_params *prm, int n_instances, int n_items, const btba_fuse_segment *segments, int H, int W,
                         const float *K, const int32_t *box, int capacity, const float *xyz_dev, const float *normal_dev, const int32_t *cell_index_dev,
                         float *pose_out_dev, btba_register_result *result_dev, btba_register_iter *trace_dev)
{
    // every argument is checked before the first HIP call
    if (!ws || !pose_out_dev || !result_dev || misaligned(pose_out_dev, 4) || misaligned(result_dev, 8) || misaligned(trace_dev, 8)) return BTBA_EINVAL;
    RegisterCall c;
    if (!register_call_ok(prm, n_instances, n_items, segments, H, W, K, box, capacity, xyz_dev, normal_dev, cell_index_dev, c)) return BTBA_EINVAL;
    if (n_items == 0) return BTBA_OK;

    DeviceGuard device_guard(ws);
    if (int rc = ws->registration.ensure(std::max(c.L.total, (size_t)256))) return rc;
    unsigned char *base = ws->registration.as<unsigned char>();
    RegScratch X{ reinterpret_cast<double *>(base + c.L.partials), reinterpret_cast<float *>(base + c.L.poses), reinterpret_cast<int32_t *>(base + c.L.state) };
    const RegModel M{ reinterpret_cast<const float4 *>(xyz_dev), reinterpret_cast<const float4 *>(normal_dev), cell_index_dev, capacity };
    Mat4 Kinv{};
    float intr[4];
    if (fuse_has_frames(n_items, segments)) scaled_intrinsics(H, W, H, W, K, intr, &Kinv);      // btba_depth_to_normals' inverse

    // the chunks are built once: every iteration launches over the same kernel arguments
    struct Chunk { RegItems S{}; int ns = 0, n_max = 0; };
    std::vector<Chunk> chunks;
    for (int s0 = 0; s0 < n_items; s0 += kFuseChunk) {
        Chunk ch;
        RegPoses Q{};
        ch.ns = std::min(kFuseChunk, n_items - s0);
        ch.n_max = register_chunk(segments, s0, ch.ns, H, W, box, c, ch.S, Q);
        k_register_init<<<(ch.ns * 12 + 255) / 256, 256, 0, ws->stream>>>(Q, s0, ch.ns, X);
        HIP_TRY(hipGetLastError());
        chunks.push_back(ch);
    }
    for (int it = 0; it <= prm->n_iters; it++) {
        const int final = it == prm->n_iters;
        for (const Chunk &ch : chunks) {
            if (ch.n_max > 0) {
                k_register_accumulate<<<dim3((unsigned)register_blocks(ch.n_max), ch.ns), kRegThreads, 0, ws->stream>>>(W, Kinv, c.P, ch.S, M, X, final);
                HIP_TRY(hipGetLastError());
            }
            k_register_solve<<<ch.ns, 64, 0, ws->stream>>>(c.P, ch.S, X, it, final, pose_out_dev, result_dev, trace_dev);
            HIP_TRY(hipGetLastError());
        }
    }
    return BTBA_OK;
}

int btba_register_associate(btba_workspace *ws, const btba_register_params *prm, int n_instances, int n_items, const btba_fuse_segment *segments, int H, int W,
                            const float *K, const int32_t *box, int capacity, const float *xyz_dev, const float *normal_dev, const int32_t *cell_index_dev,
                            int32_t *const *match_out)
{
    // every argument is checked before the first HIP call
    if (!ws || (n_items > 0 && !match_out)) return BTBA_EINVAL;
    RegisterCall c;
    if (!register_call_ok(prm, n_instances, n_items, segments, H, W, K, box, capacity, xyz_dev, normal_dev, cell_index_dev, c)) return BTBA_EINVAL;
    for (int i = 0; i < n_items; i++) {
        const int64_t n = segments[i].kind == BTBA_FUSE_FRAME ? (int64_t)H * W : segments[i].n;
        if ((n > 0 && !match_out[i]) || misaligned(match_out[i], 4)) return BTBA_EINVAL;
    }
    DeviceGuard device_guard(ws);
    const RegModel M{ reinterpret_cast<const float4 *>(xyz_dev), reinterpret_cast<const float4 *>(normal_dev), cell_index_dev, capacity };
    Mat4 Kinv{};
    float intr[4];
    if (fuse_has_frames(n_items, segments)) scaled_intrinsics(H, W, H, W, K, intr, &Kinv);
    for (int s0 = 0; s0 < n_items; s0 += kFuseChunk) {
        const int ns = std::min(kFuseChunk, n_items - s0);
        RegItems S{};
        RegPoses Q{};
        RegMatchOut O{};
        const int n_max = register_chunk(segments, s0, ns, H, W, box, c, S, Q);
        for (int z = 0; z < ns; z++) O.out[z] = match_out[s0 + z];
        if (n_max == 0) continue;
        k_register_associate<<<dim3(std::min((n_max + 255) / 256, kRegAssociateGridX), ns), 256, 0, ws->stream>>>(W, Kinv, c.P, S, Q, M, O);
        HIP_TRY(hipGetLastError());
    }
    return BTBA_OK;
}

}  // extern "C"
