// match_host.cpp -- CPU restatement of btba_match_pairs (include/btba.h), for the tests.
//
// Same arguments as the library call minus the workspace, all on the host.  Every operation the contract fixes is written out
// explicitly: the fmaf chains of the distance, the cofactor inverse of the intrinsics and the camera-space point of
// btba_depth_to_normals, the uncontracted transform and the gate.  Built with -ffp-contract=off, so the compiler adds no fma of its
// own; a correct implementation reproduces this file's output bit for bit.  Pairs are spread over threads (results do not depend
// on their number).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <thread>
#include <vector>

#include "../../include/btba.h"

namespace {

struct Cand { float d2; int idx; };
bool cand_less(const Cand &a, const Cand &b) { return a.d2 < b.d2 || (a.d2 == b.d2 && a.idx < b.idx); }

// the generic cofactor inverse of the 4 x 4 embedding of K, in fp32 (what btba_depth_to_normals uses)
void intrinsics_inverse(const float *K, float Ki[16])
{
    const float m[16] = { K[0], K[1], K[2], 0, K[3], K[4], K[5], 0, K[6], K[7], K[8], 0, 0, 0, 0, 1 };
    auto minor = [&](int r0, int r1, int r2, int c0, int c1, int c2) {
        return m[4 * r0 + c0] * (m[4 * r1 + c1] * m[4 * r2 + c2] - m[4 * r1 + c2] * m[4 * r2 + c1])
             - m[4 * r0 + c1] * (m[4 * r1 + c0] * m[4 * r2 + c2] - m[4 * r1 + c2] * m[4 * r2 + c0])
             + m[4 * r0 + c2] * (m[4 * r1 + c0] * m[4 * r2 + c1] - m[4 * r1 + c1] * m[4 * r2 + c0]);
    };
    float adj[16];
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) {
            int rr[3], cc[3], a = 0, b = 0;
            for (int k = 0; k < 4; k++) { if (k != r) rr[a++] = k; if (k != c) cc[b++] = k; }
            const float mn = minor(rr[0], rr[1], rr[2], cc[0], cc[1], cc[2]);
            adj[4 * c + r] = ((r + c) & 1) ? -mn : mn;
        }
    const float det = m[0] * adj[0] + m[1] * adj[4] + m[2] * adj[8] + m[3] * adj[12];
    const float rdet = 1.0f / det;
    for (int k = 0; k < 16; k++) Ki[k] = adj[k] * rdet;
}

struct V3 { float x, y, z; };

struct Ctx {
    const btba_match_params *prm;
    int H, W, D;
    float Ki[16];
    const float *const *desc, *const *kpts, *const *depth, *const *normal;
    const int32_t *n;
    const float *poses;
};

bool lookup(const Ctx &c, int f, int i, V3 &pt, V3 &nrm)
{
    const float u = std::round(c.kpts[f][2 * i]), v = std::round(c.kpts[f][2 * i + 1]);
    if (!(u >= 0.0f && u < (float)c.W && v >= 0.0f && v < (float)c.H)) return false;
    const int x = (int)u, y = (int)v;
    const size_t o = (size_t)y * c.W + x;
    const float d = c.depth[f][o];
    if (!((double)d >= 0.1)) pt = V3{ 0.f, 0.f, 0.f };
    else {
        const float *K = c.Ki;
        const float vx = (float)x * d, vy = (float)y * d;
        pt = V3{ K[0] * vx + K[1] * vy + K[2] * d + K[3] * d, K[4] * vx + K[5] * vy + K[6] * d + K[7] * d, K[12] * vx + K[13] * vy + K[14] * d + K[15] * d };
    }
    if (pt.z < c.prm->min_z) return false;
    nrm = V3{ c.normal[f][4 * o], c.normal[f][4 * o + 1], c.normal[f][4 * o + 2] };
    return true;
}

V3 model_point(const float *T, const V3 &p)
{
    return V3{ T[0] * p.x + T[1] * p.y + T[2] * p.z + T[3], T[4] * p.x + T[5] * p.y + T[6] * p.z + T[7], T[8] * p.x + T[9] * p.y + T[10] * p.z + T[11] };
}

V3 model_normal(const float *T, const V3 &n)
{
    V3 r{ T[0] * n.x + T[1] * n.y + T[2] * n.z, T[4] * n.x + T[5] * n.y + T[6] * n.z, T[8] * n.x + T[9] * n.y + T[10] * n.z };
    const float z = r.x * r.x + r.y * r.y + r.z * r.z;
    if (z > 0.0f) { const float s = std::sqrt(z); r = V3{ r.x / s, r.y / s, r.z / s }; }
    return r;
}

float chain(const float *a, const float *b, int D)
{
    float s = 0.0f;
    for (int k = 0; k < D; k++) s = std::fma(a[k], b[k], s);
    return s;
}

// one direction: for every query of frame fq, its first gated neighbour in frame ft (slot -1 = none) and that neighbour
void direction(const Ctx &c, int fq, int ft, float max_dist, float cos_max, std::vector<Cand> &best)
{
    const int nq = c.n[fq], nt = c.n[ft], D = c.D, k = std::min(c.prm->k, nt);
    best.assign(nq, Cand{ 0.0f, -1 });
    if (nq == 0 || nt == 0) return;
    std::vector<float> tn(nt), tt((size_t)D * nt);
    for (int j = 0; j < nt; j++) {
        tn[j] = chain(c.desc[ft] + (size_t)j * D, c.desc[ft] + (size_t)j * D, D);
        for (int d = 0; d < D; d++) tt[(size_t)d * nt + j] = c.desc[ft][(size_t)j * D + d];
    }
    std::vector<float> dot(nt);
    std::vector<Cand> list;
    for (int i = 0; i < nq; i++) {
        const float *a = c.desc[fq] + (size_t)i * D;
        const float na = chain(a, a, D);
        std::fill(dot.begin(), dot.end(), 0.0f);
        for (int d = 0; d < D; d++) {                           // the k-th link of every chain at once (each chain stays in k order)
            const float ad = a[d];
            const float *row = tt.data() + (size_t)d * nt;
            for (int j = 0; j < nt; j++) dot[j] = std::fma(ad, row[j], dot[j]);
        }
        list.clear();
        for (int j = 0; j < nt; j++) {
            const float x = std::fma(-2.0f, dot[j], na + tn[j]);
            const Cand cj{ x > 0.0f ? x : 0.0f, j };
            if ((int)list.size() < k) list.insert(std::upper_bound(list.begin(), list.end(), cj, cand_less), cj);
            else if (cand_less(cj, list.back())) { list.pop_back(); list.insert(std::upper_bound(list.begin(), list.end(), cj, cand_less), cj); }
        }
        V3 pq, nq3;
        if (!lookup(c, fq, i, pq, nq3)) continue;
        const V3 PQ = model_point(c.poses + 16 * fq, pq), NQ = model_normal(c.poses + 16 * fq, nq3);
        for (const Cand &m : list) {
            V3 pt, nt3;
            if (!lookup(c, ft, m.idx, pt, nt3)) continue;
            const V3 PT = model_point(c.poses + 16 * ft, pt), NT = model_normal(c.poses + 16 * ft, nt3);
            const float dx = PQ.x - PT.x, dy = PQ.y - PT.y, dz = PQ.z - PT.z;
            if (std::sqrt(dx * dx + dy * dy + dz * dz) > max_dist) continue;
            if (NQ.x * NT.x + NQ.y * NT.y + NQ.z * NT.z < cos_max) continue;
            best[i] = m;
            break;
        }
    }
}

}  // namespace

extern "C" __attribute__((visibility("default"))) int match_host(const btba_match_params *prm, int n_frames, int H, int W, const float *K,
                                                                  const float *const *desc, int D, const float *const *kpts, const int32_t *n_kpts,
                                                                  const float *const *depth, const float *const *normal, const float *poses,
                                                                  const int32_t *frame_ids, int n_pairs, const int32_t *pairs,
                                                                  btba_match *out, float *ptsA, float *ptsB, int32_t *n_out, int n_threads)
{
    Ctx c{ prm, H, W, D, {}, desc, kpts, depth, normal, n_kpts, poses };
    intrinsics_inverse(K, c.Ki);
    std::vector<std::vector<btba_match>> per(n_pairs);
    auto run = [&](int p) {
        const int a = pairs[2 * p], b = pairs[2 * p + 1];
        const bool neighbor = std::abs((long long)frame_ids[a] - (long long)frame_ids[b]) == 1;
        const float md = neighbor ? prm->max_dist_neighbor : prm->max_dist_no_neighbor;
        const float cm = neighbor ? prm->cos_max_normal_neighbor : prm->cos_max_normal_no_neighbor;
        std::vector<Cand> ab, ba;
        direction(c, a, b, md, cm, ab);
        if (prm->mutual) direction(c, b, a, md, cm, ba);
        for (int dir = 0; dir < (prm->mutual ? 2 : 1); dir++) {
            const std::vector<Cand> &v = dir ? ba : ab;
            for (int i = 0; i < (int)v.size(); i++) {
                if (v[i].idx < 0) continue;
                btba_match r{};
                r.idx_a = dir ? v[i].idx : i;
                r.idx_b = dir ? i : v[i].idx;
                r.dist = std::sqrt(v[i].d2);
                r.dir = dir;
                V3 pa, pb, na, nb;
                lookup(c, a, r.idx_a, pa, na);
                lookup(c, b, r.idx_b, pb, nb);
                std::memcpy(r.ptA_cam, &pa, 12);
                std::memcpy(r.ptB_cam, &pb, 12);
                per[p].push_back(r);
            }
        }
    };
    std::vector<std::thread> pool;
    const int T = std::max(1, std::min(n_threads, n_pairs));
    for (int t = 0; t < T; t++)
        pool.emplace_back([&, t] { for (int p = t; p < n_pairs; p += T) run(p); });
    for (auto &th : pool) th.join();
    size_t o = 0;
    for (int p = 0; p < n_pairs; p++) {
        n_out[p] = (int32_t)per[p].size();
        const int a = pairs[2 * p], b = pairs[2 * p + 1];
        for (const btba_match &r : per[p]) {
            out[o] = r;
            const V3 PA = model_point(poses + 16 * a, V3{ r.ptA_cam[0], r.ptA_cam[1], r.ptA_cam[2] });
            const V3 PB = model_point(poses + 16 * b, V3{ r.ptB_cam[0], r.ptB_cam[1], r.ptB_cam[2] });
            if (ptsA) { ptsA[4 * o] = PA.x; ptsA[4 * o + 1] = PA.y; ptsA[4 * o + 2] = PA.z; ptsA[4 * o + 3] = 1.0f; }
            if (ptsB) { ptsB[4 * o] = PB.x; ptsB[4 * o + 1] = PB.y; ptsB[4 * o + 2] = PB.z; ptsB[4 * o + 3] = 1.0f; }
            o++;
        }
    }
    return 0;
}
static_assert(sizeof(btba_match) == 40, "btba_match is 40 bytes");
