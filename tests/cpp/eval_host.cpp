// eval_host.cpp -- CPU restatement of btba_pose_errors (include/btba.h), for the tests.
//
// Same arguments as the library call minus the workspace, all on the host.  Every operation the contract fixes is written out:
// the fmaf chains of the transforms, d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx)), the correctly rounded sqrtf, the fp64 sum in
// 256 slots and the binary tree over them.  Built with -ffp-contract=off, so the compiler adds no fma of its own; a correct
// implementation reproduces this file's output bit for bit.  Queries are spread over threads (results do not depend on their
// number: each query's minimum is its own, and the sums run afterwards in the fixed order).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <thread>
#include <vector>

namespace {

struct P3 { float x, y, z; };

P3 xform(const float *T, const float *p)
{
    return { std::fma(T[2], p[2], std::fma(T[1], p[1], std::fma(T[0], p[0], T[3]))),
             std::fma(T[6], p[2], std::fma(T[5], p[1], std::fma(T[4], p[0], T[7]))),
             std::fma(T[10], p[2], std::fma(T[9], p[1], std::fma(T[8], p[0], T[11]))) };
}

float d2(P3 a, P3 b)
{
    const float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
    return std::fma(dz, dz, std::fma(dy, dy, dx * dx));
}

bool finite_pose(const float *P, const float *G)
{
    for (int k = 0; k < 16; k++)
        if (!std::isfinite(P[k]) || !std::isfinite(G[k])) return false;
    return true;
}

// (double) d_i summed in slot i % 256 in ascending i, then acc[l] += acc[l + s] for s = 128 .. 1
float fixed_mean(const std::vector<float> &d)
{
    double acc[256] = {};
    for (size_t i = 0; i < d.size(); i++) acc[i % 256] += (double)d[i];
    for (int s = 128; s >= 1; s >>= 1)
        for (int l = 0; l < s; l++) acc[l] += acc[l + s];
    return (float)(acc[0] / (double)d.size());
}

}  // namespace

extern "C" __attribute__((visibility("default"))) void eval_host(int n_models, const float *const *model_pts, const int32_t *n_pts, int n_evals,
                                                                const int32_t *model_index, const float *poses_pred, const float *poses_gt,
                                                                float *add_out, float *adds_out, int n_threads)
{
    (void)n_models;
    for (int e = 0; e < n_evals; e++) {
        const float *P = poses_pred + 16 * (size_t)e, *G = poses_gt + 16 * (size_t)e;
        if (!finite_pose(P, G)) {
            add_out[e] = adds_out[e] = std::numeric_limits<float>::quiet_NaN();
            continue;
        }
        const float *x = model_pts[model_index[e]];
        const int n = n_pts[model_index[e]];
        std::vector<P3> q(n), c(n);
        for (int i = 0; i < n; i++) { q[i] = xform(G, x + 3 * (size_t)i); c[i] = xform(P, x + 3 * (size_t)i); }
        std::vector<float> add(n), adds(n);
        const int T = std::max(1, std::min(n_threads, (n + 63) / 64));
        std::vector<std::thread> pool;
        for (int t = 0; t < T; t++)
            pool.emplace_back([&, t] {
                for (int i = t; i < n; i += T) {
                    float m = std::numeric_limits<float>::infinity();
                    const P3 qi = q[i];
                    for (int j = 0; j < n; j++) {
                        const float v = d2(qi, c[j]);
                        m = v < m ? v : m;
                    }
                    add[i] = std::sqrt(d2(qi, c[i]));
                    adds[i] = std::sqrt(m);
                }
            });
        for (auto &th : pool) th.join();
        add_out[e] = fixed_mean(add);
        adds_out[e] = fixed_mean(adds);
    }
}
