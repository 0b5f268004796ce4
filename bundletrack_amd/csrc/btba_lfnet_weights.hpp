// btba_lfnet_weights.hpp -- what turns a checkpoint's host arrays into a device model's float arena, for both LF-Net nets
// (btba_api_lfnet.hip, btba_api_lfnet_det.hip): the argument rules of a btba_lfnet_desc_layer record (include/btba.h), the fold of
// bias and batch norm into (scale, shift), and the arena's layout.  Internal, and free of HIP: only btba.h and the standard library.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstring>
#include <vector>

#include "../../include/btba.h"

namespace btba_host __attribute__((visibility("hidden"))) {

inline bool lfnet_all_finite(const float *a, size_t n)
{
    for (size_t i = 0; i < n; i++)
        if (!std::isfinite(a[i])) return false;
    return true;
}

// a [K][N] convolution or fully connected layer: weights present and finite, biases absent or finite
inline bool lfnet_conv_ok(const btba_lfnet_desc_layer &l, size_t K, size_t N)
{
    return l.weights && lfnet_all_finite(l.weights, K * N) && (!l.biases || lfnet_all_finite(l.biases, N));
}

// the batch-norm arrays of a record: absent, or complete enough and sane
inline bool lfnet_bn_ok(const btba_lfnet_desc_layer &l, size_t N, float eps)
{
    if ((l.moving_mean == nullptr) != (l.moving_variance == nullptr)) return false;
    if (!l.moving_mean) return true;
    if (!lfnet_all_finite(l.moving_mean, N) || !lfnet_all_finite(l.moving_variance, N) || (l.gamma && !lfnet_all_finite(l.gamma, N)) ||
        (l.beta && !lfnet_all_finite(l.beta, N)))
        return false;
    for (size_t n = 0; n < N; n++)
        if (!((double)l.moving_variance[n] + (double)eps > 0.0)) return false;
    return true;
}

// (scale, shift) of y = x * scale + shift for the batch norm of `bn` behind a bias (bias NULL: none), fp64 rounded once
inline void lfnet_fold(const btba_lfnet_desc_layer &bn, const float *bias, int N, float eps, float *scale, float *shift)
{
    for (int n = 0; n < N; n++) {
        const double b = bias ? (double)bias[n] : 0.0;
        double sc = 1.0, sh = b;
        if (bn.moving_mean) {
            sc = (bn.gamma ? (double)bn.gamma[n] : 1.0) / std::sqrt((double)bn.moving_variance[n] + (double)eps);
            sh = (bn.beta ? (double)bn.beta[n] : 0.0) + (b - (double)bn.moving_mean[n]) * sc;
        }
        scale[n] = (float)sc;
        shift[n] = (float)sh;
    }
}

// A model's device floats, laid out on the host first.  take() every region (each starts on 64 floats = 256 bytes: 16-byte loads of
// weight rows), then fill(): zeros of the total size, into which put() and lfnet_fold write.
struct LfnetArena {
    size_t total = 0;
    std::vector<float> host;
    size_t take(size_t n) { const size_t at = total; total += (n + 63) & ~(size_t)63; return at; }
    void fill() { host.assign(total, 0.0f); }
    float *at(size_t off) { return host.data() + off; }
    void put(size_t off, const float *src, size_t n) { std::memcpy(at(off), src, sizeof(float) * n); }
};

}  // namespace btba_host
