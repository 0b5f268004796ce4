// btba_vos_net.hpp -- the VOS backbone's kernels (btba_vos_features; include/btba.h; the plan: btba_vos_net_plan.hpp)
//   ResNet.forward, Bottleneck, BasicBlock   transductive-vos.pytorch/modeling/backbone/resnet.py:36-52, 71-91, 136-145
//   VOSNet.forward                           transductive-vos.pytorch/modeling/network.py:41-50
// rgb [n][3][H][W] -> k_vos_stem -> k_vos_pool -> k_vos_conv per convolution of the plan -> features [n][256][Hd][Wd].  Activations
// are NHWC in between; every batch norm is a (scale, shift) pair folded on the host.
//
// k_vos_stem   C_in = 3, K = 147: too thin for the matrix cores.  One thread per (frame, output position, four output channels): 147
//              fmaf in (ky, kx, c_in) order on the planar input, a tap outside the image is 0; scale, shift, relu; one 16-byte store.
// k_vos_pool   3 x 3, stride 2, pad 1 on NHWC: one thread per (frame, output position, four channels); padding never wins.
// k_vos_conv   out[m][n] = [relu](scale[n] * sum_k A[m][k] W[k][n] + shift[n] [+ res[m][n]]) on v_mfma_f32_32x32x2_f32, built as
//              k_desc_gemm (btba_lfnet_desc.hpp) is.  M = frames x output positions flat, so a tile may straddle frames; N = C_out;
//              K = ks * ks * C_in in (ky, kx, c_in) order.  A is never materialised: sixteen consecutive k are sixteen consecutive
//              channels of ONE input pixel (C_in is a multiple of 16), read as 16-byte pieces from the NHWC activations, zero where
//              the convolution pads.  grid (ceil(M / 64), N / 64), 256 threads = 2 x 2 waves of one 32 x 32 accumulator each.  K is
//              walked in stages of 16: the next stage's A and B pieces are loaded to registers while the eight MFMAs of the current
//              one run from LDS, then stored to the other LDS buffer; one barrier per stage.  LDS 16.5 KB.
//              Every output element is ONE chain over k = 0 .. K - 1 in that order, wherever its row lies: no split of K.
//              The lane that holds an accumulator element reads its residual and writes its output, so a residual may be the
//              output buffer itself.  The last convolution stores NCHW.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/btba.h"

namespace btba {

constexpr int kVosBM = 64, kVosBN = 64, kVosKT = 16;
constexpr int kVosAStride = kVosBM + 4;          // [k][row] image of the A tile: the four k-quads of a row land in four different bank groups

typedef float vos_f32x16 __attribute__((ext_vector_type(16)));

struct VosStem {
    const float *rgb;                            // [n][3][H][W]
    const float *w, *scale, *shift;              // [147][64], [64], [64]
    float *out;                                  // [n][Ho][Wo][64]
    int H, W, Ho, Wo;
    long long threads;                           // n * Ho * Wo * 16
};

__global__ void __launch_bounds__(256) k_vos_stem(const VosStem G)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= G.threads) return;
    const int c = (int)(idx & 15) * 4;
    const long long pos = idx >> 4;
    const int ox = (int)(pos % G.Wo), oy = (int)((pos / G.Wo) % G.Ho);
    const long long f = pos / ((long long)G.Wo * G.Ho);
    const size_t plane = (size_t)G.H * G.W;
    const float *__restrict__ img = G.rgb + (size_t)f * 3 * plane;
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll 1                                  // rolled: unrolled, the 147 weight loads are hoisted and spill
    for (int ky = 0; ky < 7; ky++) {
        const int iy = 2 * oy + ky - 3;
        const bool row = iy >= 0 && iy < G.H;
#pragma unroll 1
        for (int kx = 0; kx < 7; kx++) {
            const int ix = 2 * ox + kx - 3;
            const bool in = row && ix >= 0 && ix < G.W;
            const size_t at = in ? (size_t)iy * G.W + ix : 0;
#pragma unroll
            for (int ch = 0; ch < 3; ch++) {
                const float x = in ? img[ch * plane + at] : 0.0f;
                const float4 w = *reinterpret_cast<const float4 *>(G.w + ((ky * 7 + kx) * 3 + ch) * 64 + c);
                acc.x = fmaf(x, w.x, acc.x); acc.y = fmaf(x, w.y, acc.y); acc.z = fmaf(x, w.z, acc.z); acc.w = fmaf(x, w.w, acc.w);
            }
        }
    }
    const float4 sc = *reinterpret_cast<const float4 *>(G.scale + c), sh = *reinterpret_cast<const float4 *>(G.shift + c);
    float4 o;
    o.x = fmaxf(fmaf(acc.x, sc.x, sh.x), 0.0f); o.y = fmaxf(fmaf(acc.y, sc.y, sh.y), 0.0f);
    o.z = fmaxf(fmaf(acc.z, sc.z, sh.z), 0.0f); o.w = fmaxf(fmaf(acc.w, sc.w, sh.w), 0.0f);
    *reinterpret_cast<float4 *>(G.out + (size_t)pos * 64 + c) = o;
}

struct VosPool {
    const float *in;                             // [n][Hi][Wi][64]
    float *out;                                  // [n][Ho][Wo][64]
    int Hi, Wi, Ho, Wo;
    long long threads;                           // n * Ho * Wo * 16
};

__global__ void __launch_bounds__(256) k_vos_pool(const VosPool G)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= G.threads) return;
    const int c = (int)(idx & 15) * 4;
    const long long pos = idx >> 4;
    const int ox = (int)(pos % G.Wo), oy = (int)((pos / G.Wo) % G.Ho);
    const long long f = pos / ((long long)G.Wo * G.Ho);
    const float *__restrict__ img = G.in + (size_t)f * G.Hi * G.Wi * 64;
    const float ninf = -__builtin_huge_valf();
    float4 m = make_float4(ninf, ninf, ninf, ninf);
#pragma unroll
    for (int ky = 0; ky < 3; ky++) {
#pragma unroll
        for (int kx = 0; kx < 3; kx++) {
            const int iy = 2 * oy + ky - 1, ix = 2 * ox + kx - 1;
            if (iy < 0 || iy >= G.Hi || ix < 0 || ix >= G.Wi) continue;
            const float4 v = *reinterpret_cast<const float4 *>(img + ((size_t)iy * G.Wi + ix) * 64 + c);
            m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w);
        }
    }
    *reinterpret_cast<float4 *>(G.out + (size_t)pos * 64 + c) = m;
}

struct VosConv {
    const float *in;                             // NHWC [n][Hi][Wi][Cin]
    const float *w, *scale, *shift;              // [K][N], [N], [N]
    const float *res;                            // NULL or NHWC [M][N]; may be `out`
    float *out;                                  // NHWC [M][N], or with nchw [n][N][Ho * Wo]
    int M, N, K, Hi, Wi, Cin, Ho, Wo, ks, stride, pad, relu, nchw;
};

__global__ void __launch_bounds__(256) k_vos_conv(const VosConv G)
{
    __shared__ __attribute__((aligned(16))) float As[2][kVosKT][kVosAStride];
    __shared__ __attribute__((aligned(16))) float Bs[2][kVosKT][kVosBN];
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, h = lane >> 5, j = lane & 31;
    const int m0 = blockIdx.x * kVosBM, n0 = blockIdx.y * kVosBN, pos = G.Ho * G.Wo;

    // this thread's piece of the A tile: row ar, channels 4 aq .. 4 aq + 3 of the stage's sixteen
    const int ar = tid >> 2, aq = tid & 3, am = m0 + ar;
    const int af = am / pos, arem = am - af * pos, aoy = arem / G.Wo, aox = arem - aoy * G.Wo;
    const bool a_row = am < G.M;
    const int iy0 = G.stride * aoy - G.pad, ix0 = G.stride * aox - G.pad;
    const float *__restrict__ a_img = G.in + (size_t)af * G.Hi * G.Wi * G.Cin;
    // ... and of the B tile: row bk, columns bn .. bn + 3 (N is a multiple of 64)
    const int bk = tid >> 4, bn = (tid & 15) * 4;
    const float *__restrict__ b_ptr = G.w + (size_t)bk * G.N + n0 + bn;

    auto load_a = [&](int k0) {
        const int tap = k0 / G.Cin, c = k0 - tap * G.Cin + 4 * aq, ky = tap / G.ks, kx = tap - ky * G.ks;
        const int iy = iy0 + ky, ix = ix0 + kx;
        if (!a_row || iy < 0 || iy >= G.Hi || ix < 0 || ix >= G.Wi) return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return *reinterpret_cast<const float4 *>(a_img + ((size_t)iy * G.Wi + ix) * G.Cin + c);
    };
    auto load_b = [&](int k0) { return *reinterpret_cast<const float4 *>(b_ptr + (size_t)k0 * G.N); };
    auto store = [&](int buf, const float4 &a, const float4 &b) {
        As[buf][4 * aq + 0][ar] = a.x; As[buf][4 * aq + 1][ar] = a.y; As[buf][4 * aq + 2][ar] = a.z; As[buf][4 * aq + 3][ar] = a.w;
        *reinterpret_cast<float4 *>(&Bs[buf][bk][bn]) = b;
    };

    vos_f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; r++) acc[r] = 0.0f;
    const int wm = (wv & 1) * 32, wn = (wv >> 1) * 32, stages = G.K / kVosKT;
    store(0, load_a(0), load_b(0));
    __syncthreads();
    for (int t = 0; t < stages; t++) {
        const int buf = t & 1;
        float4 a_nxt = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b_nxt = a_nxt;
        if (t + 1 < stages) { a_nxt = load_a((t + 1) * kVosKT); b_nxt = load_b((t + 1) * kVosKT); }
#pragma unroll
        for (int s = 0; s < kVosKT / 2; s++)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[buf][2 * s + h][wm + j], Bs[buf][2 * s + h][wn + j], acc, 0, 0, 0);
        if (t + 1 < stages) store(buf ^ 1, a_nxt, b_nxt);      // last read before the barrier that ended stage t - 1
        __syncthreads();
    }

    const int n = n0 + wn + j;
    const float sc = G.scale[n], sh = G.shift[n];
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int m = m0 + wm + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (m >= G.M) continue;
        float v = fmaf(acc[r], sc, sh);
        if (G.res) v += G.res[(size_t)m * G.N + n];
        if (G.relu) v = fmaxf(v, 0.0f);
        if (G.nchw) {
            const int f = m / pos;
            G.out[((size_t)f * G.N + n) * pos + (m - f * pos)] = v;
        } else {
            G.out[(size_t)m * G.N + n] = v;
        }
    }
}

}  // namespace btba
