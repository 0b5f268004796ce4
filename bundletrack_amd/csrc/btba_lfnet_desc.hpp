// btba_lfnet_desc.hpp -- LF-Net's descriptor net (btba_lfnet_desc_*, btba_lfnet_descriptors; include/btba.h)
//   get_model               lf-net-release/models/simple_desc.py:10-91
//   conv2d, fully_connected lf-net-release/common/tf_layer_utils.py:228-286, 405-434
//   tf_batch_norm_act       lf-net-release/common/tf_layer_utils.py:167-199   (inference: folded into scale, shift on the host)
// Patches [P][P] -> conv1 (k_desc_conv1) -> conv2 .. convL, fc1, fc2 (k_desc_gemm) -> l2_normalize (k_desc_finish).
//
// k_desc_conv1   C_in = 1, K = 9: too thin for the matrix cores.  One thread per (patch, output position, four output channels): nine
//                fmaf in (ky, kx) order, the folded batch norm, the activation, one 16-byte store into the NHWC output.
// k_desc_gemm    out[m][n] = act(scale[n] * sum_k A[m][k] W[k][n] + shift[n]) on v_mfma_f32_32x32x2_f32.  M = patches x output
//                positions, N = C_out, K = ks * ks * C_in in (ky, kx, c_in) order; a fully connected layer is the same kernel with a
//                1 x 1 "image" and ks = 1.  A is never materialised: a row of A is an output position, and sixteen consecutive k are
//                sixteen consecutive channels of ONE input pixel (C_in is a multiple of 16), read as 16-byte pieces straight from the
//                NHWC activations of the layer before, zero where TensorFlow's SAME rule pads.  W lies [K][N], which is TensorFlow's
//                own [3][3][C_in][C_out]: a B fragment is two 128-byte rows.
//                grid (ceil(M / 64), ceil(N / 64)), 256 threads = 2 x 2 waves of one 32 x 32 accumulator each (the instruction's
//                issue interval equals its dependent latency, so one accumulator per wave keeps the pipe full).  K is walked in stages
//                of 16: the next stage's A and B pieces are loaded to registers while the eight MFMAs of the current one run from LDS,
//                then stored to the other LDS buffer; one barrier per stage.  LDS: 2 x (16 x 68 + 16 x 64) x 4 = 16.5 KB; 30 VGPRs + 16 AGPRs.
//                Every output element is ONE chain over k = 0 .. K - 1 in that order, wherever its row lies in the grid: no split of K.
//                A tile whose rows all belong to slots past their frame's count returns at once; rows past the count inside a live tile
//                read zeros.
// k_desc_finish  one wave per descriptor: sum of squares (lane-strided, then a butterfly: an order fixed by out_dim), x * (1 / sqrt(max(
//                sum, 1e-12))) or the plain copy; zeros into the slots past the count.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/btba.h"
#include "btba_lfnet_net.hpp"

namespace btba {

constexpr int kDescBM = 64, kDescBN = 64, kDescKT = 16;
constexpr int kDescAStride = kDescBM + 4;        // [k][row] image of the A tile: the four k-quads of a row land in four different bank groups
constexpr int kDescChunk = 2048;                 // patches per pass over the layers: bounds the scratch (two buffers of the widest layer)

typedef float desc_f32x16 __attribute__((ext_vector_type(16)));

// slot (g mod slots) of frame (g / slots) holds a patch
__device__ inline bool desc_live(const int32_t *__restrict__ n_kpts, int slots, int g)
{
    if (!n_kpts) return true;
    const int f = g / slots;
    return g - f * slots < n_kpts[f];
}

struct DescConv1 {
    const float *patches;                        // [n_patches][P][P]
    const float *w, *scale, *shift;              // [9][C], [C], [C]
    float *out;                                  // [n_patches][Ho][Ho][C]
    const int32_t *n_kpts;
    int n_patches, P, Ho, pad, C, act, slots, patch0;
    float alpha;
};

__global__ void __launch_bounds__(256) k_desc_conv1(const DescConv1 G)
{
    const int quads = G.C >> 2;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= G.n_patches * G.Ho * G.Ho * quads) return;
    const int c = (idx % quads) * 4, pos = idx / quads, ox = pos % G.Ho, oy = (pos / G.Ho) % G.Ho, p = pos / (G.Ho * G.Ho);
    if (!desc_live(G.n_kpts, G.slots, G.patch0 + p)) return;
    const float *__restrict__ img = G.patches + (size_t)p * G.P * G.P;
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
    for (int ky = 0; ky < 3; ky++) {
#pragma unroll
        for (int kx = 0; kx < 3; kx++) {
            const int iy = 2 * oy + ky - G.pad, ix = 2 * ox + kx - G.pad;
            const float x = (iy >= 0 && iy < G.P && ix >= 0 && ix < G.P) ? img[iy * G.P + ix] : 0.0f;
            const float4 w = *reinterpret_cast<const float4 *>(G.w + (ky * 3 + kx) * G.C + c);
            acc.x = fmaf(x, w.x, acc.x); acc.y = fmaf(x, w.y, acc.y); acc.z = fmaf(x, w.z, acc.z); acc.w = fmaf(x, w.w, acc.w);
        }
    }
    *reinterpret_cast<float4 *>(G.out + (size_t)pos * G.C + c) = lfnet_bn_act4(acc, G.scale, G.shift, c, G.act, G.alpha);
}

struct DescGemm {
    const float *in;                             // NHWC [patches][Hi][Wi][Cin]  (fully connected: Hi = Wi = 1, Cin = K)
    const float *w, *scale, *shift;              // [K][N], [N], [N]
    float *out;                                  // [M][N] = NHWC [patches][Ho][Wo][N]
    const int32_t *n_kpts;
    int M, N, K, Hi, Wi, Cin, Ho, Wo, ks, pad, act, slots, patch0;
    float alpha;
};

__global__ void __launch_bounds__(256) k_desc_gemm(const DescGemm G)
{
    __shared__ __attribute__((aligned(16))) float As[2][kDescKT][kDescAStride];
    __shared__ __attribute__((aligned(16))) float Bs[2][kDescKT][kDescBN];
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, h = lane >> 5, j = lane & 31;
    const int m0 = blockIdx.x * kDescBM, n0 = blockIdx.y * kDescBN, pos = G.Ho * G.Wo;

    // this thread's piece of the A tile: row ar, channels 4 aq .. 4 aq + 3 of the stage's sixteen
    const int ar = tid >> 2, aq = tid & 3, am = m0 + ar;
    const int ap = am / pos, arem = am - ap * pos, aoy = arem / G.Wo, aox = arem - aoy * G.Wo;
    const bool a_row = am < G.M && desc_live(G.n_kpts, G.slots, G.patch0 + ap);
    if (G.n_kpts && !__syncthreads_or(a_row)) return;            // every row of the tile lies past its frame's count
    const int iy0 = 2 * aoy - G.pad, ix0 = 2 * aox - G.pad;
    const float *__restrict__ a_img = G.in + (size_t)ap * G.Hi * G.Wi * G.Cin;
    // ... and of the B tile: row bk, columns bn .. bn + 3
    const int bk = tid >> 4, bn = (tid & 15) * 4;
    const bool b_col = n0 + bn < G.N;                            // N is a multiple of 16
    const float *__restrict__ b_ptr = G.w + (size_t)bk * G.N + n0 + bn;

    auto load_a = [&](int k0) {
        const int tap = k0 / G.Cin, c = k0 - tap * G.Cin + 4 * aq, ky = tap / G.ks, kx = tap - ky * G.ks;
        const int iy = iy0 + ky, ix = ix0 + kx;
        if (!a_row || iy < 0 || iy >= G.Hi || ix < 0 || ix >= G.Wi) return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return *reinterpret_cast<const float4 *>(a_img + ((size_t)iy * G.Wi + ix) * G.Cin + c);
    };
    auto load_b = [&](int k0) {
        return b_col ? *reinterpret_cast<const float4 *>(b_ptr + (size_t)k0 * G.N) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    };
    auto store = [&](int buf, const float4 &a, const float4 &b) {
        As[buf][4 * aq + 0][ar] = a.x; As[buf][4 * aq + 1][ar] = a.y; As[buf][4 * aq + 2][ar] = a.z; As[buf][4 * aq + 3][ar] = a.w;
        *reinterpret_cast<float4 *>(&Bs[buf][bk][bn]) = b;
    };

    desc_f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; r++) acc[r] = 0.0f;
    const int wm = (wv & 1) * 32, wn = (wv >> 1) * 32, stages = G.K / kDescKT;
    store(0, load_a(0), load_b(0));
    __syncthreads();
    for (int t = 0; t < stages; t++) {
        const int buf = t & 1;
        float4 a_nxt = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b_nxt = a_nxt;
        if (t + 1 < stages) { a_nxt = load_a((t + 1) * kDescKT); b_nxt = load_b((t + 1) * kDescKT); }
#pragma unroll
        for (int s = 0; s < kDescKT / 2; s++)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[buf][2 * s + h][wm + j], Bs[buf][2 * s + h][wn + j], acc, 0, 0, 0);
        if (t + 1 < stages) store(buf ^ 1, a_nxt, b_nxt);      // last read before the barrier that ended stage t - 1
        __syncthreads();
    }

    const int n = n0 + wn + j;
    if (n >= G.N) return;
    const float sc = G.scale[n], sh = G.shift[n];
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int m = m0 + wm + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (m < G.M) G.out[(size_t)m * G.N + n] = lfnet_act(fmaf(acc[r], sc, sh), G.act, G.alpha);
    }
}

// grid ceil(M / 4), 256 threads: wave w of a workgroup owns descriptor 4 blockIdx.x + w
__global__ void __launch_bounds__(256) k_desc_finish(const float *__restrict__ raw, float *__restrict__ out, const int32_t *__restrict__ n_kpts,
                                                     int M, int D, int l2, int slots, int patch0)
{
    const int m = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (m >= M) return;
    const float *__restrict__ x = raw + (size_t)m * D;
    float *__restrict__ o = out + (size_t)m * D;
    if (!desc_live(n_kpts, slots, patch0 + m)) {
        for (int n = lane; n < D; n += 64) o[n] = 0.0f;
        return;
    }
    float inv = 1.0f;
    if (l2) {
        float ss = 0.0f;
        for (int n = lane; n < D; n += 64) ss = fmaf(x[n], x[n], ss);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) ss += __shfl_xor(ss, d);
        inv = 1.0f / sqrtf(fmaxf(ss, 1e-12f));
    }
    for (int n = lane; n < D; n += 64) o[n] = x[n] * inv;
}

}  // namespace btba
