// btba_lfnet_det.hpp -- LF-Net's detector net (btba_lfnet_det_*, btba_lfnet_scores; include/btba.h)
//   get_model, building_block    lf-net-release/models/mso_resnet_detector.py:10-173
//   conv2d_fixed_padding, conv2d_custom, tf_batch_norm_act    lf-net-release/common/tf_layer_utils.py:167-199, 228-402
// photo [H][W] -> init_conv (k_det_init) -> blocks x (conv1, conv2) (k_det_conv) -> per scale the score map, and the orientation map
// (k_det_head).  Activations are NHWC fp32 in two workspace buffers: x (the residual stream) and t (conv1's output).
//
// k_det_init   C_in = 1: too thin for the matrix cores.  One thread per (pixel, four output channels): k * k fmaf in (ky, kx) order,
//              the bias, one 16-byte store.
// k_det_conv   out = act(scale * conv(in') + shift) [+ shortcut], C -> C, on v_mfma_f32_16x16x4_f32.  An implicit GEMM with M = pixels,
//              N = C, K = k * k * C in (ky, kx, c_in) order and no im2col buffer: a workgroup of 4 waves owns a 16 x 16 pixel tile; the
//              tile and its k / 2 halo lie in LDS as [y][x][C + 4] (the pad of 4 floats puts the 16 pixels x 4 channels of an A
//              fragment into 64 different banks), written once with pre-bn and the activation applied (in' = act(in * s + b)) and
//              zeros for the taps outside the image AFTER that.  A wave owns 4 rows of 16 pixels = 4 M tiles and all C / 16 N tiles:
//              4 C / 16 independent accumulators of 4 registers, which covers the instruction's 40-cycle dependent latency at its
//              32-cycle issue.  An A fragment is one LDS dword per lane (pixel = lane & 15, k = lane >> 4), a B fragment one global
//              dword per lane from the [K][C] weights (TensorFlow's [k][k][C][C] read flat; 256 contiguous bytes per wave, served
//              from L1 / L2 for every workgroup alike) and feeds 4 MFMAs.  N = 16 is the instruction's own width: the 64 x 64 tile
//              of k_desc_gemm would idle three quarters of its B tile here.
//              Every output element is ONE chain over k = 0 .. k * k * C - 1 in that order: no split of K, nothing that depends
//              on where the pixel lies in the grid, the batch or the pass.  The epilogue applies the folded mid-bn and activation
//              (conv1) or the bias and the shortcut (conv2, which may write over the shortcut's buffer: every element is read and
//              written by the same lane).
// k_det_head   the thin ends, C -> NO (1: a score map, 2: the orientation map) on the vector ALU.  A workgroup owns a 16 x 16 tile
//              of the OUTPUT map; the staging pass computes f = act(fin-bn(x)) and, where the map is not the photo's size, TF1's
//              bilinear resize of f, straight into the LDS tile (so neither f nor a resized copy of it is ever written out), zeros
//              outside the map.  One thread per output pixel: fmaf over (ky, kx, c) in order against scalar-loaded weights; the
//              bias; for the orientation x * (1 / sqrt(max(x0^2 + x1^2, 1e-12))).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/btba.h"
#include "btba_lfnet_net.hpp"

namespace btba {

constexpr int kDetTile = 16;

typedef float det_f32x4 __attribute__((ext_vector_type(4)));

__host__ __device__ inline int det_lds_floats(int C, int ks) { const int r = kDetTile + 2 * (ks / 2); return r * r * (C + 4); }

struct DetInit {
    const float *photo;                          // [frames][H][W]
    const float *w, *bias;                       // [k * k][C], [C]
    float *out;                                  // NHWC [frames][H][W][C]
    int H, W, C, ks;
    long long threads;                           // frames * H * W * C / 4
};

__global__ void __launch_bounds__(256) k_det_init(const DetInit G)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= G.threads) return;
    const int quads = G.C >> 2, c = (int)(idx % quads) * 4, h = G.ks / 2;
    const long long pix = idx / quads;
    const int x = (int)(pix % G.W), y = (int)((pix / G.W) % G.H);
    const float *__restrict__ img = G.photo + (pix - ((long long)y * G.W + x));
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (int ky = 0; ky < G.ks; ky++)
        for (int kx = 0; kx < G.ks; kx++) {
            const int iy = y + ky - h, ix = x + kx - h;
            const float v = (iy >= 0 && iy < G.H && ix >= 0 && ix < G.W) ? img[(size_t)iy * G.W + ix] : 0.0f;
            const float4 w = *reinterpret_cast<const float4 *>(G.w + (ky * G.ks + kx) * G.C + c);
            acc.x = fmaf(v, w.x, acc.x); acc.y = fmaf(v, w.y, acc.y); acc.z = fmaf(v, w.z, acc.z); acc.w = fmaf(v, w.w, acc.w);
        }
    const float4 b = *reinterpret_cast<const float4 *>(G.bias + c);
    *reinterpret_cast<float4 *>(G.out + (size_t)pix * G.C + c) = make_float4(acc.x + b.x, acc.y + b.y, acc.z + b.z, acc.w + b.w);
}

struct DetConv {
    const float *in;                             // NHWC [frames][H][W][C]
    const float *w;                              // [k * k * C][C]
    const float *in_scale, *in_shift;            // [C]: pre-bn, applied with the activation while the tile is staged; NULL: the input as it is
    const float *scale, *shift;                  // [C]: the epilogue's
    const float *shortcut;                       // NHWC like out, or NULL
    float *out;
    int H, W, tiles_x, tiles_y, act, out_act;
    float alpha;
};

// grid: frames * tiles_y * tiles_x, 256 threads, det_lds_floats(16 NT, KS) floats of dynamic LDS
template <int NT, int KS>
__global__ void __launch_bounds__(256) k_det_conv(const DetConv G)
{
    extern __shared__ __attribute__((aligned(16))) float det_lds[];
    constexpr int C = 16 * NT, HALO = KS / 2, R = kDetTile + 2 * HALO, PS = C + 4, Q = C / 4;
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, lx = lane & 15, lk = lane >> 4;
    int b = blockIdx.x;
    const int tx = b % G.tiles_x; b /= G.tiles_x;
    const int ty = b % G.tiles_y, f = b / G.tiles_y;
    const int x0 = tx * kDetTile, y0 = ty * kDetTile;
    const size_t frame = (size_t)f * G.H * G.W;
    const float *__restrict__ img = G.in + frame * C;

    for (int i = tid; i < R * R * Q; i += 256) {
        const int q = i % Q, p = i / Q, gy = y0 + p / R - HALO, gx = x0 + p % R - HALO;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (gy >= 0 && gy < G.H && gx >= 0 && gx < G.W) {
            v = *reinterpret_cast<const float4 *>(img + ((size_t)gy * G.W + gx) * C + 4 * q);
            if (G.in_scale) v = lfnet_bn_act4(v, G.in_scale, G.in_shift, 4 * q, G.act, G.alpha);
        }
        *reinterpret_cast<float4 *>(det_lds + p * PS + 4 * q) = v;
    }
    __syncthreads();

    det_f32x4 acc[4][NT];
#pragma unroll
    for (int mt = 0; mt < 4; mt++)
#pragma unroll
        for (int nt = 0; nt < NT; nt++) acc[mt][nt] = det_f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };
    const float *__restrict__ wlane = G.w + (size_t)lk * C + lx;
    for (int ky = 0; ky < KS; ky++)
        for (int kx = 0; kx < KS; kx++) {
            const float *a_tap = det_lds + ((wv * 4 + ky) * R + lx + kx) * PS + lk;
            const float *__restrict__ w_tap = wlane + (size_t)(ky * KS + kx) * C * C;
#pragma unroll
            for (int c4 = 0; c4 < Q; c4++) {
                float bv[NT];
#pragma unroll
                for (int nt = 0; nt < NT; nt++) bv[nt] = w_tap[c4 * 4 * C + nt * 16];
#pragma unroll
                for (int mt = 0; mt < 4; mt++) {
                    const float a = a_tap[mt * R * PS + c4 * 4];
#pragma unroll
                    for (int nt = 0; nt < NT; nt++) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv[nt], acc[mt][nt], 0, 0, 0);
                }
            }
        }

    // C/D: column (channel) lane & 15, row (pixel of the M tile) 4 (lane >> 4) + register
#pragma unroll
    for (int mt = 0; mt < 4; mt++) {
        const int gy = y0 + wv * 4 + mt;
        if (gy >= G.H) continue;
#pragma unroll
        for (int nt = 0; nt < NT; nt++) {
            const int n = nt * 16 + lx;
            const float sc = G.scale[n], sh = G.shift[n];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int gx = x0 + lk * 4 + r;
                if (gx >= G.W) continue;
                const size_t o = (frame + (size_t)gy * G.W + gx) * C + n;
                float v = lfnet_act(fmaf(acc[mt][nt][r], sc, sh), G.out_act, G.alpha);
                if (G.shortcut) v += G.shortcut[o];
                G.out[o] = v;
            }
        }
    }
}

struct DetHead {
    const float *x;                              // NHWC [frames][H][W][C]
    const float *fscale, *fshift;                // [C]: fin-bn
    const float *w;                              // [k * k * C][NO]
    float *out;                                  // [frames][h][w][NO]
    float bias0, bias1;
    int H, W, h, w_out, C, ks, tiles_x, tiles_y, act;
    float alpha;
};

// grid: frames * tiles_y * tiles_x over the OUTPUT map, 256 threads, det_lds_floats(C, ks) floats of dynamic LDS
template <int NO>
__global__ void __launch_bounds__(256) k_det_head(const DetHead G)
{
    extern __shared__ __attribute__((aligned(16))) float det_lds[];
    const int C = G.C, halo = G.ks / 2, R = kDetTile + 2 * halo, PS = C + 4, Q = C >> 2, tid = threadIdx.x;
    int b = blockIdx.x;
    const int tx = b % G.tiles_x; b /= G.tiles_x;
    const int ty = b % G.tiles_y, f = b / G.tiles_y;
    const int x0 = tx * kDetTile, y0 = ty * kDetTile;
    const float *__restrict__ img = G.x + (size_t)f * G.H * G.W * C;
    const bool same = G.h == G.H && G.w_out == G.W;
    const float ry = (float)G.H / (float)G.h, rx = (float)G.W / (float)G.w_out;

    for (int i = tid; i < R * R * Q; i += 256) {
        const int q = i % Q, p = i / Q, my = y0 + p / R - halo, mx = x0 + p % R - halo, c = 4 * q;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (my >= 0 && my < G.h && mx >= 0 && mx < G.w_out) {
            auto feat = [&](int yy, int xx) {
                return lfnet_bn_act4(*reinterpret_cast<const float4 *>(img + ((size_t)yy * G.W + xx) * C + c), G.fscale, G.fshift, c, G.act, G.alpha);
            };
            if (same) {
                v = feat(my, mx);
            } else {
                const float sy = (float)my * ry, sx = (float)mx * rx;
                const int ya = min((int)floorf(sy), G.H - 1), xa = min((int)floorf(sx), G.W - 1);
                const int yb = min(ya + 1, G.H - 1), xb = min(xa + 1, G.W - 1);
                const float fy = sy - (float)ya, fx = sx - (float)xa;
                const float4 tl = feat(ya, xa), tr = feat(ya, xb), bl = feat(yb, xa), br = feat(yb, xb);
                const float4 top = make_float4(tl.x + (tr.x - tl.x) * fx, tl.y + (tr.y - tl.y) * fx, tl.z + (tr.z - tl.z) * fx, tl.w + (tr.w - tl.w) * fx);
                const float4 bot = make_float4(bl.x + (br.x - bl.x) * fx, bl.y + (br.y - bl.y) * fx, bl.z + (br.z - bl.z) * fx, bl.w + (br.w - bl.w) * fx);
                v = make_float4(top.x + (bot.x - top.x) * fy, top.y + (bot.y - top.y) * fy, top.z + (bot.z - top.z) * fy, top.w + (bot.w - top.w) * fy);
            }
        }
        *reinterpret_cast<float4 *>(det_lds + p * PS + c) = v;
    }
    __syncthreads();

    const int px = tid & 15, py = tid >> 4, my = y0 + py, mx = x0 + px;
    if (my >= G.h || mx >= G.w_out) return;
    const float *__restrict__ w = G.w;
    float a0 = 0.0f, a1 = 0.0f;
    for (int ky = 0; ky < G.ks; ky++)
        for (int kx = 0; kx < G.ks; kx++) {
            const float *a_tap = det_lds + ((py + ky) * R + px + kx) * PS;
            const float *__restrict__ w_tap = w + (size_t)(ky * G.ks + kx) * C * NO;
            for (int c = 0; c < C; c += 4) {
                const float4 a = *reinterpret_cast<const float4 *>(a_tap + c);
                if (NO == 1) {
                    a0 = fmaf(a.x, w_tap[c], a0); a0 = fmaf(a.y, w_tap[c + 1], a0); a0 = fmaf(a.z, w_tap[c + 2], a0); a0 = fmaf(a.w, w_tap[c + 3], a0);
                } else {
                    a0 = fmaf(a.x, w_tap[2 * c], a0); a1 = fmaf(a.x, w_tap[2 * c + 1], a1);
                    a0 = fmaf(a.y, w_tap[2 * c + 2], a0); a1 = fmaf(a.y, w_tap[2 * c + 3], a1);
                    a0 = fmaf(a.z, w_tap[2 * c + 4], a0); a1 = fmaf(a.z, w_tap[2 * c + 5], a1);
                    a0 = fmaf(a.w, w_tap[2 * c + 6], a0); a1 = fmaf(a.w, w_tap[2 * c + 7], a1);
                }
            }
        }
    const size_t o = ((size_t)f * G.h + my) * G.w_out + mx;
    if (NO == 1) {
        G.out[o] = a0 + G.bias0;
    } else {
        const float u = a0 + G.bias0, v = a1 + G.bias1;
        const float inv = 1.0f / sqrtf(fmaxf(fmaf(v, v, u * u), 1e-12f));
        G.out[2 * o] = u * inv;                  // ori_dev is only known to be aligned to 4 bytes
        G.out[2 * o + 1] = v * inv;
    }
}

}  // namespace btba
