// btba_vos.hpp -- mask propagation of the tracker's video segmentation (btba_vos_*, include/btba.h)
//   predict                 transductive-vos.pytorch/lib/predict.py:11-59   (k_vos_partial + k_vos_merge)
//   prepare_first_frame     run_video.py:68-82                               (k_vos_first_labels)
//   the mask of a frame     run_video.py:151-155                             (k_vos_masks)
//   rgb_normalize           run_video.py:81,113-114                          (k_vos_inputs)
// predict is an attention with a multiplicative bias applied after the softmax: for a target position q and a key k = (reference r,
// position p)   pred[c,q] = sum_k label_r[c,p] * softmax_k(temperature * <ref_r[:,p], tgt[:,q]>) * exp(-|p - q|^2 / sigma(r)^2).
// Neither the [n_ref*HW][HW] similarity matrix nor the [HW][HW] weight tables exist here.
//
// k_vos_partial    grid (ceil(HW / QT), splits, items of a chunk), 512 threads = 8 waves.  A workgroup owns QT = 32 * NQ target
//                  positions (NQ = 4 up to C = 256, 2 above: the target tile [C][QT] stays in LDS, at most 128 KB) and one split of the
//                  item's key tiles (32 positions of ONE reference each; the last tile of a reference may be partial).  Wave w walks the
//                  split's tiles w, w + 8, ...:
//                    S^T (32 keys x 32 targets) = v_mfma_f32_32x32x2_f32 over the channels, A = the reference's features straight from
//                    global memory (lane l: channel 2 s + (l >> 5), key l & 31: two 128-byte rows per load, prefetched two groups of four
//                    steps ahead), B = the target tile from LDS.  The result has the target on the lane and 16 keys in registers, so the
//                    running maximum is 15 v_max and one exchange with lane ^ 32;
//                    e = exp(s - m), the Gaussian from the two positions, and  pred^T += label^T . (e * w)  as 16 more MFMAs whose B
//                    operand is the register the first product left the value in (k = lane >> 5 is the same key split), A = the labels
//                    (lane l: class l & 31, zero from d on).  Rows 0 .. 15 of that accumulator are the classes.
//                  The eight waves' (m, l, acc) are merged through LDS in wave order and written to the split's slot of the scratch.
// k_vos_merge      one thread per (item, target): the splits' partials merged in split order, pred = acc / l, optional one-hot of
//                  the argmax (lowest class on ties).
// Every sum runs in an order fixed by the shapes of the item alone (the number of splits is a function of HW and n_ref), with no
// atomics: the same item gives the same bits in any batch.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/btba.h"

namespace btba {

constexpr int kVosChunk = 4;                     // items per launch: their pointer tables travel as kernel arguments
constexpr int kVosMaxRef = BTBA_VOS_MAX_REF;
constexpr int kVosMaxClasses = BTBA_VOS_MAX_CLASSES;
constexpr int kVosMaxSplits = 16;
constexpr int kVosWaves = 8;                     // waves of a k_vos_partial workgroup
constexpr float kVosNone = -3.0e38f;             // "no key yet": finite, so m - m' never is inf - inf

typedef float vos_f32x16 __attribute__((ext_vector_type(16)));

struct VosItems {
    const float *ref[kVosChunk][kVosMaxRef];
    const float *lab[kVosChunk][kVosMaxRef];
    const float *tgt[kVosChunk];
    float *pred[kVosChunk];
    float *onehot[kVosChunk];                    // NULL = not wanted
    int32_t n_ref[kVosChunk], n_dense[kVosChunk], n_split[kVosChunk];
};

// key tiles of 32 positions per reference, and the number of splits of an item's n_ref * tiles: enough workgroups to fill the
// device once from one item, at least eight tiles (one per wave) per split.  A function of the item's own shape only.
__host__ __device__ inline int vos_tiles_per_ref(int HW) { return (HW + 31) / 32; }
__host__ __device__ inline int vos_splits(int HW, int n_ref, int QT)
{
    const int q_tiles = (HW + QT - 1) / QT, T = n_ref * vos_tiles_per_ref(HW);
    int s = 256 / q_tiles;                                       // one of these workgroups per compute unit (its LDS tile): one round
    if (s > (T + kVosWaves - 1) / kVosWaves) s = (T + kVosWaves - 1) / kVosWaves;
    if (s > kVosMaxSplits) s = kVosMaxSplits;
    return s < 1 ? 1 : s;
}
__host__ __device__ inline size_t vos_part_floats(int HW, int d) { return (size_t)kVosMaxSplits * (2 + d) * HW; }      // per item

// scratch of one item: [split][field][HW], field 0 = m, 1 = l, 2 + c = acc[c]
template <int NQ>
__global__ void __launch_bounds__(64 * kVosWaves) k_vos_partial(const VosItems I, int C, int d, int Hd, int Wd, float temperature, float sd2, float ss2,
                                                     float *__restrict__ part, int item0)
{
    constexpr int QT = 32 * NQ;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int b = blockIdx.z, sp = blockIdx.y, n_split = I.n_split[b];
    if (sp >= n_split) return;                                   // (uniform)
    const int HW = Hd * Wd, q0 = blockIdx.x * QT, tid = threadIdx.x, w = tid >> 6, lane = tid & 63, h = lane >> 5, j = lane & 31;
    const int n_ref = I.n_ref[b], first_dense = n_ref - I.n_dense[b];
    const int Tr = vos_tiles_per_ref(HW), T = n_ref * Tr, tps = (T + n_split - 1) / n_split;
    const int t_begin = sp * tps, t_end = min(T, t_begin + tps);

    const float *__restrict__ tgt = I.tgt[b];
    for (int i = tid; i < C * QT; i += 64 * kVosWaves) {
        const int c = i / QT, q = q0 + (i % QT);
        smem[i] = q < HW ? tgt[(size_t)c * HW + q] : 0.0f;
    }
    __syncthreads();

    float m[NQ], l[NQ];
    vos_f32x16 acc[NQ];
    int qy[NQ], qx[NQ];
#pragma unroll
    for (int n = 0; n < NQ; n++) {
        m[n] = kVosNone; l[n] = 0.0f;
        for (int r = 0; r < 16; r++) acc[n][r] = 0.0f;
        const int q = q0 + 32 * n + j;
        qy[n] = q / Wd; qx[n] = q % Wd;
    }

    const int groups = C >> 3;                                   // four MFMA steps (eight channels) per group
    for (int t = t_begin + w; t < t_end; t += kVosWaves) {
        const int r = t / Tr, p0 = (t - r * Tr) * 32;
        const float *__restrict__ R = I.ref[b][r];
        const float *__restrict__ L = I.lab[b][r];
        const float sigma2 = r >= first_dense ? sd2 : ss2;
        const int pc = min(p0 + j, HW - 1);                       // a partial tile's rows past the reference repeat its last position; masked below
        const float *a_ptr = R + (size_t)h * HW + pc;

        vos_f32x16 s[NQ];
#pragma unroll
        for (int n = 0; n < NQ; n++)
            for (int r2 = 0; r2 < 16; r2++) s[n][r2] = 0.0f;
        float a_cur[4], a_nxt[4] = { 0.0f, 0.0f, 0.0f, 0.0f }, a_far[4] = { 0.0f, 0.0f, 0.0f, 0.0f };      // groups g, g + 1, g + 2
#pragma unroll
        for (int u = 0; u < 4; u++) a_cur[u] = a_ptr[(size_t)(2 * u) * HW];
        if (groups > 1) {
#pragma unroll
            for (int u = 0; u < 4; u++) a_nxt[u] = a_ptr[(size_t)(8 + 2 * u) * HW];
        }
        for (int g = 0; g < groups; g++) {
            if (g + 2 < groups) {
#pragma unroll
                for (int u = 0; u < 4; u++) a_far[u] = a_ptr[(size_t)(8 * (g + 2) + 2 * u) * HW];
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const float *bq = smem + (8 * g + 2 * u + h) * QT + j;
#pragma unroll
                for (int n = 0; n < NQ; n++) s[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur[u], bq[32 * n], s[n], 0, 0, 0);
            }
#pragma unroll
            for (int u = 0; u < 4; u++) { a_cur[u] = a_nxt[u]; a_nxt[u] = a_far[u]; }
        }

        // this lane's 16 keys: rows (reg & 3) + 8 (reg >> 2) + 4 h of the tile
        float lab[16];
        int ky[16], kx[16];
        bool kv[16];
#pragma unroll
        for (int r2 = 0; r2 < 16; r2++) {
            const int kp = p0 + (r2 & 3) + 8 * (r2 >> 2) + 4 * h;
            kv[r2] = kp < HW;
            ky[r2] = kp / Wd; kx[r2] = kp - ky[r2] * Wd;
            lab[r2] = (j < d && kv[r2]) ? L[(size_t)j * HW + kp] : 0.0f;      // A operand of the second product: class j, key (r2, h)
        }
#pragma unroll
        for (int n = 0; n < NQ; n++) {
            float mx = kVosNone;
#pragma unroll
            for (int r2 = 0; r2 < 16; r2++) {
                s[n][r2] = kv[r2] ? temperature * s[n][r2] : kVosNone;
                mx = fmaxf(mx, s[n][r2]);
            }
            mx = fmaxf(mx, __shfl_xor(mx, 32));                  // row 0 of every tile exists, so mx is a real logit
            const float m_new = fmaxf(m[n], mx), scale = expf(m[n] - m_new);
            m[n] = m_new;
            l[n] *= scale;
#pragma unroll
            for (int r2 = 0; r2 < 8; r2++) acc[n][r2] *= scale;  // classes live in rows 0 .. 15 = registers 0 .. 7
#pragma unroll
            for (int r2 = 0; r2 < 16; r2++) {
                const float e = kv[r2] ? expf(s[n][r2] - m_new) : 0.0f;
                l[n] += e;
                const float dy = (float)(ky[r2] - qy[n]), dx = (float)(kx[r2] - qx[n]);
                const float wgt = expf(-(dy * dy + dx * dx) / sigma2);
                acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(lab[r2], e * wgt, acc[n], 0, 0, 0);
            }
        }
    }

    // the waves' states, merged in wave order: sm[w][field][QT], field 0 = m, 1 = l (both lane halves), 2 + c = acc[c]
    __syncthreads();                                             // the target tile is no longer read
    const int F = 2 + kVosMaxClasses;
    float *mine = smem + (size_t)w * F * QT;
#pragma unroll
    for (int n = 0; n < NQ; n++) {
        const float lt = l[n] + __shfl_xor(l[n], 32);
        if (h == 0) { mine[0 * QT + 32 * n + j] = m[n]; mine[1 * QT + 32 * n + j] = lt; }
#pragma unroll
        for (int r2 = 0; r2 < 8; r2++) {
            const int c = (r2 & 3) + 8 * (r2 >> 2) + 4 * h;
            mine[(2 + c) * QT + 32 * n + j] = acc[n][r2];
        }
    }
    __syncthreads();
    if (tid < QT && q0 + tid < HW) {
        float M = kVosNone;
        for (int v = 0; v < kVosWaves; v++) M = fmaxf(M, smem[(size_t)v * F * QT + tid]);
        float f[kVosWaves];
        for (int v = 0; v < kVosWaves; v++) {
            const float mv = smem[(size_t)v * F * QT + tid];
            f[v] = mv == kVosNone ? 0.0f : expf(mv - M);
        }
        float *out = part + ((size_t)(item0 + b) * kVosMaxSplits + sp) * (size_t)(2 + d) * HW + q0 + tid;
        out[0] = M;
        for (int fld = 1; fld < 2 + d; fld++) {
            float sum = 0.0f;
            for (int v = 0; v < kVosWaves; v++) sum += f[v] * smem[((size_t)v * F + fld) * QT + tid];
            out[(size_t)fld * HW] = sum;
        }
    }
}

__global__ void __launch_bounds__(256) k_vos_merge(const VosItems I, int d, int HW, const float *__restrict__ part, int item0)
{
    const int b = blockIdx.y, q = blockIdx.x * 256 + threadIdx.x;
    if (q >= HW) return;
    const int n_split = I.n_split[b];
    const size_t stride = (size_t)(2 + d) * HW;
    const float *p = part + (size_t)(item0 + b) * kVosMaxSplits * stride + q;
    float M = kVosNone;
    for (int s = 0; s < n_split; s++) M = fmaxf(M, p[s * stride]);
    float L = 0.0f, acc[kVosMaxClasses];
#pragma unroll
    for (int c = 0; c < kVosMaxClasses; c++) acc[c] = 0.0f;
    for (int s = 0; s < n_split; s++) {
        const float ms = p[s * stride];
        if (ms == kVosNone) continue;                            // a split without tiles
        const float f = expf(ms - M);
        L += f * p[s * stride + HW];
#pragma unroll
        for (int c = 0; c < kVosMaxClasses; c++)
            if (c < d) acc[c] += f * p[s * stride + (size_t)(2 + c) * HW];
    }
    float *pred = I.pred[b], *onehot = I.onehot[b];
    float best = 0.0f;
    int arg = 0;
#pragma unroll
    for (int c = 0; c < kVosMaxClasses; c++) {
        if (c < d) {
            const float v = acc[c] / L;
            pred[(size_t)c * HW + q] = v;
            if (c == 0 || v > best) { best = v; arg = c; }
        }
    }
    if (onehot)
        for (int c = 0; c < d; c++) onehot[(size_t)c * HW + q] = c == arg ? 1.0f : 0.0f;
}

// torch's interpolate(mode='bilinear', align_corners=False) along one axis: the two taps and their weights for output index o
__device__ inline void vos_taps(int o, int n_in, int n_out, int &i0, int &i1, float &w0, float &w1)
{
    const float scale = (float)n_in / (float)n_out;
    float src = __fsub_rn(__fmul_rn(scale, (float)o + 0.5f), 0.5f);       // product and difference rounded separately, as torch's
    src = src < 0.0f ? 0.0f : src;
    i0 = min((int)src, n_in - 1);
    i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
    w1 = src - (float)i0;
    w0 = 1.0f - w1;
}

// grid (ceil(Wd / 64), ceil(Hd / 4)), 64 x 4 threads: one output position, all classes
__global__ void __launch_bounds__(256) k_vos_first_labels(int H, int W, int Hd, int Wd, int d, const uint8_t *__restrict__ label,
                                                          float *__restrict__ out)
{
    const int ox = blockIdx.x * 64 + threadIdx.x, oy = blockIdx.y * 4 + threadIdx.y;
    if (ox >= Wd || oy >= Hd) return;
    int y0, y1, x0, x1;
    float wy0, wy1, wx0, wx1;
    vos_taps(oy, H, Hd, y0, y1, wy0, wy1);
    vos_taps(ox, W, Wd, x0, x1, wx0, wx1);
    const int l00 = label[(size_t)y0 * W + x0], l01 = label[(size_t)y0 * W + x1], l10 = label[(size_t)y1 * W + x0], l11 = label[(size_t)y1 * W + x1];
    for (int c = 0; c < d; c++) {
        const float v00 = l00 == c, v01 = l01 == c, v10 = l10 == c, v11 = l11 == c;
        out[((size_t)c * Hd + oy) * Wd + ox] = wy0 * (wx0 * v00 + wx1 * v01) + wy1 * (wx0 * v10 + wx1 * v11);
    }
}

// grid (ceil(W / 64), ceil(H / 4)), 64 x 4 threads: one pixel; the d upsampled values exist in registers only
__global__ void __launch_bounds__(256) k_vos_masks(int d, int Hd, int Wd, int H, int W, const float *__restrict__ pred, uint8_t *__restrict__ mask)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= W || y >= H) return;
    int y0, y1, x0, x1;
    float wy0, wy1, wx0, wx1;
    vos_taps(y, Hd, H, y0, y1, wy0, wy1);
    vos_taps(x, Wd, W, x0, x1, wx0, wx1);
    float best = 0.0f;
    int arg = 0;
    for (int c = 0; c < d; c++) {
        const float *p = pred + (size_t)c * Hd * Wd;
        const float v = wy0 * (wx0 * p[y0 * Wd + x0] + wx1 * p[y0 * Wd + x1]) + wy1 * (wx0 * p[y1 * Wd + x0] + wx1 * p[y1 * Wd + x1]);
        if (c == 0 || v > best) { best = v; arg = c; }
    }
    mask[(size_t)y * W + x] = (uint8_t)arg;
}

constexpr int kVosInputChunk = 32;
struct VosInputFrames { const uint8_t *bgr[kVosInputChunk]; };

// grid (ceil(H * W / 256), frames of a chunk): pixel p of frame z, BGR bytes -> planes R, G, B
__global__ void __launch_bounds__(256) k_vos_inputs(int n_px, const VosInputFrames F, float *__restrict__ out, int frame0)
{
    const int p = blockIdx.x * 256 + threadIdx.x, z = blockIdx.y;
    if (p >= n_px) return;
    const uint8_t *__restrict__ bgr = F.bgr[z] + 3 * (size_t)p;
    float *o = out + (size_t)(frame0 + z) * 3 * n_px + p;
    o[0] = ((float)bgr[2] / 255.0f - 0.485f) / 0.229f;
    o[(size_t)n_px] = ((float)bgr[1] / 255.0f - 0.456f) / 0.224f;
    o[2 * (size_t)n_px] = ((float)bgr[0] / 255.0f - 0.406f) / 0.225f;
}

}  // namespace btba
