// btba_lfnet.hpp -- LF-Net's keypoint head between its two conv nets (lf-net-release/inference.py::
// build_multi_scale_deep_detector_3DNMS and build_patch_extraction, on det_tools.py and spatial_transformer.py), as three stages.
//
// Stage A (k_lfnet_moments, k_lfnet_heat).  Per score map x [h_s][w_s]: mean and biased variance in fp64 (two passes, as
// tf.nn.moments), inv = 1 / sqrt((float)var + 1e-3f), logit = x * inv - mean * inv in fp32.  Every scale is resized to H x W as TF1's
// resize_images does (src = dst * (in / (float)out), lower tap floor, upper tap min(lower + 1, in - 1), top = tl + (tr - tl) * fx,
// bottom likewise, value = top + (bottom - top) * fy).  With N(q) the S x k x k scale-space window of q cut to the image:
//   M(q)   = max over N(q) of the logits                                  (max_pool3d, SAME)
//   e_s(q) = exp(com * (logit_s(q) - M(q)))
//   p_s(q) = e_s(q) / (sum over N(q) of e + 1e-6)                          (conv3d of ones, SAME: outside counts as zero)
//   heat   = sum_s p_s * (a_s / (sum a + 1e-8)),  a_s = exp(score_com * (p_s - max_s p))
//   scale  = sum_s scale_factors[s] * (b_s / (sum b + 1e-8)),  b_s = exp(scale_com * (p_s - max_s p))
// and heat is multiplied by the pad_size frame mask.  One workgroup makes a T x T output tile.  With h = k / 2 it needs M on the
// tile grown by h and the logits on the tile grown by 2 h: every resized logit of the grown tile is produced once, folded into a
// max-over-scales plane, and kept in LDS only where an exponential will need it (the tile grown by h).  The window maximum and
// the window sum are separable: rows, then columns.  Nothing full-size is written except the two outputs.
//
// Stage B (k_lfnet_peaks, k_lfnet_select): exact.  works = heat below nms_thresh ? 0 : heat; a peak is strictly greater than its
// ksize^2 - 1 neighbours of works, zeros outside the image; score = heat * peak * crop_radius frame mask; tf.nn.top_k over the
// flattened frame (equal values: the lower flat index first); of the chosen positions the peaks survive, in raster order.  The
// k-th largest score T over ALL positions is found by a radix select on the order-preserving image of the float bits over the
// compacted peaks, the non-peaks entering as one count at the image of zero.  A peak above T survives; a peak equal to T survives
// if fewer than (k - count above T) positions equal to T lie before it -- for T = 0 that count is its flat index minus the nonzero
// peaks before it (the fill case), otherwise the equal peaks before it.  The list is compacted in raster order, so is the output.
//
// Stage C (k_lfnet_crops): one wave per keypoint slot.  transformer_crop as written: g = linspace(-1, 1, n) (start + i * step),
// (x, y) = ((s c g_x - s sn g_y) n / 2 + kp_x, (s sn g_x + s c g_y) n / 2 + kp_y), taps floor and floor + 1 CLAMPED into the image,
// weights from the clamped tap coordinates, value = wa Ia + wb Ib + wc Ic + wd Id.  soft_argmax_2d over the L x L scale-only crop
// of the heat map, kpt = (float)kp + dxdy * scale * L / 2, then the P x P crop of the photo with scale and orientation.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace btba {

constexpr int kLfnetMaxScales = 16;
constexpr int kLfnetSelectThreads = 1024;

struct LfnetMaps {
    const float *p[kLfnetMaxScales];                 // [n_frames][h][w] per scale
    int h[kLfnetMaxScales], w[kLfnetMaxScales];
    float sf[kLfnetMaxScales];
};

__host__ __device__ inline size_t lfnet_heat_lds_floats(int S, int T, int h)
{
    const size_t R2 = T + 2 * h, R4 = T + 4 * h;
    return (size_t)S * R2 * R2 + R4 * R4 + R4 * R2 + R2 * T;
}

// grid (S, n_frames), 256 threads: stats[f * S + s] = (inv, mean * inv)
__global__ __launch_bounds__(256) void k_lfnet_moments(LfnetMaps M, float2 *__restrict__ stats)
{
    __shared__ double red[256];
    const int s = blockIdx.x, f = blockIdx.y, S = gridDim.x, t = threadIdx.x;
    const int n = M.h[s] * M.w[s];
    const float *x = M.p[s] + (size_t)f * n;
    double a = 0.0;
    for (int i = t; i < n; i += 256) a += (double)x[i];
    red[t] = a;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if (t < o) red[t] += red[t + o]; __syncthreads(); }
    const double mean = red[0] / (double)n;
    __syncthreads();
    double b = 0.0;
    for (int i = t; i < n; i += 256) { const double d = (double)x[i] - mean; b += d * d; }
    red[t] = b;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if (t < o) red[t] += red[t + o]; __syncthreads(); }
    if (t == 0) {
        const float var = (float)(red[0] / (double)n), inv = 1.0f / sqrtf(var + 1e-3f);
        stats[f * S + s] = make_float2(inv, (float)mean * inv);
    }
}

// grid (ceil(W / T), ceil(H / T), n_frames), 256 threads, lfnet_heat_lds_floats(S, T, h) floats of dynamic LDS
__global__ __launch_bounds__(256) void k_lfnet_heat(LfnetMaps M, const float2 *__restrict__ stats, int S, int H, int W, int T, int h,
                                                    float com, float c1, float c2, int pad, float *__restrict__ heat_out,
                                                    float *__restrict__ scale_out)
{
    extern __shared__ float lds[];
    const int R2 = T + 2 * h, R4 = T + 4 * h, K = 2 * h + 1;
    float *L = lds, *P0 = L + (size_t)S * R2 * R2, *P1 = P0 + R4 * R4, *P2 = P1 + R4 * R2;
    const int f = blockIdx.z, x0 = blockIdx.x * T, y0 = blockIdx.y * T, t = threadIdx.x;
    const float NEG = -__builtin_inff();

    // 1: the resized logits of the tile grown by 2 h, once; max over scales into P0, the part grown by h kept in L
    for (int i = t; i < R4 * R4; i += 256) {
        const int ry = i / R4, rx = i - ry * R4, gy = y0 - 2 * h + ry, gx = x0 - 2 * h + rx;
        const bool inside = gy >= 0 && gy < H && gx >= 0 && gx < W;
        const int qy = ry - h, qx = rx - h;
        const bool keep = qy >= 0 && qy < R2 && qx >= 0 && qx < R2;
        float m = NEG;
        for (int s = 0; s < S; s++) {
            float v = 0.0f;
            if (inside) {
                const int hs = M.h[s], wsz = M.w[s];
                const float sy = (float)gy * ((float)hs / (float)H), sx = (float)gx * ((float)wsz / (float)W);
                const int ya = min((int)floorf(sy), hs - 1), xa = min((int)floorf(sx), wsz - 1);
                const int yb = min(ya + 1, hs - 1), xb = min(xa + 1, wsz - 1);
                const float fy = sy - (float)ya, fx = sx - (float)xa;
                const float *src = M.p[s] + (size_t)f * hs * wsz;
                const float2 st = stats[f * S + s];
                const float tl = src[(size_t)ya * wsz + xa] * st.x - st.y, tr = src[(size_t)ya * wsz + xb] * st.x - st.y;
                const float bl = src[(size_t)yb * wsz + xa] * st.x - st.y, br = src[(size_t)yb * wsz + xb] * st.x - st.y;
                const float top = tl + (tr - tl) * fx, bot = bl + (br - bl) * fx;
                v = top + (bot - top) * fy;
                m = fmaxf(m, v);
            }
            if (keep) L[(size_t)s * R2 * R2 + qy * R2 + qx] = v;
        }
        P0[i] = m;
    }
    __syncthreads();
    // 2: window maximum along rows: P1 [R4][R2]
    for (int i = t; i < R4 * R2; i += 256) {
        const int r = i / R2, c = i - r * R2;
        float m = NEG;
        for (int d = 0; d < K; d++) m = fmaxf(m, P0[r * R4 + c + d]);
        P1[i] = m;
    }
    __syncthreads();
    // 3: along columns: M on the tile grown by h, into P0 [R2][R2]
    for (int i = t; i < R2 * R2; i += 256) {
        const int r = i / R2, c = i - r * R2;
        float m = NEG;
        for (int d = 0; d < K; d++) m = fmaxf(m, P1[(r + d) * R2 + c]);
        P0[i] = m;
    }
    __syncthreads();
    // 4: sum over scales of the exponentials, zero outside the image: P1 [R2][R2]
    for (int i = t; i < R2 * R2; i += 256) {
        const int r = i / R2, c = i - r * R2, gy = y0 - h + r, gx = x0 - h + c;
        float e = 0.0f;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const float mx = P0[i];
            for (int s = 0; s < S; s++) e += expf(com * (L[(size_t)s * R2 * R2 + i] - mx));
        }
        P1[i] = e;
    }
    __syncthreads();
    // 5: window sum along rows: P2 [R2][T]
    for (int i = t; i < R2 * T; i += 256) {
        const int r = i / T, c = i - r * T;
        float a = 0.0f;
        for (int d = 0; d < K; d++) a += P1[r * R2 + c + d];
        P2[i] = a;
    }
    __syncthreads();
    // 6: along columns, the probabilities of the pixel's S scales, the soft max and arg-max over them
    for (int i = t; i < T * T; i += 256) {
        const int ty = i / T, tx = i - ty * T, gy = y0 + ty, gx = x0 + tx;
        if (gy >= H || gx >= W) continue;
        float sum = 0.0f;
        for (int d = 0; d < K; d++) sum += P2[(ty + d) * T + tx];
        const int c = (ty + h) * R2 + tx + h;
        const float mx = P0[c], den = sum + 1e-6f;
        float pm = NEG;
        for (int s = 0; s < S; s++) pm = fmaxf(pm, expf(com * (L[(size_t)s * R2 * R2 + c] - mx)) / den);
        float sa = 0.0f, sb = 0.0f;
        for (int s = 0; s < S; s++) {
            const float p = expf(com * (L[(size_t)s * R2 * R2 + c] - mx)) / den;
            sa += expf(c1 * (p - pm));
            sb += expf(c2 * (p - pm));
        }
        // sum_s p_s (a_s / (sum a + 1e-8)) with the quotient taken per scale, as the reference does
        float heat = 0.0f, scl = 0.0f;
        const float da = sa + 1e-8f, db = sb + 1e-8f;
        for (int s = 0; s < S; s++) {
            const float p = expf(com * (L[(size_t)s * R2 * R2 + c] - mx)) / den;
            heat += p * (expf(c1 * (p - pm)) / da);
            scl += M.sf[s] * (expf(c2 * (p - pm)) / db);
        }
        const bool in_pad = gy >= pad && gy < H - pad && gx >= pad && gx < W - pad;
        const size_t o = ((size_t)f * H + gy) * W + gx;
        heat_out[o] = in_pad ? heat : 0.0f;
        scale_out[o] = scl;
    }
}

// grid (ceil(H W / 256), n_frames): peak[f][i] = 1 where works is strictly greater than all its neighbours
__global__ __launch_bounds__(256) void k_lfnet_peaks(const float *__restrict__ heat, int H, int W, float thresh, int hk, uint8_t *__restrict__ peak)
{
    const int i = blockIdx.x * 256 + threadIdx.x, f = blockIdx.y;
    if (i >= H * W) return;
    const float *hm = heat + (size_t)f * H * W;
    const int y = i / W, x = i - y * W;
    float c = hm[i];
    if (c < thresh) c = 0.0f;
    bool is_peak = true;
    for (int dy = -hk; dy <= hk && is_peak; dy++)
        for (int dx = -hk; dx <= hk; dx++) {
            if (dy == 0 && dx == 0) continue;
            const int yy = y + dy, xx = x + dx;
            float v = 0.0f;
            if (yy >= 0 && yy < H && xx >= 0 && xx < W) { v = hm[(size_t)yy * W + xx]; if (v < thresh) v = 0.0f; }
            if (!(c > v)) { is_peak = false; break; }
        }
    peak[(size_t)f * H * W + i] = is_peak ? 1 : 0;
}

__device__ __forceinline__ uint32_t lfnet_key(float v)
{
    if (v == 0.0f) return 0x80000000u;                 // -0 and +0 are one score
    const uint32_t b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// Exclusive prefix of `flag` over the workgroup in thread order; `total` is the workgroup's count.  wsum: one int per wave.
__device__ __forceinline__ int lfnet_block_scan(bool flag, int *wsum, int &total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
    const unsigned long long b = __ballot(flag);
    const int before = __popcll(b & ((1ull << lane) - 1ull));
    __syncthreads();                                   // the previous scan's readers are done with wsum
    if (lane == 0) wsum[wave] = __popcll(b);
    __syncthreads();
    int off = 0, tot = 0;
    for (int w = 0; w < n_waves; w++) { const int c = wsum[w]; if (w < wave) off += c; tot += c; }
    total = tot;
    return off + before;
}

// grid n_frames, kLfnetSelectThreads threads.  list_idx / list_key: [n_frames][H W] scratch.
__global__ __launch_bounds__(kLfnetSelectThreads) void k_lfnet_select(const float *__restrict__ heat, const uint8_t *__restrict__ peak, int H, int W,
                                                                      int crop, int top_k, int32_t *__restrict__ list_idx,
                                                                      uint32_t *__restrict__ list_key, int32_t *__restrict__ kpts_xy,
                                                                      int32_t *__restrict__ n_kpts)
{
    __shared__ int wsum[kLfnetSelectThreads / 64];
    __shared__ unsigned hist[256];
    __shared__ unsigned sel_prefix, sel_need;
    const int f = blockIdx.x, t = threadIdx.x, HW = H * W, NT = kLfnetSelectThreads;
    const float *hm = heat + (size_t)f * HW;
    const uint8_t *pk = peak + (size_t)f * HW;
    int32_t *li = list_idx + (size_t)f * HW;
    uint32_t *lk = list_key + (size_t)f * HW;
    int32_t *out = kpts_xy + (size_t)f * top_k * 2;
    const uint32_t U0 = 0x80000000u;

    // the peaks, compacted in raster order
    int n_peaks = 0;
    for (int base = 0; base < HW; base += NT) {
        const int i = base + t;
        const bool flag = i < HW && pk[i] != 0;
        int total;
        const int pos = lfnet_block_scan(flag, wsum, total);
        if (flag) {
            const int y = i / W, x = i - y * W;
            const bool in_crop = y >= crop && y < H - crop && x >= crop && x < W - crop;
            li[n_peaks + pos] = i;
            lk[n_peaks + pos] = in_crop ? lfnet_key(hm[i]) : U0;
        }
        n_peaks += total;
    }
    __syncthreads();                                   // the list is this workgroup's own: visible after the barrier

    // radix select: the k-th largest key over all H W positions, the non-peaks counted at U0
    const unsigned k = (unsigned)min(top_k, HW), n_rest = (unsigned)(HW - n_peaks);
    if (t == 0) { sel_prefix = 0u; sel_need = k; }
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (t < 256) hist[t] = 0u;
        __syncthreads();
        const uint32_t prefix = sel_prefix, hi_mask = shift == 24 ? 0u : ~0u << (shift + 8);
        for (int j = t; j < n_peaks; j += NT) {
            const uint32_t u = lk[j];
            if ((u & hi_mask) == prefix) atomicAdd(&hist[(u >> shift) & 255u], 1u);
        }
        if (t == 0 && (U0 & hi_mask) == prefix) atomicAdd(&hist[(U0 >> shift) & 255u], n_rest);
        __syncthreads();
        if (t == 0) {
            unsigned need = sel_need;
            int b = 255;
            for (; b > 0; b--) { if (hist[b] >= need) break; need -= hist[b]; }
            sel_prefix = prefix | ((uint32_t)b << shift);
            sel_need = need;
        }
        __syncthreads();
    }
    const uint32_t Tk = sel_prefix;
    const int need = (int)sel_need;                    // how many of the positions equal to Tk are taken, lowest flat index first
    const bool fill = Tk == U0;

    // the survivors, in list order = raster order
    int n_out = 0, before = 0;                         // before: nonzero peaks (fill) or peaks equal to Tk seen so far
    for (int base = 0; base < n_peaks; base += NT) {
        const int j = base + t;
        const bool live = j < n_peaks;
        const uint32_t u = live ? lk[j] : 0u;
        const int idx = live ? li[j] : 0;
        const bool tie = live && u == Tk;
        int total;
        const int r = lfnet_block_scan(live && (fill ? u != U0 : u == Tk), wsum, total);
        const int rank = fill ? idx - (before + r) : before + r;
        before += total;
        const bool sel = live && (u > Tk || (tie && rank < need));
        int n_sel;
        const int slot = lfnet_block_scan(sel, wsum, n_sel);
        if (sel && n_out + slot < top_k) {
            const int y = idx / W;
            out[2 * (n_out + slot)] = idx - y * W;
            out[2 * (n_out + slot) + 1] = y;
        }
        n_out += n_sel;
    }
    for (int j = n_out + t; j < top_k; j += NT) { out[2 * j] = 0; out[2 * j + 1] = 0; }
    if (t == 0) n_kpts[f] = n_out;
}

__device__ __forceinline__ float lfnet_wave_max(float v)
{
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float lfnet_wave_sum(float v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// transformer_crop's sample (row i, column j) of an n x n crop at (kx, ky): thetas = [[a, b], [c, d]]
__device__ __forceinline__ float lfnet_crop_sample(const float *__restrict__ img, int H, int W, int n, int i, int j, float a, float b,
                                                   float c, float d, float kx, float ky)
{
    const float step = 2.0f / (float)(n - 1), gx = -1.0f + (float)j * step, gy = -1.0f + (float)i * step;
    const float x = (a * gx + b * gy) * (float)n / 2.0f + kx, y = (c * gx + d * gy) * (float)n / 2.0f + ky;
    const float fx = fminf(fmaxf(floorf(x), -2.0f), (float)W), fy = fminf(fmaxf(floorf(y), -2.0f), (float)H);
    const int xi = (int)fx, yi = (int)fy;
    const int xa = min(max(xi, 0), W - 1), xb = min(max(xi + 1, 0), W - 1);
    const int ya = min(max(yi, 0), H - 1), yb = min(max(yi + 1, 0), H - 1);
    const float Ia = img[(size_t)ya * W + xa], Ib = img[(size_t)yb * W + xa], Ic = img[(size_t)ya * W + xb], Id = img[(size_t)yb * W + xb];
    const float wa = ((float)xb - x) * ((float)yb - y), wb = ((float)xb - x) * (y - (float)ya);
    const float wc = (x - (float)xa) * ((float)yb - y), wd = (x - (float)xa) * (y - (float)ya);
    return wa * Ia + wb * Ib + wc * Ic + wd * Id;
}

// grid (top_k, n_frames), 64 threads: one wave per keypoint slot
__global__ __launch_bounds__(64) void k_lfnet_crops(const float *__restrict__ photo, const float *__restrict__ ori, const float *__restrict__ heat,
                                                    const float *__restrict__ scales, const int32_t *__restrict__ kpts_xy,
                                                    const int32_t *__restrict__ n_kpts, int H, int W, int top_k, int soft, int L, int do_softmax,
                                                    float kp_com, int P, float *__restrict__ kpts_out, float *__restrict__ scale_out,
                                                    float *__restrict__ ori_out, float *__restrict__ patches)
{
    __shared__ float loc[64 * 64];
    const int slot = blockIdx.x, f = blockIdx.y, lane = threadIdx.x;
    const size_t ks = (size_t)f * top_k + slot, HW = (size_t)H * W;
    float *patch = patches + ks * P * P;
    if (slot >= n_kpts[f]) {
        for (int i = lane; i < P * P; i += 64) patch[i] = 0.0f;
        if (lane == 0) { kpts_out[2 * ks] = 0.0f; kpts_out[2 * ks + 1] = 0.0f; scale_out[ks] = 0.0f; ori_out[2 * ks] = 0.0f; ori_out[2 * ks + 1] = 0.0f; }
        return;
    }
    const int kx = min(max(kpts_xy[2 * ks], 0), W - 1), ky = min(max(kpts_xy[2 * ks + 1], 0), H - 1);
    const size_t px = f * HW + (size_t)ky * W + kx;
    const float sc = scales[px], co = ori[2 * px], sn = ori[2 * px + 1];
    float rx = (float)kx, ry = (float)ky;
    if (soft) {
        const float *hm = heat + f * HW;
        float m = -__builtin_inff();
        for (int i = lane; i < L * L; i += 64) {
            const float v = lfnet_crop_sample(hm, H, W, L, i / L, i % L, sc, 0.0f, 0.0f, sc, rx, ry);
            loc[i] = v;
            m = fmaxf(m, v);
        }
        m = lfnet_wave_max(m);
        float se = 0.0f;
        if (do_softmax) {
            for (int i = lane; i < L * L; i += 64) { const float e = expf(kp_com * (loc[i] - m)); loc[i] = e; se += e; }
            se = lfnet_wave_sum(se) + 1e-8f;
        }
        const float step = 2.0f / (float)(L - 1);
        float dx = 0.0f, dy = 0.0f;
        for (int i = lane; i < L * L; i += 64) {
            const float w = do_softmax ? loc[i] / se : loc[i];
            dx += (-1.0f + (float)(i % L) * step) * w;
            dy += (-1.0f + (float)(i / L) * step) * w;
        }
        dx = lfnet_wave_sum(dx);
        dy = lfnet_wave_sum(dy);
        rx = rx + dx * sc * (float)L / 2.0f;
        ry = ry + dy * sc * (float)L / 2.0f;
    }
    if (lane == 0) { kpts_out[2 * ks] = rx; kpts_out[2 * ks + 1] = ry; scale_out[ks] = sc; ori_out[2 * ks] = co; ori_out[2 * ks + 1] = sn; }
    const float *ph = photo + f * HW;
    const float a = sc * co, b = sc * -sn, c = sc * sn, d = sc * co;
    for (int i = lane; i < P * P; i += 64) patch[i] = lfnet_crop_sample(ph, H, W, P, i / P, i % P, a, b, c, d, rx, ry);
}

}  // namespace btba
