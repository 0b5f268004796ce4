// btba_detect.hpp -- detector front end (btba_detector_inputs, btba_detector_keypoints_to_image, include/btba.h)
//   Lfnet::detectFeature   src/FeatureManager.cpp:811-908  (crop to the ROI, zero-pad to a square, cv::resize to S x S, and the
//                                                            inverse transform applied to the returned keypoints; rot_deg = 0)
//   run_server.py          lf-net-release/run_server.py:160-165  (RGB2GRAY on the BGR bytes, / 255)
// The reference does the crop and resize on the host with OpenCV and ships the bytes over zmq.  Here, per chunk of up to
// kDetChunk frames (pointers, crop origins and transform coefficients travel as kernel arguments, so an asynchronous call keeps
// no host memory alive and the workspace needs no scratch):
//   k_detect_inputs       grid (ceil(S / 256), S / 4, frames), 64 x 4 threads: each lane makes 4 consecutive output pixels of one
//                         row -- its own column and row coefficients (OpenCV's fixed-point INTER_LINEAR, or the 2 x 2 box of
//                         INTER_AREA when side == 2 S), taps read straight from the uchar4 colour map with the zero padding
//                         decided per tap, one 12-byte store of BGR bytes and one 16-byte store of grey floats (exact g / 255.0f
//                         from a 256-entry LDS table)
//   k_detect_keypoints    grid (ceil(max n / 256), frames), 256 threads: one keypoint per lane, two uncontracted fp32 mul + add
// All integer logic plus rounded fp32 / fp64 steps written out in include/btba.h: the outputs equal a CPU restatement exactly
// (tests/detector_ref.py).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace btba {

constexpr int kDetChunk = 32;                  // frames per launch
constexpr int kDetMaxSize = 4096;              // out_size <= 4096, a multiple of 4
constexpr int kDetMaxKpts = 8192;              // keypoints per frame

struct DetectFrames {
    const uchar4 *color[kDetChunk];            // the crop's top-left pixel, colour(vmin, umin)
    int wc[kDetChunk], hc[kDetChunk];          // crop width and height; side = max(wc, hc)
};

struct KptFrames {
    const float2 *in[kDetChunk];
    float2 *out[kDetChunk];
    int n[kDetChunk];
    float r00[kDetChunk], r02[kDetChunk], r11[kDetChunk], r12[kDetChunk];
};

// g / 255.0f for g = 0 .. 255, folded by the compiler (IEEE division, correctly rounded)
struct GreyTable {
    float v[256];
    constexpr GreyTable() : v()
    {
        for (int g = 0; g < 256; g++) v[g] = (float)g / 255.0f;
    }
};
__constant__ const GreyTable kGreyTable = GreyTable();

// cv::resize's per-coordinate setup (resizeGeneric, INTER_LINEAR, fixed point): source index and the two 11-bit weights.
// `zero_border` is the column rule (fx = 0 at both ends); rows keep fy and clamp their two indices instead.
__device__ __forceinline__ void det_coeff(int d, double scale, int side, bool zero_border, int &s0, int &s1, int &w0, int &w1)
{
#pragma clang fp contract(off)
    float f = (float)((d + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    if (zero_border) {
        if (s < 0) { f = 0.f; s = 0; }
        if (s >= side - 1) { f = 0.f; s = side - 1; }
        s0 = s;
        s1 = min(s + 1, side - 1);             // only read where w1 = 0 when clamped
    } else {
        s0 = min(max(s, 0), side - 1);
        s1 = min(max(s + 1, 0), side - 1);
    }
    w0 = (int)rintf((1.f - f) * 2048.f);
    w1 = (int)rintf(f * 2048.f);
}

// one padded-square texel: colour bytes (B, G, R) inside the crop, 0 in the padding
__device__ __forceinline__ int3 det_tap(const uchar4 *__restrict__ c, int W, int wc, int hc, int y, int x)
{
    if (x >= wc || y >= hc) return make_int3(0, 0, 0);
    const uchar4 p = c[(size_t)y * W + x];
    return make_int3(p.x, p.y, p.z);
}

__global__ void __launch_bounds__(256) k_detect_inputs(int W, int S, const DetectFrames F, int frame0, uint8_t *__restrict__ bgr_out,
                                                       float *__restrict__ gray_out)
{
    __shared__ float grey[256];
    const int li = threadIdx.y * 64 + threadIdx.x;
    grey[li] = kGreyTable.v[li];
    __syncthreads();
    const int z = blockIdx.z, dy = blockIdx.y * 4 + threadIdx.y, dx0 = (blockIdx.x * 64 + threadIdx.x) * 4;
    if (dx0 >= S) return;                      // S % 4 == 0: a lane has all four pixels or none; dy < S by the grid
    const uchar4 *c = F.color[z];
    const int wc = F.wc[z], hc = F.hc[z], side = max(wc, hc);
    int3 px[4];
    if (side == 2 * S) {                       // cv::resize's INTER_AREA switch for an exact 2 x 2 reduction
        for (int i = 0; i < 4; i++) {
            const int x = 2 * (dx0 + i), y = 2 * dy;
            const int3 a = det_tap(c, W, wc, hc, y, x), b = det_tap(c, W, wc, hc, y, x + 1);
            const int3 d = det_tap(c, W, wc, hc, y + 1, x), e = det_tap(c, W, wc, hc, y + 1, x + 1);
            px[i] = make_int3((a.x + b.x + d.x + e.x + 2) >> 2, (a.y + b.y + d.y + e.y + 2) >> 2, (a.z + b.z + d.z + e.z + 2) >> 2);
        }
    } else {
        const double scale = 1.0 / ((double)S / side);
        int y0, y1, b0, b1;
        det_coeff(dy, scale, side, false, y0, y1, b0, b1);
        for (int i = 0; i < 4; i++) {
            int x0, x1, a0, a1;
            det_coeff(dx0 + i, scale, side, true, x0, x1, a0, a1);
            const int3 p00 = det_tap(c, W, wc, hc, y0, x0), p01 = det_tap(c, W, wc, hc, y0, x1);
            const int3 p10 = det_tap(c, W, wc, hc, y1, x0), p11 = det_tap(c, W, wc, hc, y1, x1);
            // VResizeLinearVec_32s8u: (h >> 4) as int16, mul_hi by the row weight, + 2 >> 2, saturated to uint8
            auto v = [&](int t0, int t1, int u0, int u1) {
                const int h0 = t0 * a0 + t1 * a1, h1 = u0 * a0 + u1 * a1;
                const int r = ((((h0 >> 4) * b0) >> 16) + (((h1 >> 4) * b1) >> 16) + 2) >> 2;
                return min(max(r, 0), 255);
            };
            px[i] = make_int3(v(p00.x, p01.x, p10.x, p11.x), v(p00.y, p01.y, p10.y, p11.y), v(p00.z, p01.z, p10.z, p11.z));
        }
    }
    const size_t o = ((size_t)(frame0 + z) * S + dy) * S + dx0;
    if (bgr_out) {
        uint32_t w[3] = { 0, 0, 0 };
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int b = 3 * i;
            w[b >> 2] |= (uint32_t)px[i].x << (8 * (b & 3));
            w[(b + 1) >> 2] |= (uint32_t)px[i].y << (8 * ((b + 1) & 3));
            w[(b + 2) >> 2] |= (uint32_t)px[i].z << (8 * ((b + 2) & 3));
        }
        uint32_t *dst = reinterpret_cast<uint32_t *>(bgr_out + 3 * o);          // o % 4 == 0: 4-byte aligned
        dst[0] = w[0];
        dst[1] = w[1];
        dst[2] = w[2];
    }
    if (gray_out) {
        float g[4];
#pragma unroll
        for (int i = 0; i < 4; i++) g[i] = grey[(9798 * px[i].x + 19235 * px[i].y + 3735 * px[i].z + 16384) >> 15];
        *reinterpret_cast<float4 *>(gray_out + o) = make_float4(g[0], g[1], g[2], g[3]);
    }
}

__global__ void __launch_bounds__(256) k_detect_keypoints(const KptFrames F)
{
#pragma clang fp contract(off)
    const int z = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= F.n[z]) return;
    const float2 k = F.in[z][i];
    F.out[z][i] = make_float2(F.r00[z] * k.x + F.r02[z], F.r11[z] * k.y + F.r12[z]);
}

}  // namespace btba
