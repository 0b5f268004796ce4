// btba_ingest.hpp -- batched frame ingest (btba_ingest_frames, include/btba.h): what Frame's constructor does to the two images
// of a new frame, for many frames in one call
//   Utils::readDepthImage           src/Utils.cpp:50-69    (16-bit codes -> metres, below 0.1 -> 0)
//   Frame::updateColorGPU           src/Frame.cpp:114-127  (BGR bytes -> uchar4 (B, G, R, 0))
//   Frame::processDepth             src/Frame.cpp:152-180  (btba_image.hpp: process_depth_tile)
//   Frame::depthToCloudAndNormals   src/Frame.cpp:182-233  (btba_image.hpp: depth_to_normals_pixel)
// Per chunk of up to BTBA_INGEST_CHUNK frames (the pointer tables travel as kernel arguments, so an asynchronous call keeps no
// host memory alive and the workspace needs no scratch), two launches with grid.z = the frame within the chunk:
//   k_ingest_depth     grid (ceil(W / 32), ceil(H / 8), frames), 256 threads: btba_process_depth's tile chain with the decode in the
//                      tile's stage-0 load -- the uint16 path reads 2 bytes per pixel and writes no decoded image unless
//                      depth_raw_out asks for one (each workgroup then writes its own 32 x 8 interior)
//   k_ingest_maps      grid (ceil(W / 64), ceil(H / 4), frames), 64 x 4 threads: btba_depth_to_normals' pixel on the processed depth,
//                      and the colour pack on the same grid read as a flat index: lane t packs pixels 4t .. 4t + 3 from three dword
//                      loads into four dword stores (bytewise for the last W * H % 4 pixels and for a BGR image off 4-byte alignment)
// The arithmetic is the per-frame kernels' own device functions, so every output equals theirs bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/btba.h"
#include "btba_image.hpp"

namespace btba {

constexpr int kIngestChunk = BTBA_INGEST_CHUNK;       // frames per launch

struct IngestDepthFrames {
    const void *in[kIngestChunk];                      // uint16 codes or float metres
    float *out[kIngestChunk];                          // the processed depth
    float *raw[kIngestChunk];                          // NULL, or the decoded depth
};

struct IngestMapFrames {
    const float *depth[kIngestChunk];                  // the processed depth
    float4 *normals[kIngestChunk];
    float4 *xyz[kIngestChunk];                         // NULL, or the camera-space points
    const uint8_t *bgr[kIngestChunk];                  // NULL with color
    uint32_t *color[kIngestChunk];                     // NULL, or uchar4 (B, G, R, 0) as one dword per pixel
};

template <int RE, int RF, typename TIn>
__global__ void __launch_bounds__(256) k_ingest_depth(DepthFilterParams P, const IngestDepthFrames F)
{
    extern __shared__ __attribute__((aligned(16))) float tile[];
    const int z = blockIdx.z;
    const TIn *in = static_cast<const TIn *>(F.in[z]);
    const int h = (RE >= 0 ? RE : P.erode_radius) + 2 * (RF >= 0 ? RF : P.bf_radius);
    const int x0 = blockIdx.x * kTileW - h, y0 = blockIdx.y * kTileH - h;
    const bool interior = x0 >= 0 && y0 >= 0 && x0 + kTileW + 2 * h <= P.W && y0 + kTileH + 2 * h <= P.H;      // (uniform)
    if (interior) process_depth_tile<RE, RF, true, TIn>(P, in, F.out[z], tile, F.raw[z]);
    else process_depth_tile<RE, RF, false, TIn>(P, in, F.out[z], tile, F.raw[z]);
}

template <typename TIn>
inline void launch_ingest_depth(const DepthFilterParams &P, const IngestDepthFrames &F, dim3 grid, size_t lds, hipStream_t stream)
{
    if (P.erode_radius == 1 && P.bf_radius == 2) k_ingest_depth<1, 2, TIn><<<grid, 256, lds, stream>>>(P, F);        // the tracker's stencils, unrolled
    else k_ingest_depth<-1, -1, TIn><<<grid, 256, lds, stream>>>(P, F);
}

// grid (ceil(W/64), ceil(H/4)) x (64, 4).  normals (and optionally the xyz map) for one frame.
__global__ void __launch_bounds__(256) k_depth_to_normals(int W, int H, Mat4 Kinv, const float *__restrict__ depth, float4 *__restrict__ normals, float4 *__restrict__ xyz_out)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= W || y >= H) return;
    depth_to_normals_pixel(W, H, Kinv, depth, normals, xyz_out, x, y);
}

__global__ void __launch_bounds__(256) k_ingest_maps(int W, int H, Mat4 Kinv, const IngestMapFrames F)
{
    const int z = blockIdx.z;
    uint32_t *__restrict__ color = F.color[z];
    if (color) {                                       // (uniform)
        const uint8_t *__restrict__ bgr = F.bgr[z];
        const size_t n = (size_t)W * H;
        const size_t p0 = 4 * (((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 256 + threadIdx.y * 64 + threadIdx.x);
        if (p0 + 4 <= n && (reinterpret_cast<uintptr_t>(bgr) & 3) == 0) {
            const uint32_t *src = reinterpret_cast<const uint32_t *>(bgr + 3 * p0);          // b0 g0 r0 b1 | g1 r1 b2 g2 | r2 b3 g3 r3
            const uint32_t w0 = src[0], w1 = src[1], w2 = src[2];
            color[p0] = w0 & 0xffffffu;
            color[p0 + 1] = (w0 >> 24) | ((w1 & 0xffffu) << 8);
            color[p0 + 2] = (w1 >> 16) | ((w2 & 0xffu) << 16);
            color[p0 + 3] = w2 >> 8;
        } else {
            for (size_t p = p0; p < n && p < p0 + 4; p++)
                color[p] = (uint32_t)bgr[3 * p] | ((uint32_t)bgr[3 * p + 1] << 8) | ((uint32_t)bgr[3 * p + 2] << 16);
        }
    }
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= W || y >= H) return;
    depth_to_normals_pixel(W, H, Kinv, F.depth[z], F.normals[z], F.xyz[z], x, y);
}

}  // namespace btba
