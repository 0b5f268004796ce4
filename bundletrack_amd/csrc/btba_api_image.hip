// btba_api_image.hip -- host side of libbtba.so: depth filtering, normals, frame ingest, foreground masks and the detector front end.
#include "btba_host_common.hpp"
#include "btba_ingest.hpp"
#include "btba_mask.hpp"
#include "btba_detect.hpp"

extern "C" {

int btba_process_depth(btba_workspace *ws, int H, int W, const float *depth_in_dev, float *depth_out_dev,
                       int erode_radius, float erode_diff, float erode_ratio, int bf_radius, float sigma_d, float sigma_r)
{
    DeviceGuard device_guard(ws);
    if (!ws || H < 1 || W < 1 || !depth_in_dev || !depth_out_dev || depth_in_dev == depth_out_dev) return BTBA_EINVAL;
    if (erode_radius < 0 || bf_radius < 0 || erode_radius + 2 * bf_radius > 16 || !(sigma_d > 0.0f) || !(sigma_r > 0.0f)) return BTBA_EINVAL;
    DepthFilterParams P{ W, H, erode_radius, erode_diff, erode_ratio, bf_radius, sigma_d, sigma_r };
    const int h = erode_radius + 2 * bf_radius;
    const size_t lds = 2 * sizeof(float) * (size_t)(kTileW + 2 * h) * (kTileH + 2 * h);
    const dim3 grid((W + kTileW - 1) / kTileW, (H + kTileH - 1) / kTileH);
    if (erode_radius == 1 && bf_radius == 2) k_process_depth<1, 2><<<grid, 256, lds, ws->stream>>>(P, depth_in_dev, depth_out_dev);        // the tracker's stencils, unrolled
    else k_process_depth<-1, -1><<<grid, 256, lds, ws->stream>>>(P, depth_in_dev, depth_out_dev);
    HIP_TRY(hipGetLastError());
    return BTBA_OK;
}

int btba_depth_to_normals(btba_workspace *ws, int H, int W, const float *K, const float *depth_dev, float *normals_dev, float *xyz_dev)
{
    DeviceGuard device_guard(ws);
    if (!ws || H < 1 || W < 1 || !K || !depth_dev || !normals_dev) return BTBA_EINVAL;
    float intr[4];
    Mat4 Kinv;
    scaled_intrinsics(H, W, H, W, K, intr, &Kinv);       // only the generic cofactor inverse of the 4x4 embedding is used
    k_depth_to_normals<<<dim3((W + 63) / 64, (H + 3) / 4), dim3(64, 4), 0, ws->stream>>>(W, H, Kinv, depth_dev, reinterpret_cast<float4 *>(normals_dev), reinterpret_cast<float4 *>(xyz_dev));
    HIP_TRY(hipGetLastError());
    return BTBA_OK;
}

void btba_ingest_params_default(btba_ingest_params *p)
{
    if (!p) return;
    p->depth_format = 0;
    p->erode_radius = 1; p->erode_diff = 0.001f; p->erode_ratio = 0.8f;          // config_ycbineoat.yml:9-16
    p->bf_radius = 2; p->sigma_d = 2.0f; p->sigma_r = 100000.0f;
}

int btba_ingest_frames(btba_workspace *ws, const btba_ingest_params *prm, int n_frames, int H, int W, const float *K,
                       const void *const *depth_in_dev, const uint8_t *const *bgr_in_dev, float *const *depth_out_dev,
                       float *const *normal_out_dev, uint8_t *const *color_out_dev, float *const *depth_raw_out_dev,
                       float *const *xyz_out_dev)
{
    // every argument is checked before the first HIP call
    if (!ws || !prm || n_frames < 1 || H < 1 || W < 1 || !K || !depth_in_dev || !depth_out_dev || !normal_out_dev) return BTBA_EINVAL;
    if (prm->depth_format < 0 || prm->depth_format > 1) return BTBA_EINVAL;
    if (prm->erode_radius < 0 || prm->bf_radius < 0 || prm->erode_radius + 2 * prm->bf_radius > 16 || !(prm->sigma_d > 0.0f) || !(prm->sigma_r > 0.0f))
        return BTBA_EINVAL;
    const size_t n_px = (size_t)H * W, in_bytes = n_px * (prm->depth_format == 0 ? sizeof(uint16_t) : sizeof(float));
    for (int f = 0; f < n_frames; f++) {
        const void *in = depth_in_dev[f];
        const uint8_t *bgr = bgr_in_dev ? bgr_in_dev[f] : nullptr;
        uint8_t *color = color_out_dev ? color_out_dev[f] : nullptr;
        float *raw = depth_raw_out_dev ? depth_raw_out_dev[f] : nullptr, *xyz = xyz_out_dev ? xyz_out_dev[f] : nullptr;
        if (!in || !depth_out_dev[f] || !normal_out_dev[f] || (color && !bgr)) return BTBA_EINVAL;
        if (misaligned(in, prm->depth_format == 0 ? 2 : 4) || misaligned(depth_out_dev[f], 4) || misaligned(normal_out_dev[f], 16) ||
            misaligned(color, 4) || misaligned(raw, 4) || misaligned(xyz, 16))
            return BTBA_EINVAL;
        auto overlaps_input = [&](const void *q, size_t bytes) {
            const uintptr_t a = reinterpret_cast<uintptr_t>(in), b = reinterpret_cast<uintptr_t>(q);
            return q && a < b + bytes && b < a + in_bytes;
        };
        if (overlaps_input(depth_out_dev[f], 4 * n_px) || overlaps_input(normal_out_dev[f], 16 * n_px) || overlaps_input(color, 4 * n_px) ||
            overlaps_input(raw, 4 * n_px) || overlaps_input(xyz, 16 * n_px))
            return BTBA_EINVAL;
    }
    DeviceGuard device_guard(ws);
    DepthFilterParams P{ W, H, prm->erode_radius, prm->erode_diff, prm->erode_ratio, prm->bf_radius, prm->sigma_d, prm->sigma_r };
    const int h = P.erode_radius + 2 * P.bf_radius;
    const size_t lds = 2 * sizeof(float) * (size_t)(kTileW + 2 * h) * (kTileH + 2 * h);
    float intr[4];
    Mat4 Kinv;
    scaled_intrinsics(H, W, H, W, K, intr, &Kinv);       // btba_depth_to_normals' inverse
    for (int b0 = 0; b0 < n_frames; b0 += kIngestChunk) {
        const int nf = std::min(kIngestChunk, n_frames - b0);
        IngestDepthFrames D{};
        IngestMapFrames M{};
        for (int z = 0; z < nf; z++) {
            const int f = b0 + z;
            D.in[z] = depth_in_dev[f];
            D.out[z] = depth_out_dev[f];
            D.raw[z] = depth_raw_out_dev ? depth_raw_out_dev[f] : nullptr;
            M.depth[z] = depth_out_dev[f];
            M.normals[z] = reinterpret_cast<float4 *>(normal_out_dev[f]);
            M.xyz[z] = xyz_out_dev ? reinterpret_cast<float4 *>(xyz_out_dev[f]) : nullptr;
            M.color[z] = color_out_dev ? reinterpret_cast<uint32_t *>(color_out_dev[f]) : nullptr;
            M.bgr[z] = M.color[z] ? bgr_in_dev[f] : nullptr;
        }
        const dim3 grid_d((W + kTileW - 1) / kTileW, (H + kTileH - 1) / kTileH, nf);
        if (prm->depth_format == 0) launch_ingest_depth<uint16_t>(P, D, grid_d, lds, ws->stream);
        else launch_ingest_depth<float>(P, D, grid_d, lds, ws->stream);
        HIP_TRY(hipGetLastError());
        k_ingest_maps<<<dim3((W + 63) / 64, (H + 3) / 4, nf), dim3(64, 4), 0, ws->stream>>>(W, H, Kinv, M);
        HIP_TRY(hipGetLastError());
    }
    return BTBA_OK;
}

void btba_mask_params_default(btba_mask_params *p)
{
    if (!p) return;
    p->largest_component_hull = 0;                                    // config_ycbineoat.yml: data_dir without "NOCS"
    p->dilate = 5;                                                    // Frame.cpp:310 (MORPH_RECT 5 x 5)
}

int btba_apply_masks(btba_workspace *ws, const btba_mask_params *prm, int n_frames, int H, int W,
                     const uint8_t *const *mask_dev, float *const *depth_dev, float *const *normal_dev,
                     uint8_t *const *color_dev, uint8_t *const *mask_out_dev, float *roi_out)
{
    // every argument is checked before the first HIP call
    if (!ws || !prm || prm->dilate < 1 || prm->dilate > 2 * kMaskMaxR + 1 || prm->dilate % 2 == 0 || n_frames < 1 || H < 1 || W < 1 ||
        (int64_t)H * W >= ((int64_t)1 << 31) || !mask_dev || !depth_dev || !normal_dev)
        return BTBA_EINVAL;
    for (int f = 0; f < n_frames; f++)
        if (!mask_dev[f] || !depth_dev[f] || !normal_dev[f] || misaligned(normal_dev[f], 16) ||
            (color_dev && color_dev[f] && misaligned(color_dev[f], 4)) ||
            (mask_out_dev && mask_out_dev[f] && static_cast<const void *>(mask_out_dev[f]) == static_cast<const void *>(mask_dev[f])))
            return BTBA_EINVAL;
    DeviceGuard device_guard(ws);
    const bool hull = prm->largest_component_hull != 0;
    const int r = prm->dilate / 2, chunk = std::min(n_frames, kMaskChunk);
    const size_t HW = (size_t)H * W;
    Scratch S;
    const auto s_roi = S.add<int>(4 * (size_t)n_frames, roi_out != nullptr);
    const auto s_lab = S.add<int>(chunk * HW, hull), s_cnt = S.add<int>(chunk * HW, hull);
    const auto s_best = S.add<unsigned long long>(chunk, hull);
    const auto s_rows = S.add<int2>(chunk * (size_t)H, hull), s_span = S.add<int2>(chunk * (size_t)H, hull);
    const auto s_stk = S.add<int2>(chunk * (4 * (size_t)H + 2), hull && H > kHullLdsMaxH);
    int rc;
    if ((rc = S.bind(ws->mask, 256))) return rc;
    int *d_roi = s_roi, *d_lab = s_lab, *d_cnt = s_cnt;
    unsigned long long *d_best = s_best;
    int2 *d_rows = s_rows, *d_span = s_span, *d_stk = s_stk;
    if (d_roi) HIP_TRY(hipMemsetAsync(d_roi, 0, sizeof(int) * 4 * n_frames, ws->stream));      // the zero start of k_mask_apply's ROI encoding
    const dim3 lgrid((W + kLabelTile - 1) / kLabelTile, (H + kLabelTile - 1) / kLabelTile, 1), lblock(kLabelTile, kLabelTile);
    const dim3 agrid((W + kMaskTileW - 1) / kMaskTileW, (H + kMaskTileH - 1) / kMaskTileH, 1), ablock(kMaskTileW, 4);
    const size_t hull_lds = H <= kHullLdsMaxH ? sizeof(int2) * (5 * (size_t)H + 2) : 0;
    for (int b0 = 0; b0 < n_frames; b0 += kMaskChunk) {
        const int nf = std::min(kMaskChunk, n_frames - b0);
        MaskFrames F{};
        for (int z = 0; z < nf; z++) {
            F.mask[z] = mask_dev[b0 + z];
            F.depth[z] = depth_dev[b0 + z];
            F.normal[z] = reinterpret_cast<float4 *>(normal_dev[b0 + z]);
            F.color[z] = color_dev ? reinterpret_cast<uchar4 *>(color_dev[b0 + z]) : nullptr;
            F.mask_out[z] = mask_out_dev ? mask_out_dev[b0 + z] : nullptr;
        }
        dim3 lg = lgrid, ag = agrid;
        lg.z = ag.z = nf;
        if (hull) {
            k_mask_label_local<<<lg, lblock, 0, ws->stream>>>(W, H, F, d_lab, d_cnt, d_best);
            k_mask_label_merge<<<lg, lblock, 0, ws->stream>>>(W, H, d_lab);
            k_mask_label_count<<<lg, lblock, 0, ws->stream>>>(W, H, d_lab, d_cnt);
            k_mask_argmax<<<dim3((unsigned)((HW + 255) / 256), nf), 256, 0, ws->stream>>>((int)HW, d_cnt, d_best);
            k_mask_rows<<<dim3((H + 3) / 4, nf), 256, 0, ws->stream>>>(W, H, d_lab, d_best, d_rows);
            k_mask_hull<<<nf, 256, hull_lds, ws->stream>>>(W, H, d_rows, d_stk, d_span);
            k_mask_apply<true><<<ag, ablock, 0, ws->stream>>>(W, H, r, F, d_span, d_roi, b0);
        } else {
            k_mask_apply<false><<<ag, ablock, 0, ws->stream>>>(W, H, r, F, nullptr, d_roi, b0);
        }
        HIP_TRY(hipGetLastError());
    }
    if (roi_out) {
        std::vector<int> h(4 * (size_t)n_frames);
        HIP_TRY(hipMemcpyAsync(h.data(), d_roi, sizeof(int) * h.size(), hipMemcpyDeviceToHost, ws->stream));
        HIP_TRY(hipStreamSynchronize(ws->stream));
        for (int f = 0; f < n_frames; f++) {
            roi_out[4 * f + 0] = (float)(9999 - h[4 * f + 0]);
            roi_out[4 * f + 1] = (float)h[4 * f + 1];
            roi_out[4 * f + 2] = (float)(9999 - h[4 * f + 2]);
            roi_out[4 * f + 3] = (float)h[4 * f + 3];
        }
    }
    return BTBA_OK;
}

}  // extern "C"

// ---- detector front end (btba_detect.hpp) ----------------------------------------------------------------------
namespace {
struct DetRoi { int umin, vmin, wc, hc; };

// the ROI rules shared by the three entry points: integral, non-negative, below 2^24 (exact in float), at least 1 x 1 after the
// crop, and inside the H x W image when that is known (H > 0)
bool det_roi(const float *r, int H, int W, DetRoi &o)
{
    for (int q = 0; q < 4; q++)
        if (!(r[q] >= 0.0f && r[q] < 16777216.0f) || r[q] != std::floor(r[q])) return false;
    o.umin = (int)r[0];
    o.vmin = (int)r[2];
    o.wc = (int)(r[1] - r[0]);
    o.hc = (int)(r[3] - r[2]);
    if (o.wc < 1 || o.hc < 1) return false;
    return H <= 0 || ((int64_t)o.umin + o.wc <= W && (int64_t)o.vmin + o.hc <= H);
}

bool det_params_ok(const btba_detector_params *p)
{
    return p && p->out_size >= 4 && p->out_size <= kDetMaxSize && p->out_size % 4 == 0;
}

// Lfnet::detectFeature's forward_transform (scale * translation, formed by Eigen's 3 x 3 product) and Eigen's cofactor inverse
// of it, in fp32 (include/btba.h)
void det_transform(int S, const float *roi, const DetRoi &r, float *fwd, float *bwd)
{
#pragma clang fp contract(off)
    const float s = (float)S / (float)std::max(r.wc, r.hc);
    const float su = s * roi[0], sv = s * roi[2];
    const float F[9] = { s, 0.0f, 0.0f - su, 0.0f, s, 0.0f - sv, 0.0f, 0.0f, 1.0f };
    const float det = s * s, invdet = 1.0f / det, r00 = s * invdet;
    const float B[9] = { r00, 0.0f, (su * s) * invdet, 0.0f, r00, (sv * s) * invdet, 0.0f, 0.0f, det * invdet };
    if (fwd) std::memcpy(fwd, F, sizeof F);
    if (bwd) std::memcpy(bwd, B, sizeof B);
}
}  // namespace

extern "C" {

void btba_detector_params_default(btba_detector_params *p)
{
    if (!p) return;
    p->out_size = 400;                                                // Lfnet::detectFeature's H_input = W_input (FeatureManager.cpp:851-852)
}

int btba_detector_transform(const btba_detector_params *prm, const float *roi, float *fwd, float *bwd)
{
    DetRoi r;
    if (!det_params_ok(prm) || !roi || !fwd || !bwd || !det_roi(roi, 0, 0, r)) return BTBA_EINVAL;
    det_transform(prm->out_size, roi, r, fwd, bwd);
    return BTBA_OK;
}

int btba_detector_inputs(btba_workspace *ws, const btba_detector_params *prm, int n_frames, int H, int W,
                         const uint8_t *const *color_dev, const float *roi_host, uint8_t *bgr_out_dev, float *gray_out_dev)
{
    // every argument is checked before the first HIP call
    if (!ws || !det_params_ok(prm) || n_frames < 1 || H < 1 || W < 1 || !color_dev || !roi_host ||
        misaligned(bgr_out_dev, 4) || misaligned(gray_out_dev, 16))
        return BTBA_EINVAL;
    std::vector<DetRoi> rois(n_frames);
    for (int f = 0; f < n_frames; f++)
        if (!color_dev[f] || misaligned(color_dev[f], 4) || !det_roi(roi_host + 4 * f, H, W, rois[f])) return BTBA_EINVAL;
    if (!bgr_out_dev && !gray_out_dev) return BTBA_OK;
    DeviceGuard device_guard(ws);
    const int S = prm->out_size;
    const dim3 block(64, 4), grid((S + 255) / 256, S / 4, 1);
    for (int b0 = 0; b0 < n_frames; b0 += kDetChunk) {
        const int nf = std::min(kDetChunk, n_frames - b0);
        DetectFrames F{};
        for (int z = 0; z < nf; z++) {
            const DetRoi &r = rois[b0 + z];
            F.color[z] = reinterpret_cast<const uchar4 *>(color_dev[b0 + z]) + ((size_t)r.vmin * W + r.umin);
            F.wc[z] = r.wc;
            F.hc[z] = r.hc;
        }
        dim3 g = grid;
        g.z = nf;
        k_detect_inputs<<<g, block, 0, ws->stream>>>(W, S, F, b0, bgr_out_dev, gray_out_dev);
        HIP_TRY(hipGetLastError());
    }
    return BTBA_OK;
}

int btba_detector_keypoints_to_image(btba_workspace *ws, const btba_detector_params *prm, int n_frames, const float *roi_host,
                                     const float *const *kpts_in_dev, const int32_t *n_kpts, float *const *kpts_out_dev)
{
    if (!ws || !det_params_ok(prm) || n_frames < 1 || !roi_host || !kpts_in_dev || !n_kpts || !kpts_out_dev) return BTBA_EINVAL;
    std::vector<float> bwd(9 * (size_t)n_frames);
    for (int f = 0; f < n_frames; f++) {
        DetRoi r;
        if (n_kpts[f] < 0 || n_kpts[f] > kDetMaxKpts || (n_kpts[f] > 0 && (!kpts_in_dev[f] || !kpts_out_dev[f])) ||
            misaligned(kpts_in_dev[f], 8) || misaligned(kpts_out_dev[f], 8) || !det_roi(roi_host + 4 * f, 0, 0, r))
            return BTBA_EINVAL;
        det_transform(prm->out_size, roi_host + 4 * f, r, nullptr, bwd.data() + 9 * f);
    }
    DeviceGuard device_guard(ws);
    for (int b0 = 0; b0 < n_frames; b0 += kDetChunk) {
        const int nf = std::min(kDetChunk, n_frames - b0);
        KptFrames F{};
        int n_max = 0;
        for (int z = 0; z < nf; z++) {
            const float *B = bwd.data() + 9 * (b0 + z);
            F.in[z] = reinterpret_cast<const float2 *>(kpts_in_dev[b0 + z]);
            F.out[z] = reinterpret_cast<float2 *>(kpts_out_dev[b0 + z]);
            F.n[z] = n_kpts[b0 + z];
            F.r00[z] = B[0]; F.r02[z] = B[2]; F.r11[z] = B[4]; F.r12[z] = B[5];
            n_max = std::max(n_max, F.n[z]);
        }
        if (n_max == 0) continue;
        k_detect_keypoints<<<dim3((n_max + 255) / 256, nf), 256, 0, ws->stream>>>(F);
        HIP_TRY(hipGetLastError());
    }
    return BTBA_OK;
}

}  // extern "C"
