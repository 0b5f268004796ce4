// btba_api_vos.hip -- host side of libbtba.so: mask propagation (the tracker's video segmentation).
#include "btba_host_common.hpp"
#include "btba_vos.hpp"

extern "C" {

void btba_vos_params_default(btba_vos_params *p)
{
    if (!p) return;
    p->ref_num = 9; p->range = 40;                                                // run_video.py:42-52
    p->sigma_dense = 8.0f; p->sigma_sparse = 21.0f; p->temperature = 1.0f;
    p->continuous_frames = 4; p->sparse_after = 15;                               // lib/predict.py:48-49
}

static bool vos_params_ok(const btba_vos_params *p)
{
    return p && p->continuous_frames >= 1 && p->ref_num >= p->continuous_frames - 1 && p->ref_num >= 1 && p->ref_num <= BTBA_VOS_MAX_REF &&
           p->range >= 0 && p->sparse_after >= 0 && p->sigma_dense > 0.0f && p->sigma_sparse > 0.0f && std::isfinite(p->temperature);
}

int btba_vos_sample_frames(const btba_vos_params *p, int frame_idx, int32_t *idx_out, int32_t *n_out, int32_t *n_dense_out)
{
    if (!vos_params_ok(p) || frame_idx < 1 || !idx_out || !n_out || !n_dense_out) return BTBA_EINVAL;
    int n = 0;
    if (frame_idx <= p->ref_num) {
        for (int i = 0; i < frame_idx; i++) idx_out[n++] = i;
    } else {
        const int dense_num = p->continuous_frames - 1, sparse_num = p->ref_num - dense_num;
        const int ref_end = frame_idx - dense_num - 1, ref_start = std::max(ref_end - p->range, 0);
        // np.linspace(ref_start, ref_end, sparse_num).astype(int): start + i * step in double, product and sum rounded separately, the last element the stop itself
        const double delta = (double)ref_end - (double)ref_start;
        const int div = sparse_num - 1;
        const double step = div > 0 ? delta / (double)div : 0.0;
        for (int i = 0; i < sparse_num; i++) {
            volatile double prod = div > 0 ? (step == 0.0 ? ((double)i / (double)div) * delta : (double)i * step) : (double)i * delta;
            double y = prod + (double)ref_start;
            if (sparse_num > 1 && i == sparse_num - 1) y = (double)ref_end;
            idx_out[n++] = (int32_t)y;
        }
        for (int j = 0; j < dense_num; j++) idx_out[n++] = frame_idx - dense_num + j;
    }
    *n_out = n;
    *n_dense_out = frame_idx > p->sparse_after ? std::min(p->continuous_frames, n) : n;       // predict:48-55: [-4:] of fewer than four is all of them
    return BTBA_OK;
}

int btba_vos_first_labels(btba_workspace *ws, int H, int W, int d, const uint8_t *label_dev, float *labels_out_dev)
{
    if (!ws || H < 1 || W < 1 || d < 2 || d > BTBA_VOS_MAX_CLASSES || !label_dev || !labels_out_dev || misaligned(labels_out_dev, 4)) return BTBA_EINVAL;
    const int Hd = (H + 7) / 8, Wd = (W + 7) / 8;
    if ((int64_t)Hd * Wd > BTBA_VOS_MAX_POSITIONS) return BTBA_EINVAL;
    DeviceGuard device_guard(ws);
    k_vos_first_labels<<<dim3((Wd + 63) / 64, (Hd + 3) / 4), dim3(64, 4), 0, ws->stream>>>(H, W, Hd, Wd, d, label_dev, labels_out_dev);
    HIP_TRY(hipGetLastError());
    return BTBA_OK;
}

int btba_vos_masks(btba_workspace *ws, int d, int Hd, int Wd, int H, int W, const float *pred_dev, uint8_t *mask_out_dev)
{
    if (!ws || d < 2 || d > BTBA_VOS_MAX_CLASSES || Hd < 1 || Wd < 1 || H < 1 || W < 1 || (int64_t)Hd * Wd > BTBA_VOS_MAX_POSITIONS ||
        (int64_t)H * W > INT32_MAX || !pred_dev || !mask_out_dev || misaligned(pred_dev, 4))
        return BTBA_EINVAL;
    DeviceGuard device_guard(ws);
    k_vos_masks<<<dim3((W + 63) / 64, (H + 3) / 4), dim3(64, 4), 0, ws->stream>>>(d, Hd, Wd, H, W, pred_dev, mask_out_dev);
    HIP_TRY(hipGetLastError());
    return BTBA_OK;
}

int btba_vos_inputs(btba_workspace *ws, int n_frames, int H, int W, const uint8_t *const *bgr_dev, float *rgb_out_dev)
{
    if (!ws || n_frames < 1 || H < 1 || W < 1 || (int64_t)H * W > INT32_MAX / 4 || !bgr_dev || !rgb_out_dev || misaligned(rgb_out_dev, 4)) return BTBA_EINVAL;
    for (int f = 0; f < n_frames; f++)
        if (!bgr_dev[f]) return BTBA_EINVAL;
    DeviceGuard device_guard(ws);
    const int n_px = H * W;
    for (int f0 = 0; f0 < n_frames; f0 += kVosInputChunk) {
        const int nf = std::min(kVosInputChunk, n_frames - f0);
        VosInputFrames F{};
        for (int z = 0; z < nf; z++) F.bgr[z] = bgr_dev[f0 + z];
        k_vos_inputs<<<dim3((n_px + 255) / 256, nf), 256, 0, ws->stream>>>(n_px, F, rgb_out_dev, f0);
        HIP_TRY(hipGetLastError());
    }
    return BTBA_OK;
}

int btba_vos_propagate(btba_workspace *ws, const btba_vos_params *prm, int n_items, int C, int d, int Hd, int Wd, const int32_t *n_ref,
                       const int32_t *n_dense, const float *const *ref_feat_dev, const float *const *ref_label_dev,
                       const float *const *target_dev, float *const *pred_out_dev, float *const *onehot_out_dev)
{
    // every argument is checked before the first HIP call
    if (!ws || !vos_params_ok(prm) || n_items < 1 || !n_ref || !n_dense || !ref_feat_dev || !ref_label_dev || !target_dev || !pred_out_dev) return BTBA_EINVAL;
    if (C < 8 || C > BTBA_VOS_MAX_CHANNELS || C % 8 != 0 || d < 2 || d > BTBA_VOS_MAX_CLASSES || Hd < 1 || Wd < 1 || (int64_t)Hd * Wd > BTBA_VOS_MAX_POSITIONS)
        return BTBA_EINVAL;
    size_t k = 0;
    for (int b = 0; b < n_items; b++) {
        if (n_ref[b] < 1 || n_ref[b] > BTBA_VOS_MAX_REF || n_dense[b] < 0 || n_dense[b] > n_ref[b]) return BTBA_EINVAL;
        if (!target_dev[b] || !pred_out_dev[b] || misaligned(target_dev[b], 4) || misaligned(pred_out_dev[b], 4) ||
            (onehot_out_dev && misaligned(onehot_out_dev[b], 4)))
            return BTBA_EINVAL;
        for (int r = 0; r < n_ref[b]; r++, k++)
            if (!ref_feat_dev[k] || !ref_label_dev[k] || misaligned(ref_feat_dev[k], 4) || misaligned(ref_label_dev[k], 4)) return BTBA_EINVAL;
    }
    DeviceGuard device_guard(ws);
    const int HW = Hd * Wd, NQ = C <= 256 ? 4 : 2, QT = 32 * NQ;
    Scratch sc;
    auto part = sc.add<float>(vos_part_floats(HW, d) * (size_t)n_items);
    if (int rc = sc.bind(ws->vos)) return rc;
    const size_t lds = sizeof(float) * std::max((size_t)C * QT, (size_t)kVosWaves * (2 + kVosMaxClasses) * QT);       // at most 128 KB
    if (!ws->vos_attr_set) {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_vos_partial<4>), hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_vos_partial<2>), hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
        ws->vos_attr_set = true;
    }
    const float sd2 = prm->sigma_dense * prm->sigma_dense, ss2 = prm->sigma_sparse * prm->sigma_sparse;
    k = 0;
    for (int b0 = 0; b0 < n_items; b0 += kVosChunk) {
        const int nb = std::min(kVosChunk, n_items - b0);
        VosItems I{};
        int max_split = 1;
        for (int z = 0; z < nb; z++) {
            const int b = b0 + z;
            for (int r = 0; r < n_ref[b]; r++, k++) { I.ref[z][r] = ref_feat_dev[k]; I.lab[z][r] = ref_label_dev[k]; }
            I.tgt[z] = target_dev[b];
            I.pred[z] = pred_out_dev[b];
            I.onehot[z] = onehot_out_dev ? onehot_out_dev[b] : nullptr;
            I.n_ref[z] = n_ref[b]; I.n_dense[z] = n_dense[b];
            I.n_split[z] = vos_splits(HW, n_ref[b], QT);
            max_split = std::max(max_split, (int)I.n_split[z]);
        }
        const dim3 grid((HW + QT - 1) / QT, max_split, nb);
        if (NQ == 4) k_vos_partial<4><<<grid, 64 * kVosWaves, lds, ws->stream>>>(I, C, d, Hd, Wd, prm->temperature, sd2, ss2, part, b0);
        else k_vos_partial<2><<<grid, 64 * kVosWaves, lds, ws->stream>>>(I, C, d, Hd, Wd, prm->temperature, sd2, ss2, part, b0);
        HIP_TRY(hipGetLastError());
        k_vos_merge<<<dim3((HW + 255) / 256, nb), 256, 0, ws->stream>>>(I, d, HW, part, b0);
        HIP_TRY(hipGetLastError());
    }
    return BTBA_OK;
}

}  // extern "C"
