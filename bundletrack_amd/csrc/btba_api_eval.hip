// btba_api_eval.hip -- host side of libbtba.so: pose-accuracy and NOCS evaluation.
#include "btba_host_common.hpp"
#include "btba_eval.hpp"
#include "btba_nocs.hpp"

extern "C" {

int btba_pose_errors(btba_workspace *ws, int device_resident, int n_models, const float *const *model_pts_dev, const int32_t *n_pts,
                     int n_evals, const int32_t *model_index, const float *poses_pred, const float *poses_gt,
                     float *add_out, float *adds_out)
{
    // every argument is checked before the first HIP call
    if (!ws || n_models < 1 || !model_pts_dev || !n_pts || n_evals < 0) return BTBA_EINVAL;
    for (int m = 0; m < n_models; m++)
        if (!model_pts_dev[m] || misaligned(model_pts_dev[m], 4) || n_pts[m] < 1 || n_pts[m] > BTBA_EVAL_MAX_POINTS)
            return BTBA_EINVAL;
    if (n_evals == 0) return BTBA_OK;
    if (!model_index || !poses_pred || !poses_gt || !add_out || !adds_out) return BTBA_EINVAL;
    for (int e = 0; e < n_evals; e++)
        if (model_index[e] < 0 || model_index[e] >= n_models) return BTBA_EINVAL;
    DeviceGuard device_guard(ws);

    // chunks: at most kEvalChunkEvals evaluations and kEvalScratchPoints per-point minima each
    std::vector<EvalRec> rec(n_evals);
    std::vector<int> chunk_start{ 0 };
    int64_t pts_in_chunk = 0, max_chunk_pts = 0;
    for (int e = 0; e < n_evals; e++) {
        const int n = n_pts[model_index[e]];
        if (e > chunk_start.back() && (pts_in_chunk + n > kEvalScratchPoints || e - chunk_start.back() >= kEvalChunkEvals)) {
            chunk_start.push_back(e);
            pts_in_chunk = 0;
        }
        rec[e] = EvalRec{ model_pts_dev[model_index[e]], n, (int)pts_in_chunk };
        pts_in_chunk += n;
        max_chunk_pts = std::max(max_chunk_pts, pts_in_chunk);
    }
    chunk_start.push_back(n_evals);
    const int max_chunk = std::min(n_evals, kEvalChunkEvals);
    const bool dev = device_resident != 0;
    Scratch S;
    const auto s_rec = S.add<EvalRec>(max_chunk);
    const auto s_pp = S.add<float>(16 * (size_t)max_chunk, !dev), s_pg = S.add<float>(16 * (size_t)max_chunk, !dev);
    const auto s_out = S.add<float>(2 * (size_t)max_chunk, !dev);
    const auto s_min = S.add<unsigned>((size_t)max_chunk_pts);
    int rc = S.bind(ws->eval);
    if (rc) return rc;
    EvalRec *d_rec = s_rec;
    unsigned *d_min = s_min;
    for (size_t c = 0; c + 1 < chunk_start.size(); c++) {
        const int e0 = chunk_start[c], ne = chunk_start[c + 1] - e0;
        int max_n = 0;
        for (int e = e0; e < e0 + ne; e++) max_n = std::max(max_n, rec[e].n);
        const float *pp = poses_pred + 16 * (size_t)e0, *pg = poses_gt + 16 * (size_t)e0;
        float *oa = add_out + e0, *os = adds_out + e0;
        HIP_TRY(hipMemcpyAsync(d_rec, rec.data() + e0, sizeof(EvalRec) * ne, hipMemcpyHostToDevice, ws->stream));
        if (!dev) {
            HIP_TRY(hipMemcpyAsync(s_pp, pp, sizeof(float) * 16 * ne, hipMemcpyHostToDevice, ws->stream));
            HIP_TRY(hipMemcpyAsync(s_pg, pg, sizeof(float) * 16 * ne, hipMemcpyHostToDevice, ws->stream));
            pp = s_pp;
            pg = s_pg;
            oa = s_out;
            os = oa + max_chunk;
        }
        // split the candidates when evaluations x query tiles cannot fill the chip (the result does not depend on it)
        const int tiles = (max_n + kEvalQTile - 1) / kEvalQTile;
        const int64_t wgs = (int64_t)ne * tiles;
        int splits = 1;
        if (wgs < 2048) splits = (int)std::min<int64_t>((2048 + wgs - 1) / wgs, (max_n + kEvalCTile - 1) / kEvalCTile);
        int per = (max_n + splits - 1) / splits;
        per = (per + kEvalCTile - 1) / kEvalCTile * kEvalCTile;
        splits = (max_n + per - 1) / per;
        if (splits > 1) HIP_TRY(hipMemsetAsync(d_min, 0xff, sizeof(unsigned) * (size_t)(rec[e0 + ne - 1].off + rec[e0 + ne - 1].n), ws->stream));
        k_eval_nn<<<dim3(ne, tiles, splits), kEvalThreads, 0, ws->stream>>>(d_rec, pp, pg, per, splits > 1 ? 1 : 0, d_min);
        k_eval_reduce<<<ne, kEvalRedThreads, 0, ws->stream>>>(d_rec, pp, pg, d_min, oa, os);
        HIP_TRY(hipGetLastError());
        if (!dev) {
            HIP_TRY(hipMemcpyAsync(add_out + e0, oa, sizeof(float) * ne, hipMemcpyDeviceToHost, ws->stream));
            HIP_TRY(hipMemcpyAsync(adds_out + e0, os, sizeof(float) * ne, hipMemcpyDeviceToHost, ws->stream));
        }
    }
    HIP_TRY(hipStreamSynchronize(ws->stream));                       // the host tables above may go
    return BTBA_OK;
}

void btba_nocs_params_default(btba_nocs_params *p)
{
    if (!p) return;
    p->rot_thresh_deg = 5.0;
    p->shift_thresh = 50.0;
    p->iou_thresh = 0.25;
    p->n_sym_steps = 20;
    p->flip_z180_pred = 1;
    p->normalize_columns = 1;
    p->clamp_acos = 0;
}

int btba_nocs_errors(btba_workspace *ws, const btba_nocs_params *params_in, int device_resident, int n_boxes, const double *boxes,
                     int n_evals, const int32_t *class_id, const int32_t *handle_visible, const int32_t *box_index,
                     const double *poses_pred, const double *poses_gt, double *theta_deg_out, double *shift_out, double *iou_out)
{
    // every argument is checked before the first HIP call
    btba_nocs_params prm;
    if (params_in) prm = *params_in; else btba_nocs_params_default(&prm);
    if (!ws || !boxes || n_boxes < 1 || n_boxes > (1 << 30) || n_evals < 0 || prm.n_sym_steps < 1 || prm.n_sym_steps > kNocsMaxSteps) return BTBA_EINVAL;
    if (n_evals == 0) return BTBA_OK;
    if (!class_id || !box_index || !poses_pred || !poses_gt || !theta_deg_out || !shift_out || !iou_out) return BTBA_EINVAL;
    const bool dev = device_resident != 0;
    if (dev && (misaligned(poses_pred, 8) || misaligned(poses_gt, 8) || misaligned(theta_deg_out, 8) || misaligned(shift_out, 8) || misaligned(iou_out, 8)))
        return BTBA_EINVAL;
    std::vector<int32_t> meta(n_evals);                     // box_index << 1 | rotation-symmetric
    for (int e = 0; e < n_evals; e++) {
        const int32_t c = class_id[e];
        if (c < 1 || c > 6 || box_index[e] < 0 || box_index[e] >= n_boxes) return BTBA_EINVAL;
        const bool sym = c == 1 || c == 2 || c == 4 || (c == 6 && handle_visible && handle_visible[e] == 0);
        meta[e] = box_index[e] << 1 | (sym ? 1 : 0);
    }
    double table[2 * kNocsMaxSteps] = {};                   // (cos, sin) of ((2 pi) i) / n_sym_steps: the bits every item rotates by
    for (int i = 0; i < prm.n_sym_steps; i++) {
        const double a = 2.0 * M_PI * (double)i / (double)prm.n_sym_steps;
        table[2 * i] = std::cos(a);
        table[2 * i + 1] = std::sin(a);
    }
    const int flags = (prm.flip_z180_pred ? kNocsFlip : 0) | (prm.normalize_columns ? kNocsNormalize : 0) | (prm.clamp_acos ? kNocsClamp : 0);
    DeviceGuard device_guard(ws);

    const int max_chunk = std::min(n_evals, kNocsChunkItems);
    Scratch S;
    const auto s_meta = S.add<int32_t>(max_chunk);
    const auto s_box = S.add<double>(24 * (size_t)n_boxes);
    const auto s_tab = S.add<double>(2 * kNocsMaxSteps);
    const auto s_pp = S.add<double>(16 * (size_t)max_chunk, !dev), s_pg = S.add<double>(16 * (size_t)max_chunk, !dev);
    const auto s_out = S.add<double>(3 * (size_t)max_chunk, !dev);
    int rc = S.bind(ws->nocs);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(s_box, boxes, sizeof(double) * 24 * (size_t)n_boxes, hipMemcpyHostToDevice, ws->stream));
    HIP_TRY(hipMemcpyAsync(s_tab, table, sizeof(table), hipMemcpyHostToDevice, ws->stream));
    for (int e0 = 0; e0 < n_evals; e0 += kNocsChunkItems) {
        const int ne = std::min(kNocsChunkItems, n_evals - e0);
        const double *pp = poses_pred + 16 * (size_t)e0, *pg = poses_gt + 16 * (size_t)e0;
        double *ot = theta_deg_out + e0, *os = shift_out + e0, *oi = iou_out + e0;
        HIP_TRY(hipMemcpyAsync(s_meta, meta.data() + e0, sizeof(int32_t) * ne, hipMemcpyHostToDevice, ws->stream));
        if (!dev) {
            HIP_TRY(hipMemcpyAsync(s_pp, pp, sizeof(double) * 16 * ne, hipMemcpyHostToDevice, ws->stream));
            HIP_TRY(hipMemcpyAsync(s_pg, pg, sizeof(double) * 16 * ne, hipMemcpyHostToDevice, ws->stream));
            pp = s_pp;
            pg = s_pg;
            ot = s_out;
            os = ot + max_chunk;
            oi = os + max_chunk;
        }
        k_nocs_errors<<<(ne + kNocsItems - 1) / kNocsItems, kNocsThreads, 0, ws->stream>>>(ne, s_meta, s_box, pp, pg, s_tab, prm.n_sym_steps, flags, ot, os, oi);
        HIP_TRY(hipGetLastError());
        if (!dev) {
            HIP_TRY(hipMemcpyAsync(theta_deg_out + e0, ot, sizeof(double) * ne, hipMemcpyDeviceToHost, ws->stream));
            HIP_TRY(hipMemcpyAsync(shift_out + e0, os, sizeof(double) * ne, hipMemcpyDeviceToHost, ws->stream));
            HIP_TRY(hipMemcpyAsync(iou_out + e0, oi, sizeof(double) * ne, hipMemcpyDeviceToHost, ws->stream));
        }
    }
    HIP_TRY(hipStreamSynchronize(ws->stream));                       // the host tables above may go
    return BTBA_OK;
}

}  // extern "C"
