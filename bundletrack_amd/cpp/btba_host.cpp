// btba_host.cpp -- see btba_host.hpp.  Plain C++17 on top of include/btba.h.
#include "btba_host.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <cmath>
#include <limits>
#include <set>

namespace btba {

OptimizerGpu::OptimizerGpu(std::shared_ptr<Config> yml1, void *hip_stream) : yml(std::move(yml1))
{
    if (!yml) yml = std::make_shared<Config>();
    // the structs of include/btba.h (btba_params, btba_stats, btba_zn_aux) carry no size field: a library built from another header version must
    // not be called with them
    if (btba_version() != BTBA_VERSION) throw Error(BTBA_EINVAL, "libbtba.so was built from another include/btba.h (btba_version() != BTBA_VERSION)");
    const int rc = btba_workspace_create_on_stream(&ws_, hip_stream);       // nullptr = the legacy NULL stream, as the reference
    if (rc != BTBA_OK) throw Error(rc, "btba_workspace_create_on_stream");
}

OptimizerGpu::~OptimizerGpu() { btba_workspace_destroy(ws_); }

void OptimizerGpu::optimizeFrames(const std::vector<EntryJ> &global_corres, const std::vector<int> &n_match_per_pair, int n_frames, int H, int W,
                                  const std::vector<float *> &depths_gpu, const std::vector<uchar4 *> & /*colors_gpu*/, const std::vector<float4 *> &normals_gpu,
                                  std::vector<Matrix4f> &poses, const Matrix3f &K)
{
    if ((int)depths_gpu.size() != n_frames || (int)normals_gpu.size() != n_frames || (int)poses.size() != n_frames) throw Error(BTBA_EINVAL, "optimizeFrames");
    btba_params prm;
    btba_params_default(&prm);
    prm.n_gn_iters = yml->num_iter_outter;                      // CUDASolverBundling.cpp:193
    prm.n_pcg_iters = yml->num_iter_inner;
    prm.robust_delta = yml->robust_delta;
    prm.image_downscale = yml->image_downscale;                 // LossGPU.cu:55
    prm.dense_dist_thresh = yml->p2p_max_dist;                  // CUDASolverBundling.cpp:93
    prm.dense_normal_thresh = std::cos(yml->p2p_max_normal_angle / 180.0 * M_PI);      // :94
    float Krm[9];
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) Krm[3 * r + c] = K(r, c);
    std::vector<float> P(16 * (size_t)n_frames);                // column-major Eigen -> row-major float4x4, LossGPU.cu:88-97
    for (int i = 0; i < n_frames; i++) for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) P[16 * (size_t)i + 4 * r + c] = poses[i](r, c);
    std::vector<const float *> depth(n_frames), nrm(n_frames);
    for (int i = 0; i < n_frames; i++) { depth[i] = depths_gpu[i]; nrm[i] = reinterpret_cast<const float *>(normals_gpu[i]); }
    // stored and never read by the reference (SBA.cpp:85): any length is legal there; only a vector of P = n(n-1)/2 segment
    // lengths is handed on (it lets the library skip its host pass), anything else is ignored
    const int *nm = ((long)n_match_per_pair.size() == (long)n_frames * (n_frames - 1) / 2) ? n_match_per_pair.data() : nullptr;
    int rc;
    if (persistent_frame_cache) {
        if ((int)frame_ids.size() != n_frames) throw Error(BTBA_EINVAL, "optimizeFrames: frame_ids");
        if (keyed_correspondences) prm.flags |= BTBA_FLAG_KEYED_CORR;
        rc = btba_optimize_frames_keyed(ws_, &prm, n_frames, H, W, Krm, global_corres.data(), (uint32_t)global_corres.size(), nm,
                                        depth.data(), nrm.data(), frame_ids.data(), nullptr, 0, P.data(), &last_stats);
    } else {
        rc = btba_optimize_frames(ws_, &prm, n_frames, H, W, Krm, global_corres.data(), (uint32_t)global_corres.size(), nm,
                                  depth.data(), nrm.data(), nullptr, 0, P.data(), &last_stats);
    }
    if (rc != BTBA_OK) throw Error(rc, "btba_optimize_frames");
    for (int i = 0; i < n_frames; i++) for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) poses[i](r, c) = P[16 * (size_t)i + 4 * r + c];      // :121-130
}

// Thin SVD of a 3x3 matrix S = U diag(sig) V^T by one-sided (Hestenes) Jacobi rotations on the columns, singular values
// sorted descending like Eigen::JacobiSVD; a vanishing third singular value (coplanar points) gets the cross product of
// the first two left vectors, so U stays orthonormal.
static void svd3(const float S[9], float U[9], float sig[3], float V[9])
{
    double A[9], W[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 1 };
    for (int k = 0; k < 9; k++) A[k] = S[k];
    for (int sweep = 0; sweep < 30; sweep++) {
        double off = 0.0;
        for (int p = 0; p < 2; p++)
            for (int q = p + 1; q < 3; q++) {
                double al = 0, be = 0, ga = 0;
                for (int k = 0; k < 3; k++) { al += A[3 * k + p] * A[3 * k + p]; be += A[3 * k + q] * A[3 * k + q]; ga += A[3 * k + p] * A[3 * k + q]; }
                if (ga == 0.0 || std::fabs(ga) <= 1e-15 * std::sqrt(al * be)) continue;
                off = std::max(off, std::fabs(ga) / std::sqrt(al * be));
                const double zeta = (be - al) / (2.0 * ga);
                const double t = (zeta >= 0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / std::sqrt(1.0 + t * t), sn = c * t;
                for (int k = 0; k < 3; k++) {
                    const double ap = A[3 * k + p], aq = A[3 * k + q];
                    A[3 * k + p] = c * ap - sn * aq; A[3 * k + q] = sn * ap + c * aq;
                    const double wp = W[3 * k + p], wq = W[3 * k + q];
                    W[3 * k + p] = c * wp - sn * wq; W[3 * k + q] = sn * wp + c * wq;
                }
            }
        if (off < 1e-14) break;
    }
    double norm[3];
    int order[3] = { 0, 1, 2 };
    for (int j = 0; j < 3; j++) norm[j] = std::sqrt(A[j] * A[j] + A[3 + j] * A[3 + j] + A[6 + j] * A[6 + j]);
    std::sort(order, order + 3, [&](int a, int b) { return norm[a] > norm[b]; });
    double Ud[9];
    for (int j = 0; j < 3; j++) {
        const int o = order[j];
        sig[j] = (float)norm[o];
        for (int k = 0; k < 3; k++) { V[3 * k + j] = (float)W[3 * k + o]; Ud[3 * k + j] = norm[o] > 0 ? A[3 * k + o] / norm[o] : 0.0; }
    }
    if (norm[order[2]] <= 1e-12 * norm[order[0]]) {                   // rank 2: complete U with u0 x u1
        Ud[2] = Ud[3] * Ud[7] - Ud[6] * Ud[4]; Ud[5] = Ud[6] * Ud[1] - Ud[0] * Ud[7]; Ud[8] = Ud[0] * Ud[4] - Ud[3] * Ud[1];
    }
    for (int k = 0; k < 9; k++) U[k] = (float)Ud[k];
}

void solveRigidTransformBetweenPoints(const std::vector<float> &points1, const std::vector<float> &points2, Matrix4f &pose)
{
    pose = Matrix4f::Identity();
    const size_t n = points1.size() / 3;
    if (n < 3 || points1.size() != points2.size() || points1.size() % 3) return;      // the reference asserts
    float m1[3] = { 0, 0, 0 }, m2[3] = { 0, 0, 0 };
    for (size_t i = 0; i < n; i++) for (int c = 0; c < 3; c++) { m1[c] += points1[3 * i + c]; m2[c] += points2[3 * i + c]; }
    for (int c = 0; c < 3; c++) { m1[c] /= (float)n; m2[c] /= (float)n; }
    float S[9] = {};                                                  // P^T Q, row-major
    for (size_t i = 0; i < n; i++)
        for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) S[3 * r + c] += (points1[3 * i + r] - m1[r]) * (points2[3 * i + c] - m2[c]);
    for (float v : S) if (!std::isfinite(v)) return;
    float U[9], sig[3], V[9];
    svd3(S, U, sig, V);
    auto vut = [&](float R[9]) { for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) { R[3 * r + c] = 0; for (int k = 0; k < 3; k++) R[3 * r + c] += V[3 * r + k] * U[3 * c + k]; } };
    float R[9];
    vut(R);
    for (int r = 0; r < 3; r++)                                        // (R^T R).isApprox(I), float precision
        for (int c = 0; c < 3; c++) {
            float d = 0;
            for (int k = 0; k < 3; k++) d += R[3 * k + r] * R[3 * k + c];
            if (std::fabs(d - (r == c ? 1.0f : 0.0f)) > 1e-5f) return;
        }
    const float det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
    if (det < 0) { for (int k = 0; k < 3; k++) V[3 * k + 2] = -V[3 * k + 2]; vut(R); }
    Matrix4f out = Matrix4f::Identity();
    for (int r = 0; r < 3; r++) {
        float t = m2[r];
        for (int c = 0; c < 3; c++) { out(r, c) = R[3 * r + c]; t -= R[3 * r + c] * m1[c]; }
        out(r, 3) = t;
    }
    for (float v : out.d) if (!std::isfinite(v)) return;
    pose = out;
}

void poseErrors(btba_workspace *ws, const std::vector<const float *> &models_dev, const std::vector<int32_t> &n_pts,
                const std::vector<int32_t> &model_index, const std::vector<Matrix4f> &poses_pred, const std::vector<Matrix4f> &poses_gt,
                std::vector<float> &add, std::vector<float> &adds)
{
    const size_t n = model_index.size();
    if (models_dev.size() != n_pts.size() || poses_pred.size() != n || poses_gt.size() != n) throw Error(BTBA_EINVAL, "poseErrors: sizes differ");
    std::vector<float> pp(16 * n), pg(16 * n);                    // row-major, as the C ABI takes them
    for (size_t e = 0; e < n; e++)
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) {
                pp[16 * e + 4 * r + c] = poses_pred[e](r, c);
                pg[16 * e + 4 * r + c] = poses_gt[e](r, c);
            }
    add.assign(n, 0.0f);
    adds.assign(n, 0.0f);
    const int rc = btba_pose_errors(ws, /*device_resident=*/0, (int)models_dev.size(), models_dev.data(), n_pts.data(), (int)n, model_index.data(),
                                    pp.data(), pg.data(), add.data(), adds.data());
    if (rc != BTBA_OK) throw Error(rc, "btba_pose_errors");
}

btba_nocs_params nocsParams()
{
    btba_nocs_params p;
    btba_nocs_params_default(&p);
    return p;
}

void nocsErrors(btba_workspace *ws, const btba_nocs_params &params, const std::vector<NocsBox> &boxes, const std::vector<int32_t> &class_id,
                const std::vector<int32_t> &handle_visible, const std::vector<int32_t> &box_index, const std::vector<Matrix4d> &poses_pred,
                const std::vector<Matrix4d> &poses_gt, std::vector<double> &theta_deg, std::vector<double> &shift, std::vector<double> &iou)
{
    const size_t n = class_id.size();
    if (box_index.size() != n || poses_pred.size() != n || poses_gt.size() != n || (!handle_visible.empty() && handle_visible.size() != n))
        throw Error(BTBA_EINVAL, "nocsErrors: sizes differ");
    std::vector<double> pp(16 * n), pg(16 * n);                   // row-major, as the C ABI takes them
    for (size_t e = 0; e < n; e++)
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) {
                pp[16 * e + 4 * r + c] = poses_pred[e](r, c);
                pg[16 * e + 4 * r + c] = poses_gt[e](r, c);
            }
    theta_deg.assign(n, 0.0);
    shift.assign(n, 0.0);
    iou.assign(n, 0.0);
    const int rc = btba_nocs_errors(ws, &params, /*device_resident=*/0, (int)boxes.size(), boxes.empty() ? nullptr : boxes[0].data(), (int)n,
                                    class_id.data(), handle_visible.empty() ? nullptr : handle_visible.data(), box_index.data(), pp.data(),
                                    pg.data(), theta_deg.data(), shift.data(), iou.data());
    if (rc != BTBA_OK) throw Error(rc, "btba_nocs_errors");
}

NocsReport nocsReport(const std::vector<double> &theta_deg, const std::vector<double> &shift, const std::vector<double> &iou,
                      const std::vector<int32_t> &class_id, const std::vector<int64_t> &n_listed, const btba_nocs_params &params)
{
    const size_t n = class_id.size();
    if (theta_deg.size() != n || shift.size() != n || iou.size() != n || (!n_listed.empty() && n_listed.size() != 6))
        throw Error(BTBA_EINVAL, "nocsReport: sizes differ");
    const double nan = std::numeric_limits<double>::quiet_NaN();
    NocsReport rep;
    double acc55 = 0.0, acc25 = 0.0, acc_rot = 0.0, acc_trans = 0.0;
    for (int c = 1; c <= 6; c++) {
        int64_t items = 0, in55 = 0, over = 0, n_rot = 0;
        double sum_rot = 0.0, sum_trans = 0.0;
        for (size_t e = 0; e < n; e++) {
            if (class_id[e] != c) continue;
            items++;
            if (theta_deg[e] < params.rot_thresh_deg && shift[e] < params.shift_thresh) in55++;
            if (iou[e] > params.iou_thresh) {
                over++;
                sum_trans += shift[e];
                if (theta_deg[e] < 360.0) { sum_rot += theta_deg[e]; n_rot++; }
            }
        }
        NocsRow &row = rep.cls[c - 1];
        row.n = n_listed.empty() ? items : n_listed[c - 1];
        rep.overall.n += row.n;
        const double s55 = row.n ? (double)in55 / (double)row.n : nan, s25 = row.n ? (double)over / (double)row.n : nan;
        row.rot_err_deg = n_rot ? sum_rot / (double)n_rot : nan;
        row.trans_err = over ? sum_trans / (double)over : nan;
        acc55 = acc55 + s55 / 6;
        acc25 = acc25 + s25 / 6;
        acc_rot = acc_rot + row.rot_err_deg / 6;
        acc_trans = acc_trans + row.trans_err / 6;
        row.acc_5deg5cm = s55 * 100;
        row.acc_iou25 = s25 * 100;
        row.trans_err_cm = row.trans_err / 10;
    }
    rep.overall.acc_5deg5cm = acc55 * 100;
    rep.overall.acc_iou25 = acc25 * 100;
    rep.overall.rot_err_deg = acc_rot;
    rep.overall.trans_err = acc_trans;
    rep.overall.trans_err_cm = acc_trans / 10;
    return rep;
}

WindowLayout windowLayout(int n_frames, const std::vector<int32_t> &seg_counts, const std::vector<int32_t> &newframe_index, int min_fm_edges_newframe)
{
    const int P = n_frames >= 2 ? n_frames * (n_frames - 1) / 2 : 0;
    const size_t nw = newframe_index.size();
    if (nw == 0 || P == 0 || seg_counts.size() != nw * (size_t)P) throw Error(BTBA_EINVAL, "windowLayout: sizes differ");
    WindowLayout L;
    L.pair_offsets.assign(nw * (size_t)(P + 1), 0u);
    L.n_edges_newframe.assign(nw, 0);
    L.run_ba.assign(nw, 0);
    const int rc = btba_window_layout((int)nw, n_frames, seg_counts.data(), newframe_index.data(), min_fm_edges_newframe, &L.corr_stride,
                                      &L.max_corr_per_pair, L.pair_offsets.data(), L.n_edges_newframe.data(), L.run_ba.data());
    if (rc != BTBA_OK) throw Error(rc, "btba_window_layout");
    return L;
}

void marshalWindows(btba_workspace *ws, int n_windows, int n_frames, const btba_match *matches_dev, int64_t n_records, const uint32_t *segments_dev,
                    const WindowLayout &layout, btba_entryj *corr_dev, uint32_t *pair_offsets_dev, float *corr24_dev)
{
    const int rc = btba_marshal_windows(ws, n_windows, n_frames, matches_dev, n_records, segments_dev, layout.max_corr_per_pair,
                                        std::max<int64_t>(layout.corr_stride, 1), corr_dev, pair_offsets_dev, corr24_dev);
    if (rc != BTBA_OK) throw Error(rc, "btba_marshal_windows");
}

void procrustesPairs(btba_workspace *ws, const btba_match *matches_dev, int64_t n_records, const std::vector<std::pair<int32_t, int32_t>> &segments,
                     const std::vector<Matrix4f> &posesA, const std::vector<Matrix4f> &posesB, std::vector<Matrix4f> &poses, std::vector<float> &err)
{
    const size_t n = segments.size();
    if (posesA.size() != n || posesB.size() != n) throw Error(BTBA_EINVAL, "procrustesPairs: sizes differ");
    std::vector<int32_t> seg(2 * n);
    std::vector<float> pa(16 * n), pb(16 * n), out(16 * n);       // row-major, as the C ABI takes them
    for (size_t e = 0; e < n; e++) {
        seg[2 * e] = segments[e].first;
        seg[2 * e + 1] = segments[e].second;
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) {
                pa[16 * e + 4 * r + c] = posesA[e](r, c);
                pb[16 * e + 4 * r + c] = posesB[e](r, c);
            }
    }
    err.assign(n, 0.0f);
    const int rc = btba_procrustes_pairs(ws, /*device_resident=*/0, (int)n, matches_dev, n_records, seg.data(), pa.data(), pb.data(), out.data(),
                                         err.data(), nullptr);
    if (rc != BTBA_OK) throw Error(rc, "btba_procrustes_pairs");
    poses.resize(n);
    for (size_t e = 0; e < n; e++)
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) poses[e](r, c) = out[16 * e + 4 * r + c];
}

void linearizeBatchZn(btba_workspace *ws, const btba_params &params, int n_instances, int n_frames, int H, int W, const Matrix3f &K, const float *zn_dev,
                      const btba_zn_aux *aux, const btba_entryj *corr_dev, int64_t corr_stride, const uint32_t *pair_offsets_dev, uint32_t max_corr_per_pair,
                      const std::vector<std::pair<int32_t, int32_t>> &dense_pairs, const float *poses_dev, float *info_dev, float *rhs_dev)
{
    float Kr[9];                                                  // row-major, as the C ABI takes it
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) Kr[3 * r + c] = K(r, c);
    std::vector<int32_t> dp;
    for (const auto &p : dense_pairs) { dp.push_back(p.first); dp.push_back(p.second); }
    const int rc = btba_linearize_batch_zn_aux(ws, &params, n_instances, n_frames, H, W, Kr, zn_dev, aux, corr_dev, corr_stride, pair_offsets_dev,
                                               max_corr_per_pair, dp.empty() ? nullptr : dp.data(), (int)dense_pairs.size(), poses_dev, info_dev, rhs_dev);
    if (rc != BTBA_OK) throw Error(rc, "btba_linearize_batch_zn_aux");
}

void poseCovariances(btba_workspace *ws, int n_instances, int n_frames, const float *info_dev, double *cov_blocks_dev, int32_t *status_dev,
                     double *cov_full_dev, double *pivot_ratio_dev)
{
    const int64_t na = 6 * ((int64_t)n_frames - 1);
    const int rc = btba_pose_covariances(ws, n_instances, n_frames, info_dev, na * na, cov_blocks_dev, cov_full_dev, pivot_ratio_dev, status_dev);
    if (rc != BTBA_OK) throw Error(rc, "btba_pose_covariances");
}

void objectiveBatchZn(btba_workspace *ws, const btba_params &params, int n_instances, int n_frames, int H, int W, const Matrix3f &K, const float *zn_dev,
                      const btba_zn_aux *aux, const btba_entryj *corr_dev, int64_t corr_stride, const uint32_t *pair_offsets_dev, uint32_t max_corr_per_pair,
                      const std::vector<std::pair<int32_t, int32_t>> &dense_pairs, const float *poses_dev, btba_objective_total *total_dev,
                      btba_objective_pair *sparse_dev, btba_objective_pair *dense_dev)
{
    float Kr[9];                                                  // row-major, as the C ABI takes it
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) Kr[3 * r + c] = K(r, c);
    std::vector<int32_t> dp;
    for (const auto &p : dense_pairs) { dp.push_back(p.first); dp.push_back(p.second); }
    const int rc = btba_objective_batch_zn_aux(ws, &params, n_instances, n_frames, H, W, Kr, zn_dev, aux, corr_dev, corr_stride, pair_offsets_dev,
                                               max_corr_per_pair, dp.empty() ? nullptr : dp.data(), (int)dense_pairs.size(), poses_dev, total_dev, sparse_dev, dense_dev);
    if (rc != BTBA_OK) throw Error(rc, "btba_objective_batch_zn_aux");
}

double residualVariance(const btba_objective_total &total, int n_frames)
{
    const double dof = (double)total.n_residuals - 6.0 * (double)(n_frames - 1);
    return dof > 0.0 ? total.objective / dof : std::numeric_limits<double>::quiet_NaN();
}

static btba_fuse_segment fuseSegment(int kind, int instance, const Matrix4f &pose, const void *geom, int64_t n, const void *normal, const void *colour)
{
    btba_fuse_segment s{};
    s.kind = kind;
    s.instance = instance;
    s.n = n;
    s.geom = geom;
    s.normal = normal;
    s.colour = colour;
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) s.pose[4 * r + c] = pose(r, c);          // row-major, as the C ABI takes it
    return s;
}

btba_fuse_segment frameSegment(int instance, const Matrix4f &pose_in_model, const float *depth_gpu, const float4 *normal_gpu, const uchar4 *color_gpu)
{
    return fuseSegment(BTBA_FUSE_FRAME, instance, pose_in_model, depth_gpu, 0, normal_gpu, color_gpu);
}

btba_fuse_segment pointSegment(int instance, const Matrix4f &pose, const float4 *xyz_gpu, int64_t n, const float4 *normal_gpu, const uchar4 *color_gpu)
{
    return fuseSegment(BTBA_FUSE_POINTS, instance, pose, xyz_gpu, n, normal_gpu, color_gpu);
}

void fuseBounds(btba_workspace *ws, const btba_fuse_params &params, int n_instances, const std::vector<btba_fuse_segment> &segments, int H, int W,
                const Matrix3f &K, int32_t *box_dev)
{
    float Kr[9];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) Kr[3 * r + c] = K(r, c);
    const int rc = btba_fuse_bounds(ws, &params, n_instances, (int)segments.size(), segments.data(), H, W, Kr, box_dev);
    if (rc != BTBA_OK) throw Error(rc, "btba_fuse_bounds");
}

void fuseFrames(btba_workspace *ws, const btba_fuse_params &params, int n_instances, const std::vector<btba_fuse_segment> &segments, int H, int W,
                const Matrix3f &K, const std::vector<int32_t> &box, const ObjectCloudBuffers &out)
{
    if (box.size() != 6 * (size_t)std::max(n_instances, 0)) throw Error(BTBA_EINVAL, "fuseFrames: box");
    float Kr[9];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) Kr[3 * r + c] = K(r, c);
    const int rc = btba_fuse_frames(ws, &params, n_instances, (int)segments.size(), segments.data(), H, W, Kr, box.data(), out.capacity,
                                    reinterpret_cast<float *>(out.xyz), reinterpret_cast<float *>(out.normal), reinterpret_cast<uint8_t *>(out.colour),
                                    out.count, out.lin, out.n_out, out.n_outside, out.status);
    if (rc != BTBA_OK) throw Error(rc, "btba_fuse_frames");
}

void voxelDownsample(btba_workspace *ws, const btba_fuse_params &params, const std::vector<const float4 *> &xyz_gpu, const std::vector<int64_t> &n_points,
                     const std::vector<int32_t> &box, const ObjectCloudBuffers &out, const std::vector<const float4 *> &normal_gpu,
                     const std::vector<const uchar4 *> &color_gpu)
{
    const size_t B = xyz_gpu.size();
    if (n_points.size() != B || box.size() != 6 * B || (!normal_gpu.empty() && normal_gpu.size() != B) || (!color_gpu.empty() && color_gpu.size() != B))
        throw Error(BTBA_EINVAL, "voxelDownsample: one entry per instance");
    const int rc = btba_voxel_downsample(ws, &params, (int)B, reinterpret_cast<const float *const *>(xyz_gpu.data()),
                                         normal_gpu.empty() ? nullptr : reinterpret_cast<const float *const *>(normal_gpu.data()),
                                         color_gpu.empty() ? nullptr : reinterpret_cast<const uint8_t *const *>(color_gpu.data()), n_points.data(), box.data(),
                                         out.capacity, reinterpret_cast<float *>(out.xyz), reinterpret_cast<float *>(out.normal),
                                         reinterpret_cast<uint8_t *>(out.colour), out.count, out.lin, out.n_out, out.n_outside, out.status);
    if (rc != BTBA_OK) throw Error(rc, "btba_voxel_downsample");
}

DeviceKeyframeMemory::DeviceKeyframeMemory(btba_workspace *ws, int n_sessions, int capacity, int max_BA_frames, float min_rot_deg1, int min_feat_num1)
    : min_rot_deg(min_rot_deg1), min_feat_num(min_feat_num1), n_sessions_(n_sessions), capacity_(capacity), max_BA_(max_BA_frames)
{
    const int rc = btba_keyframes_create(ws, n_sessions, capacity, max_BA_frames, &kf_);
    if (rc != BTBA_OK) throw Error(rc, "btba_keyframes_create");
}

DeviceKeyframeMemory::~DeviceKeyframeMemory() { btba_keyframes_destroy(kf_); }

DeviceKeyframeMemory::DeviceKeyframeMemory(DeviceKeyframeMemory &&o) noexcept
    : min_rot_deg(o.min_rot_deg), min_feat_num(o.min_feat_num), kf_(o.kf_), n_sessions_(o.n_sessions_), capacity_(o.capacity_), max_BA_(o.max_BA_)
{
    o.kf_ = nullptr;
}

void DeviceKeyframeMemory::reset(int session)
{
    const int rc = btba_keyframes_reset(kf_, session);
    if (rc != BTBA_OK) throw Error(rc, "btba_keyframes_reset");
}

void DeviceKeyframeMemory::checkAndAddKeyframes(const float *pose_dev, const int32_t *frame_id_dev, const uint64_t *frame_key_dev, const int32_t *status_other_dev,
                                                const int32_t *n_keypts_dev, int32_t *added_out_dev, const int32_t *active_dev)
{
    const int rc = btba_keyframes_check_add(kf_, min_rot_deg, min_feat_num, active_dev, pose_dev, frame_id_dev, frame_key_dev, status_other_dev, n_keypts_dev,
                                            added_out_dev);
    if (rc != BTBA_OK) throw Error(rc, "btba_keyframes_check_add");
}

void DeviceKeyframeMemory::selectKeyFramesForBA(const float *newpose_dev, const int32_t *new_frame_id_dev, const uint64_t *new_frame_key_dev,
                                                const KeyframeWindows &out, const int32_t *active_dev)
{
    const int rc = btba_keyframes_select(kf_, active_dev, newpose_dev, new_frame_id_dev, new_frame_key_dev, out.n_window, out.slot, out.frame_id, out.frame_key,
                                         out.pose, out.newframe_index);
    if (rc != BTBA_OK) throw Error(rc, "btba_keyframes_select");
}

void DeviceKeyframeMemory::writeback(const int32_t *n_window_dev, const int32_t *window_slot_dev, const float *pose_dev, const int32_t *active_dev)
{
    const int rc = btba_keyframes_writeback(kf_, active_dev, n_window_dev, window_slot_dev, pose_dev);
    if (rc != BTBA_OK) throw Error(rc, "btba_keyframes_writeback");
}

KeyframePools DeviceKeyframeMemory::exportPools()
{
    KeyframePools p;
    const size_t S = (size_t)n_sessions_, SC = S * (size_t)capacity_;
    p.count.resize(S); p.overflow.resize(S); p.frame_id.resize(SC); p.frame_key.resize(SC); p.poses.resize(16 * SC);
    const int rc = btba_keyframes_export(kf_, p.count.data(), p.overflow.data(), p.frame_id.data(), p.frame_key.data(), p.poses.data());
    if (rc != BTBA_OK) throw Error(rc, "btba_keyframes_export");
    return p;
}

void rotationDistances(btba_workspace *ws, int n, const float *A_dev, const float *B_dev, float *dist_out_dev)
{
    const int rc = btba_rotation_distances(ws, n, A_dev, B_dev, dist_out_dev);
    if (rc != BTBA_OK) throw Error(rc, "btba_rotation_distances");
}

void registerIndex(btba_workspace *ws, int n_instances, const std::vector<int32_t> &box, const ObjectCloudBuffers &cloud, int32_t *cell_index_dev)
{
    if (box.size() != 6 * (size_t)std::max(n_instances, 0)) throw Error(BTBA_EINVAL, "registerIndex: box");
    const int rc = btba_register_index(ws, n_instances, box.data(), cloud.capacity, cloud.lin, cloud.n_out, cell_index_dev);
    if (rc != BTBA_OK) throw Error(rc, "btba_register_index");
}

void registerFrames(btba_workspace *ws, const btba_register_params &params, int n_instances, const std::vector<btba_fuse_segment> &items, int H, int W,
                    const Matrix3f &K, const std::vector<int32_t> &box, const ObjectCloudBuffers &cloud, const int32_t *cell_index_dev, float *pose_out_dev,
                    btba_register_result *result_dev, btba_register_iter *trace_dev)
{
    if (box.size() != 6 * (size_t)std::max(n_instances, 0)) throw Error(BTBA_EINVAL, "registerFrames: box");
    float Kr[9];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) Kr[3 * r + c] = K(r, c);
    const int rc = btba_register_frames(ws, &params, n_instances, (int)items.size(), items.data(), H, W, Kr, box.data(), cloud.capacity,
                                        reinterpret_cast<const float *>(cloud.xyz), reinterpret_cast<const float *>(cloud.normal), cell_index_dev, pose_out_dev,
                                        result_dev, trace_dev);
    if (rc != BTBA_OK) throw Error(rc, "btba_register_frames");
}

double vocapAuc(const std::vector<double> &errors, double max_threshold)
{
    const size_t n = errors.size();
    std::vector<double> b;                                        // the errors strictly below the threshold (NaN never is), sorted
    for (double x : errors)
        if (x < max_threshold) b.push_back(x);
    const size_t m = b.size();
    if (m == 0) return 0.0;
    std::sort(b.begin(), b.end());
    double area = 0.0, prev = 0.0;
    for (size_t k = 1; k <= m; k++)
        if (b[k - 1] != prev) {
            area += (b[k - 1] - prev) * (double)k / (double)n;
            prev = b[k - 1];
        }
    area += (max_threshold - prev) * (double)m / (double)n;
    return area / max_threshold;
}

std::string formatPoseTxt(const Matrix4f &M)
{
    char cell[16][32];
    size_t width = 0;
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) {
            std::snprintf(cell[4 * r + c], sizeof cell[0], "%.10g", (double)M(r, c));
            width = std::max(width, std::strlen(cell[4 * r + c]));
        }
    std::string out;
    for (int r = 0; r < 4; r++) {
        for (int c = 0; c < 4; c++) {
            if (c) out += ' ';
            out.append(width - std::strlen(cell[4 * r + c]), ' ');
            out += cell[4 * r + c];
        }
        out += '\n';
    }
    return out;
}

float rotationGeodesicDistance(const Matrix4f &A, const Matrix4f &B)
{
    // trace(R1 R2^T): diagonal entry i is the dot product of row i of R1 with row i of R2, each summed left to right and then the
    // three of them (the shape of Eigen's coefficient-based 3 x 3 product; oracle/btba_oracle_keyframes.c sums the same way)
    float tr = 0.0f;
    for (int i = 0; i < 3; i++) {
        float dot = A(i, 0) * B(i, 0);
        dot += A(i, 1) * B(i, 1);
        dot += A(i, 2) * B(i, 2);
        tr = i == 0 ? dot : tr + dot;
    }
    float tmp = (tr - 1.0f) / 2.0f;
    tmp = std::max(std::min(1.0f, tmp), -1.0f);
    return std::acos(tmp);
}

Window marshalWindow(std::vector<std::shared_ptr<Frame>> local_frames, const std::map<std::pair<int, int>, Correspondences> &matches,
                     const std::shared_ptr<Frame> &newframe, int min_fm_edges_newframe)
{
    Window w;
    std::sort(local_frames.begin(), local_frames.end(), [](const std::shared_ptr<Frame> &a, const std::shared_ptr<Frame> &b) { return a->_id < b->_id; });   // :286
    for (size_t i = 0; i < local_frames.size(); i++)
        for (size_t j = i + 1; j < local_frames.size(); j++) {
            const auto &frameA = local_frames[j], &frameB = local_frames[i];
            const auto it = matches.find({ frameA->_id, frameB->_id });
            int m = 0;
            if (it != matches.end()) {
                m = (int)(it->second.ptA_cam.size() / 3);
                for (int k = 0; k < m; k++) {
                    EntryJ e;
                    e.imgIdx_i = (uint32_t)i; e.imgIdx_j = (uint32_t)j;                      // :311-316: pos_j = ptA, pos_i = ptB
                    for (int c = 0; c < 3; c++) { e.pos_j[c] = it->second.ptA_cam[3 * k + c]; e.pos_i[c] = it->second.ptB_cam[3 * k + c]; }
                    w.global_corres.push_back(e);
                    if (frameA == newframe || frameB == newframe) w.n_edges_newframe++;
                }
            }
            w.n_match_per_pair.push_back(m);
        }
    w.frames = std::move(local_frames);
    w.run_ba = w.n_edges_newframe > min_fm_edges_newframe;
    if (!w.run_ba) newframe->_status = Frame::NO_BA;
    return w;
}

bool KeyframeMemory::checkAndAddKeyframe(const std::shared_ptr<Frame> &frame)
{
    if (frame->_id == 0) { _keyframes.push_back(frame); return true; }
    if (frame->_status != Frame::OTHER) return false;
    if (frame->_n_keypts < yml->keyframe_min_feat_num) return false;
    for (const auto &kf : _keyframes) {
        float rot_diff = rotationGeodesicDistance(frame->_pose_in_model, kf->_pose_in_model);
        rot_diff = (float)((double)(rot_diff * 180.0f) / M_PI);          // rot_diff*180/M_PI: the product in float, the division in double, stored as float (:208)
        if (rot_diff < yml->keyframe_min_rot) return false;
    }
    _keyframes.push_back(frame);
    return true;
}

std::vector<std::shared_ptr<Frame>> KeyframeMemory::selectKeyFramesForBA(const std::shared_ptr<Frame> &newframe)
{
    // The reference keeps the chosen set in a std::set<std::shared_ptr<Frame>>: ordered by the frames' ADDRESSES, which decides the order cum_dist is
    // summed in and nothing else (Bundler.cpp:252-256; the caller sorts by id, :286).  Here the set is ordered by frame id -- what an allocator that
    // hands out ascending addresses gives the reference -- so a selection does not depend on where the heap put a frame.
    auto by_id = [](const std::shared_ptr<Frame> &a, const std::shared_ptr<Frame> &b) { return a->_id < b->_id; };
    std::vector<std::shared_ptr<Frame>> frames = { newframe };
    auto has = [&](const std::shared_ptr<Frame> &f) { return std::find(frames.begin(), frames.end(), f) != frames.end(); };
    auto insert = [&](const std::shared_ptr<Frame> &f) { if (!has(f)) frames.insert(std::upper_bound(frames.begin(), frames.end(), f, by_id), f); };
    if ((int)(_keyframes.size() + frames.size()) <= yml->max_BA_frames) {
        for (const auto &kf : _keyframes) insert(kf);
        return frames;
    }
    insert(_keyframes[0]);
    while ((int)frames.size() < yml->max_BA_frames) {                // "greedy_rot"
        float best_dist = std::numeric_limits<float>::max();
        std::shared_ptr<Frame> best_kf;
        for (const auto &kf : _keyframes) {
            if (has(kf)) continue;
            float cum_dist = 0.0f;
            for (const auto &f : frames) cum_dist += rotationGeodesicDistance(kf->_pose_in_model, f->_pose_in_model);
            if (cum_dist < best_dist) { best_dist = cum_dist; best_kf = kf; }
        }
        if (!best_kf) break;
        insert(best_kf);
    }
    return frames;
}

// ---- the slice of SiftManager that Bundler calls ----------------------------------------------------------------
void FeatureManager::forgetFrame(const std::shared_ptr<Frame> &frame)
{
    for (auto it = _matches.begin(); it != _matches.end();)
        it = (it->first.first == frame->_id || it->first.second == frame->_id) ? _matches.erase(it) : std::next(it);
}

int FeatureManager::countInlierCorres(const std::shared_ptr<Frame> &frameA, const std::shared_ptr<Frame> &frameB) const
{
    const auto it = _matches.find({ frameA->_id, frameB->_id });
    return it == _matches.end() ? 0 : (int)(it->second.ptA_cam.size() / 3);      // every stored match is an inlier (pruned ones are removed, :717-738)
}

static void transform_points(const Matrix4f &T, const std::vector<float> &in, std::vector<float> &out)       // pcl::transformPointWithNormal, fp32
{
    out.resize(in.size());
    for (size_t i = 0; i + 2 < in.size(); i += 3)
        for (int r = 0; r < 3; r++) out[i + r] = T(r, 0) * in[i] + T(r, 1) * in[i + 1] + T(r, 2) * in[i + 2] + T(r, 3);
}

Matrix4f FeatureManager::procrustesByCorrespondence(const std::shared_ptr<Frame> &frameA, const std::shared_ptr<Frame> &frameB)
{
    Matrix4f pose = Matrix4f::Identity();
    if (countInlierCorres(frameA, frameB) < 5) return pose;                      // :527
    const Correspondences &m = _matches.at({ frameA->_id, frameB->_id });
    std::vector<float> src, dst;
    transform_points(frameA->_pose_in_model, m.ptA_cam, src);                    // :537-538
    transform_points(frameB->_pose_in_model, m.ptB_cam, dst);
    solveRigidTransformBetweenPoints(src, dst, pose);                            // :544 (the reference then aborts on a mean error > 1e-3 between neighbours)
    return pose;
}

void FeatureManager::runRansacMultiPairGPU(btba_workspace *ws, const std::vector<std::pair<std::shared_ptr<Frame>, std::shared_ptr<Frame>>> &pairs,
                                           int max_iter, float inlier_dist)
{
    if (pairs.empty()) return;
    std::vector<float> A, B;                                                     // float4 (x, y, z, 1) of all pairs back to back (:680-705)
    std::vector<int32_t> n_pts;
    std::vector<float> pa, pb;
    for (const auto &pr : pairs) {
        const auto it = _matches.find({ pr.first->_id, pr.second->_id });
        const size_t n = it == _matches.end() ? 0 : it->second.ptA_cam.size() / 3;
        if (n) {
            transform_points(pr.first->_pose_in_model, it->second.ptA_cam, pa);
            transform_points(pr.second->_pose_in_model, it->second.ptB_cam, pb);
            for (size_t i = 0; i < n; i++) {
                A.insert(A.end(), { pa[3 * i], pa[3 * i + 1], pa[3 * i + 2], 1.0f });
                B.insert(B.end(), { pb[3 * i], pb[3 * i + 1], pb[3 * i + 2], 1.0f });
            }
        }
        n_pts.push_back((int32_t)n);
    }
    std::vector<int32_t> ids(std::max<size_t>(A.size() / 4, 1)), n_in(pairs.size()), best(pairs.size());
    const int rc = btba_ransac_pairs(ws, (int)pairs.size(), A.data(), B.data(), n_pts.data(), max_iter, inlier_dist, /*samples=*/nullptr, /*seed=*/0,
                                     ids.data(), n_in.data(), best.data(), nullptr, nullptr, nullptr);
    if (rc != BTBA_OK) throw Error(rc, "btba_ransac_pairs");
    size_t o = 0;
    for (size_t p = 0; p < pairs.size(); p++) {                                  // :715-739
        const auto it = _matches.find({ pairs[p].first->_id, pairs[p].second->_id });
        if (it != _matches.end()) {
            Correspondences kept;
            if (n_in[p] >= 5)
                for (int k = 0; k < n_in[p]; k++) {
                    const int i = ids[o + k];
                    kept.ptA_cam.insert(kept.ptA_cam.end(), it->second.ptA_cam.begin() + 3 * i, it->second.ptA_cam.begin() + 3 * i + 3);
                    kept.ptB_cam.insert(kept.ptB_cam.end(), it->second.ptB_cam.begin() + 3 * i, it->second.ptB_cam.begin() + 3 * i + 3);
                }
            it->second = std::move(kept);                                        // fewer than 5 survivors: every match goes (:733-737)
        }
        o += (size_t)n_pts[p];
    }
}

void FeatureManager::findCorresbyNNMultiPair(btba_workspace *ws, const std::vector<std::pair<std::shared_ptr<Frame>, std::shared_ptr<Frame>>> &pairs)
{
    if (pairs.empty()) return;
    const Config cfg = yml ? *yml : Config{};
    btba_match_params prm;
    btba_match_params_default(&prm);
    prm.mutual = cfg.feature_corres_mutual ? 1 : 0;
    prm.max_dist_neighbor = cfg.feature_corres_max_dist_neighbor;
    prm.cos_max_normal_neighbor = (float)std::cos(cfg.feature_corres_max_normal_neighbor / 180.0 * M_PI);     // :252-255
    prm.max_dist_no_neighbor = cfg.feature_corres_max_dist_no_neighbor;
    prm.cos_max_normal_no_neighbor = (float)std::cos(cfg.feature_corres_max_normal_no_neighbor / 180.0 * M_PI);
    std::vector<Frame *> frames;                                                  // every frame once, in order of first appearance
    std::map<const Frame *, int> index;
    std::vector<int32_t> pr;
    for (const auto &p : pairs)
        for (const Frame *f : { p.first.get(), p.second.get() }) {
            auto it = index.find(f);
            if (it == index.end()) { it = index.emplace(f, (int)frames.size()).first; frames.push_back(const_cast<Frame *>(f)); }
            pr.push_back(it->second);
        }
    const int n = (int)frames.size();
    const Frame &f0 = *frames[0];
    int D = 4;
    std::vector<const float *> desc(n), kpts(n), depth(n), normal(n);
    std::vector<int32_t> n_kpts(n), ids(n);
    std::vector<float> poses(16 * (size_t)n);
    for (int k = 0; k < n; k++) {
        const Frame &f = *frames[k];
        if (f._H != f0._H || f._W != f0._W) throw Error(BTBA_EINVAL, "findCorresbyNNMultiPair: frames of different sizes");
        if (f._n_keypts > 0) D = f._feat_dim;
        desc[k] = f._feat_des_gpu; kpts[k] = reinterpret_cast<const float *>(f._kpts_gpu);
        depth[k] = f._depth_gpu; normal[k] = reinterpret_cast<const float *>(f._normal_gpu);
        n_kpts[k] = f._n_keypts; ids[k] = f._id;
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) poses[16 * (size_t)k + 4 * r + c] = f._pose_in_model(r, c);
    }
    float K[9];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) K[3 * r + c] = f0._K(r, c);
    int64_t cap = 0;
    int rc = btba_match_capacity(&prm, n, f0._H, f0._W, D, n_kpts.data(), (int)pairs.size(), pr.data(), &cap);
    if (rc != BTBA_OK) throw Error(rc, "btba_match_capacity");
    std::vector<btba_match> out(std::max<int64_t>(cap, 1));
    std::vector<int32_t> n_out(pairs.size());
    rc = btba_match_pairs(ws, &prm, /*device_resident=*/0, n, f0._H, f0._W, K, desc.data(), D, kpts.data(), n_kpts.data(), depth.data(), normal.data(),
                          poses.data(), ids.data(), (int)pairs.size(), pr.data(), out.data(), nullptr, nullptr, n_out.data());
    if (rc != BTBA_OK) throw Error(rc, "btba_match_pairs");
    size_t o = 0;
    for (size_t p = 0; p < pairs.size(); p++) {                                  // collectMutualMatches (:341-368): appended in the library's order
        Correspondences &m = _matches[{ pairs[p].first->_id, pairs[p].second->_id }];
        for (int i = 0; i < n_out[p]; i++, o++) {
            m.ptA_cam.insert(m.ptA_cam.end(), out[o].ptA_cam, out[o].ptA_cam + 3);
            m.ptB_cam.insert(m.ptB_cam.end(), out[o].ptB_cam, out[o].ptB_cam + 3);
        }
    }
}

void FeatureManager::findCorresbyNN(btba_workspace *ws, const std::shared_ptr<Frame> &frameA, const std::shared_ptr<Frame> &frameB)
{
    if (frameA->_n_keypts == 0 || frameB->_n_keypts == 0) return;               // :250
    findCorresbyNNMultiPair(ws, { { frameA, frameB } });
    const bool is_neighbor = std::abs(frameA->_id - frameB->_id) == 1;
    if (is_neighbor && countInlierCorres(frameA, frameB) < 5) frameA->_status = Frame::FAIL;      // :280-285
}

btba_ingest_params ingestParams()
{
    btba_ingest_params p;
    btba_ingest_params_default(&p);
    return p;
}

void ingestFrames(btba_workspace *ws, const std::vector<std::shared_ptr<Frame>> &frames, const btba_ingest_params &params)
{
    if (frames.empty()) return;
    if (params.depth_format != 0) throw Error(BTBA_EINVAL, "ingestFrames: Frame::_depth_code_gpu holds uint16 codes (depth_format 0)");
    const int n = (int)frames.size(), H = frames[0]->_H, W = frames[0]->_W;
    std::vector<const void *> depth_in(n);
    std::vector<const uint8_t *> bgr(n);
    std::vector<float *> depth(n), normal(n), raw(n), xyz(n);
    std::vector<uint8_t *> color(n);
    for (int k = 0; k < n; k++) {
        const Frame &f = *frames[k];
        if (f._H != H || f._W != W) throw Error(BTBA_EINVAL, "ingestFrames: frames of different sizes");
        depth_in[k] = f._depth_code_gpu;
        bgr[k] = f._color_gpu ? f._bgr_gpu : nullptr;
        depth[k] = f._depth_gpu;
        normal[k] = reinterpret_cast<float *>(f._normal_gpu);
        color[k] = f._bgr_gpu ? reinterpret_cast<uint8_t *>(f._color_gpu) : nullptr;
        raw[k] = f._depth_raw_gpu;
        xyz[k] = reinterpret_cast<float *>(f._xyz_gpu);
    }
    float K[9];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) K[3 * r + c] = frames[0]->_K(r, c);
    const int rc = btba_ingest_frames(ws, &params, n, H, W, K, depth_in.data(), bgr.data(), depth.data(), normal.data(), color.data(), raw.data(), xyz.data());
    if (rc != BTBA_OK) throw Error(rc, "btba_ingest_frames");
    for (auto &f : frames) f->_ingested = true;
}

btba_vos_params vosParams()
{
    btba_vos_params p;
    btba_vos_params_default(&p);
    return p;
}

void vosSampleFrames(const btba_vos_params &params, int frame_idx, std::vector<int> &idx, int &n_dense)
{
    std::vector<int32_t> buf((size_t)std::max(params.ref_num, 1));
    int32_t n = 0, nd = 0;
    const int rc = btba_vos_sample_frames(&params, frame_idx, buf.data(), &n, &nd);
    if (rc != BTBA_OK) throw Error(rc, "btba_vos_sample_frames");
    idx.assign(buf.begin(), buf.begin() + n);
    n_dense = nd;
}

void vosFirstLabels(btba_workspace *ws, int H, int W, int d, const uint8_t *label_dev, float *labels_out_dev)
{
    const int rc = btba_vos_first_labels(ws, H, W, d, label_dev, labels_out_dev);
    if (rc != BTBA_OK) throw Error(rc, "btba_vos_first_labels");
}

void vosPropagate(btba_workspace *ws, const btba_vos_params &params, int C, int d, int Hd, int Wd,
                  const std::vector<std::vector<const float *>> &refs, const std::vector<std::vector<const float *>> &labels,
                  const std::vector<const float *> &targets, const std::vector<int> &n_dense, const std::vector<float *> &pred,
                  const std::vector<float *> &onehot)
{
    const size_t n = targets.size();
    if (n == 0) return;
    if (refs.size() != n || labels.size() != n || n_dense.size() != n || pred.size() != n || (!onehot.empty() && onehot.size() != n))
        throw Error(BTBA_EINVAL, "vosPropagate: one entry per video in every table");
    std::vector<int32_t> n_ref(n), nd(n_dense.begin(), n_dense.end());
    std::vector<const float *> rf, lb;
    for (size_t b = 0; b < n; b++) {
        if (refs[b].size() != labels[b].size()) throw Error(BTBA_EINVAL, "vosPropagate: as many labels as references");
        n_ref[b] = (int32_t)refs[b].size();
        rf.insert(rf.end(), refs[b].begin(), refs[b].end());
        lb.insert(lb.end(), labels[b].begin(), labels[b].end());
    }
    const int rc = btba_vos_propagate(ws, &params, (int)n, C, d, Hd, Wd, n_ref.data(), nd.data(), rf.data(), lb.data(), targets.data(), pred.data(),
                                      onehot.empty() ? nullptr : onehot.data());
    if (rc != BTBA_OK) throw Error(rc, "btba_vos_propagate");
}

void vosMasks(btba_workspace *ws, int d, int Hd, int Wd, int H, int W, const float *pred_dev, uint8_t *mask_out_dev)
{
    const int rc = btba_vos_masks(ws, d, Hd, Wd, H, W, pred_dev, mask_out_dev);
    if (rc != BTBA_OK) throw Error(rc, "btba_vos_masks");
}

void vosInputs(btba_workspace *ws, const std::vector<const uint8_t *> &bgr_dev, int H, int W, float *rgb_out_dev)
{
    const int rc = btba_vos_inputs(ws, (int)bgr_dev.size(), H, W, bgr_dev.data(), rgb_out_dev);
    if (rc != BTBA_OK) throw Error(rc, "btba_vos_inputs");
}

MaskPropagator::MaskPropagator(btba_workspace *ws1, int d1, int H1, int W1, int C1, const btba_vos_params &params1, float *feats_dev,
                               float *labels_dev, float *pred_dev, uint8_t *mask_dev)
    : ws(ws1), d(d1), H(H1), W(W1), C(C1), Hd((H1 + 7) / 8), Wd((W1 + 7) / 8), params(params1), feats(feats_dev), labels(labels_dev),
      pred(pred_dev), mask(mask_dev)
{
    if (!feats || !labels || !pred || !mask || params.range < 0) throw Error(BTBA_EINVAL, "MaskPropagator: null buffer");
}

void MaskPropagator::start(const uint8_t *label_dev)
{
    vosFirstLabels(ws, H, W, d, label_dev, labelsOf(0));             // the features of frame 0 are in featuresOf(0) = nextFeatures()
    n_frames = 1;
}

const uint8_t *MaskPropagator::step()
{
    if (n_frames < 1) throw Error(BTBA_EINVAL, "MaskPropagator::step before start");
    const int f = n_frames;
    std::vector<int> idx;
    int n_dense = 0;
    vosSampleFrames(params, f, idx, n_dense);
    std::vector<const float *> rf, lb;
    for (int i : idx) { rf.push_back(featuresOf(i)); lb.push_back(labelsOf(i)); }
    vosPropagate(ws, params, C, d, Hd, Wd, { rf }, { lb }, { featuresOf(f) }, { n_dense }, { pred }, { labelsOf(f) });
    vosMasks(ws, d, Hd, Wd, H, W, pred, mask);
    n_frames = f + 1;
    return mask;
}

void segmentationByMaskMultiFrame(btba_workspace *ws, const std::vector<std::shared_ptr<Frame>> &frames, bool largest_component_hull, int dilate)
{
    if (frames.empty()) return;
    const int n = (int)frames.size(), H = frames[0]->_H, W = frames[0]->_W;
    std::vector<const uint8_t *> mask(n);
    std::vector<float *> depth(n), normal(n);
    std::vector<uint8_t *> color(n), out(n);
    for (int k = 0; k < n; k++) {
        const Frame &f = *frames[k];
        if (f._H != H || f._W != W) throw Error(BTBA_EINVAL, "segmentationByMask: frames of different sizes");
        mask[k] = f._mask_gpu;
        depth[k] = f._depth_gpu;
        normal[k] = reinterpret_cast<float *>(f._normal_gpu);
        color[k] = reinterpret_cast<uint8_t *>(f._color_gpu);
        out[k] = f._fg_mask_gpu;
    }
    btba_mask_params prm;
    btba_mask_params_default(&prm);
    prm.largest_component_hull = largest_component_hull ? 1 : 0;
    prm.dilate = dilate;
    std::vector<float> roi(4 * (size_t)n);
    const int rc = btba_apply_masks(ws, &prm, n, H, W, mask.data(), depth.data(), normal.data(), color.data(), out.data(), roi.data());
    if (rc != BTBA_OK) throw Error(rc, "btba_apply_masks");
    for (int k = 0; k < n; k++)
        for (int q = 0; q < 4; q++) frames[k]->_roi[q] = roi[4 * k + q];
}

void segmentationByMask(btba_workspace *ws, const std::shared_ptr<Frame> &frame, bool largest_component_hull, int dilate)
{
    segmentationByMaskMultiFrame(ws, { frame }, largest_component_hull, dilate);
}

void prepareDetectorInputs(btba_workspace *ws, const std::vector<std::shared_ptr<Frame>> &frames, uint8_t *bgr_out, float *gray_out, int out_size)
{
    if (frames.empty()) return;
    const int n = (int)frames.size(), H = frames[0]->_H, W = frames[0]->_W;
    std::vector<const uint8_t *> color(n);
    std::vector<float> roi(4 * (size_t)n);
    for (int k = 0; k < n; k++) {
        const Frame &f = *frames[k];
        if (f._H != H || f._W != W) throw Error(BTBA_EINVAL, "prepareDetectorInputs: frames of different sizes");
        color[k] = reinterpret_cast<const uint8_t *>(f._color_gpu);
        for (int q = 0; q < 4; q++) roi[4 * k + q] = f._roi[q];
    }
    btba_detector_params prm;
    btba_detector_params_default(&prm);
    prm.out_size = out_size;
    const int rc = btba_detector_inputs(ws, &prm, n, H, W, color.data(), roi.data(), bgr_out, gray_out);
    if (rc != BTBA_OK) throw Error(rc, "btba_detector_inputs");
}

void keypointsToImage(btba_workspace *ws, const std::shared_ptr<Frame> &frame, const float2 *kpts_in, int n, float2 *kpts_out, int out_size)
{
    btba_detector_params prm;
    btba_detector_params_default(&prm);
    prm.out_size = out_size;
    const float *in = reinterpret_cast<const float *>(kpts_in);
    float *out = reinterpret_cast<float *>(kpts_out);
    const int32_t cnt = n;
    const int rc = btba_detector_keypoints_to_image(ws, &prm, 1, frame->_roi, &in, &cnt, &out);
    if (rc != BTBA_OK) throw Error(rc, "btba_detector_keypoints_to_image");
    frame->_kpts_gpu = kpts_out;
    frame->_n_keypts = n;
}

// ---- GpuFeatureManager: findCorres with map points on btba_corres_chain --------------------------------------------
GpuFeatureManager::GpuFeatureManager(btba_workspace *ws, std::shared_ptr<Config> yml1) : ws_(ws)
{
    yml = yml1 ? std::move(yml1) : std::make_shared<Config>();
    const int rc = btba_mappoints_create(ws, &mp_);
    if (rc != BTBA_OK) throw Error(rc, "btba_mappoints_create");
}

GpuFeatureManager::~GpuFeatureManager() { btba_mappoints_destroy(mp_); }

void GpuFeatureManager::findCorres(const std::shared_ptr<Frame> &frameA, const std::shared_ptr<Frame> &frameB) { findCorresChain({ { frameA, frameB } }); }

void GpuFeatureManager::forgetFrame(const std::shared_ptr<Frame> &frame)
{
    FeatureManager::forgetFrame(frame);
    for (auto it = _records.begin(); it != _records.end();)
        it = (it->first.first == frame->_id || it->first.second == frame->_id) ? _records.erase(it) : std::next(it);
    const auto s = slots_.find(frame->_id);
    if (s == slots_.end()) return;
    const int rc = btba_mappoints_forget_frame(mp_, s->second);
    slots_.erase(s);
    if (rc != BTBA_OK) throw Error(rc, "btba_mappoints_forget_frame");
}

bool GpuFeatureManager::findCorresChain(const std::vector<std::pair<std::shared_ptr<Frame>, std::shared_ptr<Frame>>> &all)
{
    std::vector<std::pair<std::shared_ptr<Frame>, std::shared_ptr<Frame>>> pairs;     // pairs already matched are skipped (:176)
    std::set<std::pair<int, int>> seen;
    for (const auto &p : all) {
        const std::pair<int, int> key{ p.first->_id, p.second->_id };
        if (_matches.count(key) || !seen.insert(key).second) continue;
        pairs.push_back(p);
    }
    if (pairs.empty()) return true;
    const Config &cfg = *yml;
    btba_match_params prm;
    btba_match_params_default(&prm);
    prm.mutual = cfg.feature_corres_mutual ? 1 : 0;
    prm.max_dist_neighbor = cfg.feature_corres_max_dist_neighbor;
    prm.cos_max_normal_neighbor = (float)std::cos(cfg.feature_corres_max_normal_neighbor / 180.0 * M_PI);     // :252-255
    prm.max_dist_no_neighbor = cfg.feature_corres_max_dist_no_neighbor;
    prm.cos_max_normal_no_neighbor = (float)std::cos(cfg.feature_corres_max_normal_no_neighbor / 180.0 * M_PI);
    btba_corres_params rp;
    btba_corres_params_default(&rp);
    rp.n_trials = cfg.ransac_max_iter;
    rp.dist_thres = cfg.ransac_inlier_dist;
    std::vector<Frame *> frames;                                                  // every frame once, in order of first appearance
    std::map<const Frame *, int> index;
    std::vector<int32_t> pr;
    for (const auto &p : pairs)
        for (const Frame *f : { p.first.get(), p.second.get() }) {
            auto it = index.find(f);
            if (it == index.end()) { it = index.emplace(f, (int)frames.size()).first; frames.push_back(const_cast<Frame *>(f)); }
            pr.push_back(it->second);
        }
    const int n = (int)frames.size();
    const Frame &f0 = *frames[0];
    int D = 4;
    std::vector<const float *> desc(n), kpts(n), depth(n), normal(n);
    std::vector<int32_t> n_kpts(n), ids(n), slots(n), status(n);
    std::vector<float> poses(16 * (size_t)n);
    for (int k = 0; k < n; k++) {
        Frame &f = *frames[k];
        if (f._H != f0._H || f._W != f0._W) throw Error(BTBA_EINVAL, "findCorresChain: frames of different sizes");
        if (f._n_keypts > 0) D = f._feat_dim;
        desc[k] = f._feat_des_gpu; kpts[k] = reinterpret_cast<const float *>(f._kpts_gpu);
        depth[k] = f._depth_gpu; normal[k] = reinterpret_cast<const float *>(f._normal_gpu);
        n_kpts[k] = f._n_keypts; ids[k] = f._id;
        status[k] = f._status == Frame::FAIL ? 1 : 0;
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) poses[16 * (size_t)k + 4 * r + c] = f._pose_in_model(r, c);
        auto s = slots_.find(f._id);
        if (s == slots_.end()) {
            int32_t slot = -1;
            const int rc = btba_mappoints_register_frame(mp_, f._n_keypts, reinterpret_cast<const float *>(f._kpts_gpu), &slot);
            if (rc != BTBA_OK) throw Error(rc, "btba_mappoints_register_frame");
            s = slots_.emplace(f._id, slot).first;
        }
        slots[k] = s->second;
    }
    float K[9];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) K[3 * r + c] = f0._K(r, c);
    int64_t cap = 0;
    int rc = btba_corres_chain_capacity(&prm, n, f0._H, f0._W, D, n_kpts.data(), (int)pairs.size(), pr.data(), &cap);
    if (rc != BTBA_OK) throw Error(rc, "btba_corres_chain_capacity");
    std::vector<btba_match> out(std::max<int64_t>(cap, 1));
    std::vector<int32_t> n_out(pairs.size());
    rc = btba_corres_chain(ws_, mp_, &prm, &rp, /*device_resident=*/0, n, f0._H, f0._W, K, desc.data(), D, kpts.data(), n_kpts.data(), depth.data(),
                           normal.data(), poses.data(), ids.data(), slots.data(), status.data(), (int)pairs.size(), pr.data(), out.data(), n_out.data(), nullptr);
    if (rc != BTBA_OK) throw Error(rc, "btba_corres_chain");
    for (int k = 0; k < n; k++)
        if (status[k]) frames[k]->_status = Frame::FAIL;
    size_t o = 0;
    for (size_t p = 0; p < pairs.size(); p++) {
        const std::pair<int, int> key{ pairs[p].first->_id, pairs[p].second->_id };
        Correspondences &m = _matches[key];
        std::vector<btba_match> &rec = _records[key];
        m = Correspondences{};
        rec.assign(out.begin() + o, out.begin() + o + n_out[p]);
        for (const btba_match &r : rec) {
            m.ptA_cam.insert(m.ptA_cam.end(), r.ptA_cam, r.ptA_cam + 3);
            m.ptB_cam.insert(m.ptB_cam.end(), r.ptB_cam, r.ptB_cam + 3);
        }
        o += (size_t)n_out[p];
    }
    return true;
}

btba_lfnet_params lfnetParams()
{
    btba_lfnet_params p;
    btba_lfnet_params_default(&p);
    return p;
}

std::vector<int> lfnetKeypoints(btba_workspace *ws, const btba_lfnet_params &params, int n_frames, int H, int W, const LfnetMapSet &maps,
                                const float *photo_dev, const float *ori_dev, const LfnetBuffers &out)
{
    const size_t S = maps.score_dev.size();
    if (maps.map_h.size() != S || maps.map_w.size() != S || maps.scale_factors.size() != S || n_frames < 1)
        throw Error(BTBA_EINVAL, "lfnetKeypoints: one size and one scale factor per score map");
    std::vector<int32_t> counts((size_t)n_frames);
    const int rc = btba_lfnet_keypoints(ws, &params, n_frames, H, W, (int)S, maps.score_dev.data(), maps.map_h.data(), maps.map_w.data(),
                                        maps.scale_factors.data(), photo_dev, ori_dev, out.max_heatmaps, out.max_scales, out.kpts_xy, out.n_kpts,
                                        out.kpts, out.kpts_scale, out.kpts_ori, out.patches, counts.data());
    if (rc != BTBA_OK) throw Error(rc, "btba_lfnet_keypoints");
    return std::vector<int>(counts.begin(), counts.end());
}

DetectedFeatures LfnetDetector::operator()(const uint8_t *, const float *gray_dev, int out_size) const
{
    const float *ori_dev = nullptr;
    const LfnetMapSet maps = score_(gray_dev, out_size, ori_dev);
    const int m = lfnetKeypoints(ws_, params_, 1, out_size, out_size, maps, gray_dev, ori_dev, out_)[0];
    DetectedFeatures f;
    f.kpts_dev = reinterpret_cast<float2 *>(out_.kpts);
    f.n = m;
    f.desc_dev = desc_(out_.patches, m, f.dim);
    return f;
}

btba_lfnet_desc_config lfnetDescConfig()
{
    btba_lfnet_desc_config c;
    btba_lfnet_desc_config_default(&c);
    return c;
}

void lfnetDescriptors(btba_workspace *ws, const btba_lfnet_desc_model *model, int n_frames, int slots, const float *patches_dev,
                      const int32_t *n_kpts_dev, float *desc_dev)
{
    const int rc = btba_lfnet_descriptors(ws, model, n_frames, slots, patches_dev, n_kpts_dev, desc_dev);
    if (rc != BTBA_OK) throw Error(rc, "btba_lfnet_descriptors");
}

LfnetDetector::DescFn LfnetDescriptor::asDescNet(float *desc_dev) const
{
    return [this, desc_dev](const float *patches_dev, int m, int &dim) {
        dim = config_.out_dim;
        describe(1, m, patches_dev, nullptr, desc_dev);
        return desc_dev;
    };
}

btba_lfnet_det_config lfnetDetConfig()
{
    btba_lfnet_det_config c;
    btba_lfnet_det_config_default(&c);
    return c;
}

std::vector<double> lfnetDetScales(double min_scale, double max_scale, int num_scales)
{
    std::vector<double> out((size_t)std::max(num_scales, 1));
    const int rc = btba_lfnet_det_scales(min_scale, max_scale, num_scales, out.data());
    if (rc != BTBA_OK) throw Error(rc, "btba_lfnet_det_scales");
    return out;
}

LfnetMapSet LfnetScoreNet::mapSet(int H, int W, const std::vector<float *> &score_dev) const
{
    const size_t S = (size_t)config_.num_scales;
    if (score_dev.size() != S) throw Error(BTBA_EINVAL, "LfnetScoreNet: one score buffer per scale");
    LfnetMapSet maps;
    maps.score_dev.assign(score_dev.begin(), score_dev.end());
    maps.map_h.resize(S);
    maps.map_w.resize(S);
    const int rc = btba_lfnet_det_map_sizes(model_, H, W, maps.map_h.data(), maps.map_w.data());
    if (rc != BTBA_OK) throw Error(rc, "btba_lfnet_det_map_sizes");
    for (size_t j = 0; j < S; j++) maps.scale_factors.push_back((float)config_.scale_factors[j]);
    return maps;
}

void LfnetScoreNet::scores(int n_frames, int H, int W, const float *photo_dev, const std::vector<float *> &score_dev, float *ori_dev) const
{
    if (score_dev.size() != (size_t)config_.num_scales) throw Error(BTBA_EINVAL, "LfnetScoreNet: one score buffer per scale");
    const int rc = btba_lfnet_scores(ws_, model_, n_frames, H, W, photo_dev, score_dev.data(), ori_dev);
    if (rc != BTBA_OK) throw Error(rc, "btba_lfnet_scores");
}

LfnetDetector::ScoreFn LfnetScoreNet::asScoreNet(std::vector<float *> score_dev, float *ori_dev) const
{
    return [this, score_dev, ori_dev](const float *gray_dev, int out_size, const float *&ori_out) {
        scores(1, out_size, out_size, gray_dev, score_dev, ori_dev);
        ori_out = ori_dev;
        return mapSet(out_size, out_size, score_dev);
    };
}

btba_vos_net_config vosNetConfig()
{
    btba_vos_net_config c;
    btba_vos_net_config_default(&c);
    return c;
}

VosBackbone::VosBackbone(btba_workspace *ws, const btba_vos_net_config &config, const std::vector<btba_vos_net_layer> &layers)
    : ws_(ws), config_(config)
{
    const int rc = btba_vos_net_model_create(ws, &config, layers.data(), (int)layers.size(), &model_);
    if (rc != BTBA_OK) throw Error(rc, "btba_vos_net_model_create");
}

void VosBackbone::features(int n_frames, int H, int W, const float *rgb_dev, float *features_out_dev) const
{
    const int rc = btba_vos_features(ws_, model_, n_frames, H, W, rgb_dev, features_out_dev);
    if (rc != BTBA_OK) throw Error(rc, "btba_vos_features");
}

Bundler::SegmentFn VosBackbone::asSegmenter(int H, int W) const
{
    return [this, H, W](const float *rgb_dev, float *features_out_dev) { features(1, H, W, rgb_dev, features_out_dev); };
}

void DetectorFeatureManager::detectFeature(const std::shared_ptr<Frame> &frame)              // FeatureManager.cpp:811-908
{
    prepareDetectorInputs(ws_, { frame }, bgr_, gray_, out_size_);
    const DetectedFeatures got = detect_(bgr_, gray_, out_size_);
    keypointsToImage(ws_, frame, got.kpts_dev, got.n, got.kpts_dev, out_size_);
    frame->_feat_des_gpu = got.desc_dev;
    frame->_feat_dim = got.dim;
}

// ---- Bundler ---------------------------------------------------------------------------------------------------
Bundler::Bundler(std::shared_ptr<Config> yml1, std::shared_ptr<FeatureManager> fm, const Matrix3f &K1, int H1, int W1, OptimizeFn optimize)
    : yml(yml1 ? std::move(yml1) : std::make_shared<Config>()), _fm(std::move(fm)), memory(yml), K(K1), H(H1), W(W1), optimize_(std::move(optimize))
{
    if (!_fm) throw Error(BTBA_EINVAL, "Bundler: no feature manager");
}

void Bundler::processNewFrame(std::shared_ptr<Frame> frame)
{
    _newframe = frame;
    std::shared_ptr<Frame> last_frame;
    if (!_frames.empty()) {                                                      // :75-80
        last_frame = _frames.back();
        frame->_id = last_frame->_id + 1;
        frame->_pose_in_model = last_frame->_pose_in_model;
    }
    const bool ingest = frame->_depth_code_gpu && !frame->_ingested;             // Frame's constructor (Frame.cpp:45-89), minus the imreads
    const bool propagate = segmenter && mask_propagator && frame->_bgr_gpu && (!frame->_mask_gpu || mask_propagator->n_frames == 0);
    if (ingest || propagate || frame->_mask_gpu) {
        if (frame->_H == 0 && frame->_W == 0) { frame->_H = H; frame->_W = W; }
        btba_workspace *ws = mask_ws;
        if (!ws) {
            if (!own_opt_) own_opt_ = std::make_unique<OptimizerGpu>(yml);
            ws = own_opt_->workspace();
        }
        if (ingest) {
            if (frame->_K(2, 2) == 0.0f) frame->_K = K;                          // unset (a real K has 1 there): the Bundler's own
            ingestFrames(ws, { frame }, ingestParams());
        }
        if (propagate) {                                                         // run_video.py's loop body around the backbone
            if (!rgb_dev) throw Error(BTBA_EINVAL, "Bundler: segmenter set without rgb_dev");
            vosInputs(ws, { frame->_bgr_gpu }, frame->_H, frame->_W, rgb_dev);
            segmenter(rgb_dev, mask_propagator->nextFeatures());
            if (frame->_mask_gpu) mask_propagator->start(frame->_mask_gpu);
            else frame->_mask_gpu = const_cast<uint8_t *>(mask_propagator->step());
        }
        if (frame->_mask_gpu) segmentationByMask(ws, frame, yml->mask_largest_component_hull, yml->mask_dilate);      // :80/:84 segmentationByMaskFile
    }
    if (frame->_roi[1] - frame->_roi[0] < 10 || frame->_roi[3] - frame->_roi[2] < 10) {      // :88-93: "cloud is empty, marked FAIL" -- a plain return:
        frame->_status = Frame::FAIL;                                            // no forgetFrame, no re-initialisation request
        return;
    }
    if (frame->_status == Frame::FAIL) {                                         // :96-101 (marked FAIL before it got here)
        _fm->forgetFrame(frame);
        _need_reinit = true;
        return;
    }
    try {
        _fm->detectFeature(frame);                                               // :103-117
    } catch (const std::exception &) {
        frame->_status = Frame::FAIL;
        _need_reinit = true;
        _fm->forgetFrame(frame);
        return;
    }
    if (last_frame) {
        _fm->findCorres(frame, last_frame);                                      // :121
        if (frame->_status == Frame::FAIL) {
            _need_reinit = true;
            _fm->forgetFrame(frame);
            return;
        }
        const Matrix4f offset = _fm->procrustesByCorrespondence(frame, last_frame);      // :134-136: pose = offset * pose
        Matrix4f moved;
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) {
                float acc = 0.0f;
                for (int k = 0; k < 4; k++) acc += offset(r, k) * frame->_pose_in_model(k, c);
                moved(r, c) = acc;
            }
        frame->_pose_in_model = moved;
    }
    if ((int)_frames.size() >= yml->window_size + 3) {                           // :150-158
        if (std::find(memory._keyframes.begin(), memory._keyframes.end(), _frames.front()) == memory._keyframes.end()) _fm->forgetFrame(_frames.front());
        _frames.pop_front();
    }
    _frames.push_back(frame);
    if (frame->_id == 0) {                                                       // :162-166
        memory.checkAndAddKeyframe(frame);
        return;
    }
    _local_frames = memory.selectKeyFramesForBA(frame);                          // :168-172
    optimizeGPU();
    if (frame->_status == Frame::FAIL) {                                         // :174-180
        _fm->forgetFrame(frame);
        _frames.pop_back();
        if (own_opt_ && own_opt_->persistent_frame_cache) btba_frame_cache_evict(own_opt_->workspace(), (uint64_t)frame->_id);      // its id is handed out again
        _need_reinit = true;
        return;
    }
    memory.checkAndAddKeyframe(frame);                                           // :182
    if (!yml->pose_dir.empty()) saveNewframeResult();
}

void Bundler::optimizeGPU()
{
    std::sort(_local_frames.begin(), _local_frames.end(), [](const std::shared_ptr<Frame> &a, const std::shared_ptr<Frame> &b) { return a->_id < b->_id; });   // :286
    std::vector<std::pair<std::shared_ptr<Frame>, std::shared_ptr<Frame>>> pairs;
    for (size_t i = 0; i < _local_frames.size(); i++)
        for (size_t j = i + 1; j < _local_frames.size(); j++) pairs.emplace_back(_local_frames[j], _local_frames[i]);                                    // :303
    if (!_fm->findCorresChain(pairs))                                           // a feature manager without a chain: pair by pair
        for (const auto &p : pairs) _fm->findCorres(p.first, p.second);
    last_window = marshalWindow(_local_frames, _fm->_matches, _newframe, yml->min_fm_edges_newframe);          // :296-347 (sets NO_BA)
    if (!last_window.run_ba) return;
    const auto &fr = last_window.frames;
    std::vector<float *> depths_gpu;
    std::vector<uchar4 *> colors_gpu;
    std::vector<float4 *> normals_gpu;
    std::vector<Matrix4f> poses;
    for (const auto &f : fr) { depths_gpu.push_back(f->_depth_gpu); colors_gpu.push_back(f->_color_gpu); normals_gpu.push_back(f->_normal_gpu); poses.push_back(f->_pose_in_model); }
    if (optimize_) {
        optimize_(last_window.global_corres, last_window.n_match_per_pair, (int)fr.size(), H, W, depths_gpu, colors_gpu, normals_gpu, poses, K);
    } else {
        if (!own_opt_) own_opt_ = std::make_unique<OptimizerGpu>(yml);
        if (own_opt_->persistent_frame_cache) {
            own_opt_->frame_ids.clear();
            for (const auto &f : fr) own_opt_->frame_ids.push_back((uint64_t)f->_id);
        }
        own_opt_->optimizeFrames(last_window.global_corres, last_window.n_match_per_pair, (int)fr.size(), H, W, depths_gpu, colors_gpu, normals_gpu, poses, K);
    }
    n_ba_calls++;
    for (size_t i = 0; i < fr.size(); i++) fr[i]->_pose_in_model = poses[i];     // :353-357
}

Matrix4f inverse(const Matrix4f &M)
{
    double a[4][8];                                                              // [M | I] -> [I | M^-1], Gauss-Jordan with partial pivoting
    for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) { a[r][c] = M(r, c); a[r][4 + c] = r == c ? 1.0 : 0.0; }
    for (int k = 0; k < 4; k++) {
        int piv = k;
        for (int r = k + 1; r < 4; r++) if (std::fabs(a[r][k]) > std::fabs(a[piv][k])) piv = r;
        if (piv != k) for (int c = 0; c < 8; c++) std::swap(a[k][c], a[piv][c]);
        const double d = a[k][k];                                                // 0 for a singular matrix: the result is inf / nan, as Eigen's
        for (int c = 0; c < 8; c++) a[k][c] /= d;
        for (int r = 0; r < 4; r++) {
            if (r == k) continue;
            const double f = a[r][k];
            for (int c = 0; c < 8; c++) a[r][c] -= f * a[k][c];
        }
    }
    Matrix4f R;
    for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) R(r, c) = (float)a[r][4 + c];
    return R;
}

void Bundler::saveNewframeResult()
{
    if (yml->pose_dir.empty() || !_newframe) return;
    const std::string name = _newframe->_id_str.empty() ? std::to_string(_newframe->_id) : _newframe->_id_str;
    std::ofstream ff(yml->pose_dir + "/" + name + ".txt");                       // the caller creates the directory (the reference: system("mkdir -p"))
    ff << formatPoseTxt(inverse(_newframe->_pose_in_model));                     // ob_in_cam = cur_in_model.inverse(), :371-375
}

// ---- problem dumps (bundletrack_amd/problem_io.py documents the layout) ---------------------------------------
namespace {
const char kProblemMagic[8] = { 'B', 'T', 'B', 'A', 'P', 'R', 'B', '1' };
struct ProblemHeader { char magic[8]; int32_t n_frames, H, W; uint32_t n_corr; int32_t flags; float image_downscale; };
static_assert(sizeof(ProblemHeader) == 32, "problem dump header");
template <class T> void read_array(std::ifstream &f, std::vector<T> &v, size_t n, const std::string &path)
{
    v.resize(n);
    f.read(reinterpret_cast<char *>(v.data()), (std::streamsize)(sizeof(T) * n));
    if (!f) throw Error(BTBA_EINVAL, path + ": truncated problem dump");
}
template <class T> void write_array(std::ofstream &f, const std::vector<T> &v) { f.write(reinterpret_cast<const char *>(v.data()), (std::streamsize)(sizeof(T) * v.size())); }
}  // namespace

ProblemDump loadProblem(const std::string &path)
{
    std::ifstream f(path, std::ios::binary);
    ProblemHeader h{};
    f.read(reinterpret_cast<char *>(&h), sizeof h);
    if (!f || std::memcmp(h.magic, kProblemMagic, 8) != 0) throw Error(BTBA_EINVAL, path + ": not a BTBAPRB1 problem dump");
    if (h.n_frames < 1 || h.H < 1 || h.W < 1) throw Error(BTBA_EINVAL, path + ": corrupt problem dump header");
    ProblemDump pb;
    pb.n_frames = h.n_frames; pb.H = h.H; pb.W = h.W; pb.image_downscale = h.image_downscale;
    f.read(reinterpret_cast<char *>(pb.K), sizeof pb.K);
    const size_t N = (size_t)h.n_frames, P = N * (N - 1) / 2, npix = (size_t)h.H * h.W;
    read_array(f, pb.corr, h.n_corr, path);
    std::vector<int32_t> nm;
    read_array(f, nm, P, path);
    pb.n_match_per_pair.assign(nm.begin(), nm.end());
    read_array(f, pb.poses_init, 16 * N, path);
    if (h.flags & 1) read_array(f, pb.poses_gt, 16 * N, path);
    read_array(f, pb.depth, N * npix, path);
    read_array(f, pb.normals, 4 * N * npix, path);
    if (f.peek() != std::ifstream::traits_type::eof()) throw Error(BTBA_EINVAL, path + ": trailing bytes after the problem dump");
    return pb;
}

void saveProblem(const std::string &path, const ProblemDump &pb)
{
    const size_t N = (size_t)pb.n_frames, P = N * (N - 1) / 2, npix = (size_t)pb.H * pb.W;
    if (pb.n_frames < 1 || pb.n_match_per_pair.size() != P || pb.poses_init.size() != 16 * N || (!pb.poses_gt.empty() && pb.poses_gt.size() != 16 * N) ||
        pb.depth.size() != N * npix || pb.normals.size() != 4 * N * npix)
        throw Error(BTBA_EINVAL, "saveProblem: array sizes do not match n_frames / H / W");
    ProblemHeader h{};
    std::memcpy(h.magic, kProblemMagic, 8);
    h.n_frames = pb.n_frames; h.H = pb.H; h.W = pb.W; h.n_corr = (uint32_t)pb.corr.size(); h.flags = pb.poses_gt.empty() ? 0 : 1;
    h.image_downscale = pb.image_downscale;
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char *>(&h), sizeof h);
    f.write(reinterpret_cast<const char *>(pb.K), sizeof pb.K);
    write_array(f, pb.corr);
    write_array(f, std::vector<int32_t>(pb.n_match_per_pair.begin(), pb.n_match_per_pair.end()));
    write_array(f, pb.poses_init);
    write_array(f, pb.poses_gt);
    write_array(f, pb.depth);
    write_array(f, pb.normals);
    if (!f) throw Error(BTBA_EINVAL, path + ": write failed");
}

}  // namespace btba
