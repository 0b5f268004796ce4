// nocs_driver.cpp -- ctypes entry into the C++ host layer's btba::nocsErrors and btba::nocsReport (tests/test_gpu_nocs.py,
// tests/test_nocs_ref.py).  Everything is a flat row-major host array.
#include <vector>

#include "../../bundletrack_amd/cpp/btba_host.hpp"

namespace {
btba::Matrix4d from_rowmajor(const double *p)
{
    btba::Matrix4d M;
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) M(r, c) = p[4 * r + c];
    return M;
}
}  // namespace

extern "C" __attribute__((visibility("default"))) int nocs_errors_driver(void *ws, const btba_nocs_params *params, int n_boxes, const double *boxes,
                                                                          int n, const int32_t *class_id, const int32_t *handle_visible,
                                                                          const int32_t *box_index, const double *poses_pred, const double *poses_gt,
                                                                          double *theta_out, double *shift_out, double *iou_out)
{
    try {
        std::vector<btba::NocsBox> bx(n_boxes);
        for (int b = 0; b < n_boxes; b++)
            for (int k = 0; k < 24; k++) bx[b][k] = boxes[24 * b + k];
        std::vector<btba::Matrix4d> pp, pg;
        for (int e = 0; e < n; e++) {
            pp.push_back(from_rowmajor(poses_pred + 16 * e));
            pg.push_back(from_rowmajor(poses_gt + 16 * e));
        }
        std::vector<int32_t> hv;
        if (handle_visible) hv.assign(handle_visible, handle_visible + n);
        std::vector<double> theta, shift, iou;
        btba::nocsErrors(static_cast<btba_workspace *>(ws), params ? *params : btba::nocsParams(), bx, std::vector<int32_t>(class_id, class_id + n), hv,
                         std::vector<int32_t>(box_index, box_index + n), pp, pg, theta, shift, iou);
        for (int e = 0; e < n; e++) { theta_out[e] = theta[e]; shift_out[e] = shift[e]; iou_out[e] = iou[e]; }
        return 0;
    } catch (const btba::Error &e) {
        return e.status;
    }
}

// rows_out: double [7][6] = (n, acc_5deg5cm, acc_iou25, rot_err_deg, trans_err, trans_err_cm) of classes 1 .. 6, then overall
extern "C" __attribute__((visibility("default"))) int nocs_report_driver(int n, const double *theta, const double *shift, const double *iou,
                                                                          const int32_t *class_id, const int64_t *n_listed, double rot_thresh_deg,
                                                                          double shift_thresh, double iou_thresh, double *rows_out)
{
    try {
        btba_nocs_params prm = btba::nocsParams();
        prm.rot_thresh_deg = rot_thresh_deg;
        prm.shift_thresh = shift_thresh;
        prm.iou_thresh = iou_thresh;
        std::vector<int64_t> listed;
        if (n_listed) listed.assign(n_listed, n_listed + 6);
        const btba::NocsReport rep = btba::nocsReport(std::vector<double>(theta, theta + n), std::vector<double>(shift, shift + n),
                                                      std::vector<double>(iou, iou + n), std::vector<int32_t>(class_id, class_id + n), listed, prm);
        for (int k = 0; k < 7; k++) {
            const btba::NocsRow &r = k < 6 ? rep.cls[k] : rep.overall;
            const double row[6] = { (double)r.n, r.acc_5deg5cm, r.acc_iou25, r.rot_err_deg, r.trans_err, r.trans_err_cm };
            for (int j = 0; j < 6; j++) rows_out[6 * k + j] = row[j];
        }
        return 0;
    } catch (const btba::Error &e) {
        return e.status;
    }
}
