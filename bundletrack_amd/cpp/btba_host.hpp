// btba_host.hpp -- the host side above the C ABI, in C++ like the reference's own host code.
//
// Mirrors, name for name and argument for argument, what sits on either side of the optimiser boundary in
// wenbowen123/BundleTrack:
//   OptimizerGpu::optimizeFrames                        src/cuda/LossGPU.h:40-52, LossGPU.cu:53-139
//   Bundler::optimizeGPU's marshalling                  src/Bundler.cpp:286-347   (marshalWindow)
//   Bundler::checkAndAddKeyframe / selectKeyFramesForBA src/Bundler.cpp:185-274   (KeyframeMemory)
//   Bundler::processNewFrame / optimizeGPU / saveNewframeResult   src/Bundler.cpp:56-183, 279-359, 362-377   (Bundler)
//   SiftManager::forgetFrame / procrustesByCorrespondence / runRansacMultiPairGPU   src/FeatureManager.cpp:142-170, 523-556, 659-741
//                                                        (FeatureManager: the slice of SiftManager that Bundler calls)
//   Utils::rotationGeodesicDistance                     src/Utils.cpp:42-47
//   Utils::solveRigidTransformBetweenPoints             src/Utils.cpp:180-214     (Kabsch; a 3x3 one-sided Jacobi SVD stands in
//                                                        for Eigen::JacobiSVD)
// The reference builds these on Eigen, yaml-cpp and PCL, none of which exist in this image, so the two value types
// the interface needs are defined here with Eigen's conventions (column-major storage, (row, col) access): a
// maintainer swaps `btba::Matrix4f` for `Eigen::Matrix4f` and `btba::Config` for the YAML node and nothing else
// changes.  Only libbtba.so's C ABI (include/btba.h) is called: plain host C++ (g++), no
// device code, no torch; HIP contributes the float4 / uchar4 pixel types only.
#pragma once
#include <array>
#include <cstdint>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include <hip/hip_vector_types.h>     // float4, uchar4: the device pixel types of the reference's signatures (plain structs on the host)

#include "../../include/btba.h"

namespace btba {

struct Matrix4f {                      // Eigen::Matrix4f: column-major
    float d[16];
    float &operator()(int r, int c) { return d[c * 4 + r]; }
    float operator()(int r, int c) const { return d[c * 4 + r]; }
    static Matrix4f Identity() { Matrix4f M{}; for (int k = 0; k < 4; k++) M(k, k) = 1.0f; return M; }
};
struct Matrix4d {                      // Eigen::Matrix4d: column-major
    double d[16];
    double &operator()(int r, int c) { return d[c * 4 + r]; }
    double operator()(int r, int c) const { return d[c * 4 + r]; }
    static Matrix4d Identity() { Matrix4d M{}; for (int k = 0; k < 4; k++) M(k, k) = 1.0; return M; }
};
struct Matrix3f {                      // Eigen::Matrix3f: column-major
    float d[9];
    float &operator()(int r, int c) { return d[c * 3 + r]; }
    float operator()(int r, int c) const { return d[c * 3 + r]; }
};

using EntryJ = btba_entryj;            // src/cuda/SIFTImageManager.h:44-59, 32 bytes

// The keys of config_ycbineoat.yml the path reads (at their shipping values): bundle.* :23-36, p2p.* :63-65
struct Config {
    int num_iter_outter = 7, num_iter_inner = 5;
    float robust_delta = 0.005f, image_downscale = 4.0f;
    float p2p_max_dist = 0.02f, p2p_max_normal_angle = 45.0f;
    int max_BA_frames = 15, min_fm_edges_newframe = 5;
    float keyframe_min_rot = 10.0f;
    int keyframe_min_feat_num = 0;
    int window_size = 2;                          // bundle.window_size :26 ("exclude keyframes, include new frame")
    int ransac_max_iter = 2000;                   // ransac.* :53-56
    float ransac_inlier_dist = 0.01f;
    bool feature_corres_mutual = true;            // feature_corres.* :46-51
    float feature_corres_max_dist_no_neighbor = 0.02f, feature_corres_max_normal_no_neighbor = 45.0f;
    float feature_corres_max_dist_neighbor = 0.03f, feature_corres_max_normal_neighbor = 45.0f;
    bool mask_largest_component_hull = false;     // the reference's `data_dir contains "NOCS"` (Frame.cpp:255,280): largest component -> hull -> fill
    int mask_dilate = 5;                          // MORPH_RECT 5 x 5 (Frame.cpp:310)
    std::string pose_dir;                         // debug_dir + "/poses/" (:5; Bundler.cpp:366); empty = do not write pose files
};

class Error : public std::runtime_error {       // the reference exits / spins instead (cutil_inline_runtime.h:261-269)
public:
    int status;
    Error(int status_, const std::string &where) : std::runtime_error(where + ": " + btba_strerror(status_)), status(status_) {}
};

class OptimizerGpu {
public:
    std::shared_ptr<Config> yml;
    btba_stats last_stats{};
    bool persistent_frame_cache = false;         // hand frame ids to btba_optimize_frames_keyed (needs frame_ids below)
    std::vector<uint64_t> frame_ids;             // Frame::_id of every window frame, when persistent_frame_cache is set
    bool keyed_correspondences = false;          // with persistent_frame_cache: pair segments stay on the device too (BTBA_FLAG_KEYED_CORR)

    // The reference runs the whole path on the legacy NULL stream (no explicit streams anywhere in src/cuda), so the drop-in
    // does too: depth / normal maps produced by earlier default-stream work are ordered before the cache build.  A caller with
    // its own non-blocking producer stream passes it (the workspace then runs there) or orders with workspace().
    explicit OptimizerGpu(std::shared_ptr<Config> yml1, void *hip_stream = nullptr);
    ~OptimizerGpu();
    btba_workspace *workspace() const { return ws_; }      // btba_workspace_wait_stream / _signal_stream / _frame_cache_evict
    OptimizerGpu(const OptimizerGpu &) = delete;
    OptimizerGpu &operator=(const OptimizerGpu &) = delete;

    // LossGPU.h:50.  poses: camera -> model, updated in place; colors_gpu ignored (weight 0, SBA.cpp:32).
    void optimizeFrames(const std::vector<EntryJ> &global_corres, const std::vector<int> &n_match_per_pair, int n_frames, int H, int W,
                        const std::vector<float *> &depths_gpu, const std::vector<uchar4 *> &colors_gpu, const std::vector<float4 *> &normals_gpu,
                        std::vector<Matrix4f> &poses, const Matrix3f &K);

private:
    btba_workspace *ws_ = nullptr;               // grow-only scratch kept across calls (the reference reallocates everything)
};

// ---- the caller's side -------------------------------------------------------------------------------------
struct Frame {                                   // the fields of Frame (src/Frame.h:45-96) the BA caller touches
    enum Status { FAIL, NO_BA, OTHER };
    int _id = 0;
    std::string _id_str;                         // names the pose file (Bundler.cpp:374)
    Status _status = OTHER;
    Matrix4f _pose_in_model = Matrix4f::Identity();
    int _n_keypts = 0;
    float _roi[4] = { 0.0f, 1e9f, 0.0f, 1e9f };  // (umin, umax, vmin, vmax) of the segmentation mask (Frame.h:81): a frame whose roi is under 10 px wide or high is FAIL (Bundler.cpp:88-93)
    float *_depth_gpu = nullptr;
    float4 *_normal_gpu = nullptr;
    uchar4 *_color_gpu = nullptr;
    int _H = 0, _W = 0;                          // image size and full-resolution intrinsics (Frame.h: _H, _W, _K): the matcher's pixel lookup
    Matrix3f _K{};
    float2 *_kpts_gpu = nullptr;                 // [_n_keypts] keypoints (x, y) on the device (the reference keeps cv::KeyPoint on the host)
    float *_feat_des_gpu = nullptr;              // [_n_keypts][_feat_dim] descriptors on the device (Frame::_feat_des_gpu)
    int _feat_dim = 0;
    uint8_t *_mask_gpu = nullptr;                // [_H * _W] the raw object mask on the device, nonzero = foreground (the mask PNG); null = none
    uint8_t *_fg_mask_gpu = nullptr;             // [_H * _W] caller-owned: receives the final 0 / 1 mask (Frame::_fg_mask); null = not kept
    const uint16_t *_depth_code_gpu = nullptr;   // [_H * _W] the depth PNG's millimetre codes on the device (cv::imread(path, CV_16UC1)); null = the frame arrives with its maps made
    const uint8_t *_bgr_gpu = nullptr;           // [_H * _W * 3] the colour image on the device, imread's layout; null = no colour map is made
    float *_depth_raw_gpu = nullptr;             // [_H * _W] caller-owned: receives the decoded, unfiltered depth (Frame::_depth_raw); null = not kept
    float4 *_xyz_gpu = nullptr;                  // [_H * _W] caller-owned: receives the camera-space points (the xyz of Frame::_cloud); null = not kept
    bool _ingested = false;                      // ingestFrames has filled _depth_gpu / _normal_gpu / _color_gpu from the two images
};

// The body of Frame's constructor after the two imreads (Frame.cpp:45-89, Utils::readDepthImage) on btba_ingest_frames, for many frames
// in one call: _depth_code_gpu decoded to metres, processDepth and depthToCloudAndNormals into the caller-owned _depth_gpu and
// _normal_gpu (the reference's constructor allocates them, :68-70), _bgr_gpu packed into _color_gpu where both are set, _depth_raw_gpu
// and _xyz_gpu filled where set; _ingested = true.  Frames need _depth_code_gpu, _depth_gpu, _normal_gpu, _H, _W, _K (one size and one
// K per call: the first frame's).  params.depth_format must be 0.  Asynchronous on the workspace stream.
btba_ingest_params ingestParams();                                               // btba_ingest_params_default
void ingestFrames(btba_workspace *ws, const std::vector<std::shared_ptr<Frame>> &frames, const btba_ingest_params &params);

// The video segmentation around its backbone (transductive-vos.pytorch/run_video.py, lib/predict.py) on btba_vos_*; the rules are in
// include/btba.h.  vosSampleFrames needs no GPU; the others are asynchronous on the workspace stream and throw Error on a refusal.
// vosPropagate: refs[b] / labels[b] are video b's reference features [C][Hd*Wd] and labels [d][Hd*Wd], oldest first, the last
// n_dense[b] of them with sigma_dense; onehot may be empty (not wanted) or hold null entries.
btba_vos_params vosParams();                                                     // btba_vos_params_default
void vosSampleFrames(const btba_vos_params &params, int frame_idx, std::vector<int> &idx, int &n_dense);
void vosFirstLabels(btba_workspace *ws, int H, int W, int d, const uint8_t *label_dev, float *labels_out_dev);
void vosPropagate(btba_workspace *ws, const btba_vos_params &params, int C, int d, int Hd, int Wd,
                  const std::vector<std::vector<const float *>> &refs, const std::vector<std::vector<const float *>> &labels,
                  const std::vector<const float *> &targets, const std::vector<int> &n_dense, const std::vector<float *> &pred,
                  const std::vector<float *> &onehot);
void vosMasks(btba_workspace *ws, int d, int Hd, int Wd, int H, int W, const float *pred_dev, uint8_t *mask_out_dev);
void vosInputs(btba_workspace *ws, const std::vector<const uint8_t *> &bgr_dev, int H, int W, float *rgb_out_dev);

// One video's propagation state: run_video.py's feats_history / label_history as a device ring of range + 5 slots (no frame older
// than frame_idx - range - 4 is ever sampled; the reference keeps every frame).  The memory is the caller's, as a Frame's maps are:
//   feats [slots()][C][Hd*Wd] float, labels [slots()][d][Hd*Wd] float, pred [d][Hd*Wd] float, mask [H*W] uint8.
// The backbone writes a frame's features straight into nextFeatures() -- the slot the frame will occupy -- and then start(label_dev)
// (the annotated frame 0; a uint8 [H*W] label image with classes 0 .. d-1) or step() (every later frame: predict against the
// sampled history, the one-hot labels into the ring, the class map into `mask`) takes the frame into the history.
class MaskPropagator {
public:
    btba_workspace *ws;
    int d, H, W, C, Hd, Wd;
    btba_vos_params params;
    float *feats, *labels, *pred;
    uint8_t *mask;
    int n_frames = 0;                                               // frames in the history = the next frame_idx

    MaskPropagator(btba_workspace *ws1, int d1, int H1, int W1, int C1, const btba_vos_params &params1, float *feats_dev, float *labels_dev,
                   float *pred_dev, uint8_t *mask_dev);
    int slots() const { return params.range + 5; }
    float *featuresOf(int frame) const { return feats + (size_t)(frame % slots()) * C * Hd * Wd; }
    float *labelsOf(int frame) const { return labels + (size_t)(frame % slots()) * d * Hd * Wd; }
    float *nextFeatures() const { return featuresOf(n_frames); }
    void start(const uint8_t *label_dev);
    const uint8_t *step();                                          // returns `mask`
};

// Frame::segmentationByMaskFile (Frame.cpp:236-373) minus the PNG read, on btba_apply_masks: optionally the largest 8-connected
// component's filled convex hull, a dilate x dilate dilation, colour / depth / normals zeroed outside the mask in place, _roi set and
// the final mask written to _fg_mask_gpu when that is set.  Frames need _mask_gpu, _depth_gpu, _normal_gpu, _H, _W (one size per
// call); _color_gpu may be null.  Needs the GPU; synchronous (the ROIs come back to the host).
void segmentationByMask(btba_workspace *ws, const std::shared_ptr<Frame> &frame, bool largest_component_hull, int dilate = 5);
void segmentationByMaskMultiFrame(btba_workspace *ws, const std::vector<std::shared_ptr<Frame>> &frames, bool largest_component_hull, int dilate = 5);

// Lfnet::detectFeature (FeatureManager.cpp:811-908, rot_deg = 0) minus the detector, on btba_detector_inputs and
// btba_detector_keypoints_to_image.  prepareDetectorInputs: the frames' masked _color_gpu cropped to _roi, zero-padded to a square
// and resized to out_size x out_size, into caller-owned device buffers bgr_out [n][S][S][3] uint8 and gray_out [n][S][S] float (either
// may be null).  keypointsToImage: n keypoints in detector pixels (device float2) mapped back to full-resolution pixels into kpts_out
// (may equal kpts_in), which becomes the frame's _kpts_gpu; _n_keypts = n.  Both asynchronous on the workspace stream.
void prepareDetectorInputs(btba_workspace *ws, const std::vector<std::shared_ptr<Frame>> &frames, uint8_t *bgr_out, float *gray_out, int out_size = 400);
void keypointsToImage(btba_workspace *ws, const std::shared_ptr<Frame> &frame, const float2 *kpts_in, int n, float2 *kpts_out, int out_size = 400);

// scripts/eval_ycbineoat.py's per-frame errors (Utils.py add / adi) on btba_pose_errors: evaluation e scores poses_pred[e] against
// poses_gt[e] (object-in-camera, Bundler::saveNewframeResult's ob_in_cam) on the device point set models_dev[model_index[e]]
// (float [n_pts[m]][3], metres).  add and adds are resized to the number of evaluations.  Needs the GPU; synchronous.
void poseErrors(btba_workspace *ws, const std::vector<const float *> &models_dev, const std::vector<int32_t> &n_pts,
                const std::vector<int32_t> &model_index, const std::vector<Matrix4f> &poses_pred, const std::vector<Matrix4f> &poses_gt,
                std::vector<float> &add, std::vector<float> &adds);

// scripts/benchmark.py's per-frame figures (compute_RT_degree_cm_symmetry, compute_3d_iou_new as called at :262-272) on
// btba_nocs_errors: item e scores poses_pred[e] against poses_gt[e] (object-in-camera, translation in the unit of
// params.shift_thresh) as class class_id[e] (1 .. 6) with the box boxes[box_index[e]] (8 corner rows of 3, row-major).
// handle_visible may be empty (all visible).  theta_deg, shift and iou are resized to the number of items.  Needs the GPU; synchronous.
using NocsBox = std::array<double, 24>;
btba_nocs_params nocsParams();                                                   // btba_nocs_params_default
void nocsErrors(btba_workspace *ws, const btba_nocs_params &params, const std::vector<NocsBox> &boxes, const std::vector<int32_t> &class_id,
                const std::vector<int32_t> &handle_visible, const std::vector<int32_t> &box_index, const std::vector<Matrix4d> &poses_pred,
                const std::vector<Matrix4d> &poses_gt, std::vector<double> &theta_deg, std::vector<double> &shift, std::vector<double> &iou);
// benchmark.py:276-319 for one experiment, the same arithmetic in the same order as bundletrack_amd/nocs_eval.py::nocs_report (the two
// agree bit for bit): cls[c - 1] is the row of class c, overall the sum over the classes of (row value / 6).  n_listed: empty (each
// class's number of items) or 6 counts, class 1 first (the reference's cls_num).  Host only.
struct NocsRow { int64_t n = 0; double acc_5deg5cm = 0, acc_iou25 = 0, rot_err_deg = 0, trans_err = 0, trans_err_cm = 0; };
struct NocsReport { NocsRow cls[6]; NocsRow overall; };
NocsReport nocsReport(const std::vector<double> &theta_deg, const std::vector<double> &shift, const std::vector<double> &iou,
                      const std::vector<int32_t> &class_id, const std::vector<int64_t> &n_listed, const btba_nocs_params &params);
// Window assembly on the device (include/btba.h, "window assembly"): thin wrappers over the C ABI.
// windowLayout (host-only): seg_counts[w * P + p] matches of canonical pair p of window w, newframe_index[w] -> the layout.
// marshalWindows: the chain's device records + a device segment table uint32 [n_windows][P][2] = (first record, count) -> corr_dev,
// pair_offsets_dev and (optional, may be null) corr24_dev, all caller-owned device buffers; asynchronous on the workspace stream.
// procrustesPairs: the Kabsch fit of pair e = segments[e] = (first record, count) with the camera -> model poses of the newer (A) and
// the older (B) frame; poses and err are resized to the number of pairs.  Needs the GPU; synchronous.
struct WindowLayout {
    int64_t corr_stride = 0;
    uint32_t max_corr_per_pair = 0;
    std::vector<uint32_t> pair_offsets;                                          // [n_windows][P + 1]
    std::vector<int64_t> n_edges_newframe;                                       // [n_windows]
    std::vector<int32_t> run_ba;                                                 // [n_windows]: 1 = n_edges_newframe > min_fm_edges_newframe
};
WindowLayout windowLayout(int n_frames, const std::vector<int32_t> &seg_counts, const std::vector<int32_t> &newframe_index, int min_fm_edges_newframe = 5);
void marshalWindows(btba_workspace *ws, int n_windows, int n_frames, const btba_match *matches_dev, int64_t n_records, const uint32_t *segments_dev,
                    const WindowLayout &layout, btba_entryj *corr_dev, uint32_t *pair_offsets_dev, float *corr24_dev = nullptr);
void procrustesPairs(btba_workspace *ws, const btba_match *matches_dev, int64_t n_records, const std::vector<std::pair<int32_t, int32_t>> &segments,
                     const std::vector<Matrix4f> &posesA, const std::vector<Matrix4f> &posesB, std::vector<Matrix4f> &poses, std::vector<float> &err);

// Pose covariances (include/btba.h, "pose covariances"): thin wrappers over the C ABI, all pointers device pointers, both asynchronous on the
// workspace stream.  linearizeBatchZn: the arguments of btba_solve_batch_zn_aux with const poses -> info_dev float [n_instances][na][na]
// (na = 6 (n_frames - 1), the public (rot, trans) order) and, unless null, rhs_dev float [n_instances][n_frames - 1][6]; dense_pairs empty: the
// pair policy's default list.  poseCovariances: info (contiguous instances) -> cov_blocks_dev double [n_instances][n_frames][6][6],
// status_dev int32 [n_instances] and, unless null, cov_full_dev double [n_instances][na][na] and pivot_ratio_dev double [n_instances].
void linearizeBatchZn(btba_workspace *ws, const btba_params &params, int n_instances, int n_frames, int H, int W, const Matrix3f &K, const float *zn_dev,
                      const btba_zn_aux *aux, const btba_entryj *corr_dev, int64_t corr_stride, const uint32_t *pair_offsets_dev, uint32_t max_corr_per_pair,
                      const std::vector<std::pair<int32_t, int32_t>> &dense_pairs, const float *poses_dev, float *info_dev, float *rhs_dev = nullptr);
void poseCovariances(btba_workspace *ws, int n_instances, int n_frames, const float *info_dev, double *cov_blocks_dev, int32_t *status_dev,
                     double *cov_full_dev = nullptr, double *pivot_ratio_dev = nullptr);

// Objective report (include/btba.h, "objective report"): the arguments of linearizeBatchZn -> total_dev btba_objective_total [n_instances] and,
// unless null, sparse_dev btba_objective_pair [n_instances][n_frames (n_frames - 1) / 2] and dense_dev [n_instances][dense pairs]; asynchronous.
// residualVariance: objective / (n_residuals - 6 (n_frames - 1)) of a total copied to the host, NaN where that is not positive -- what scales the
// covariances of poseCovariances.
void objectiveBatchZn(btba_workspace *ws, const btba_params &params, int n_instances, int n_frames, int H, int W, const Matrix3f &K, const float *zn_dev,
                      const btba_zn_aux *aux, const btba_entryj *corr_dev, int64_t corr_stride, const uint32_t *pair_offsets_dev, uint32_t max_corr_per_pair,
                      const std::vector<std::pair<int32_t, int32_t>> &dense_pairs, const float *poses_dev, btba_objective_total *total_dev,
                      btba_objective_pair *sparse_dev = nullptr, btba_objective_pair *dense_dev = nullptr);
double residualVariance(const btba_objective_total &total, int n_frames);

// Keyframe fusion and voxel-grid downsampling (include/btba.h, "keyframe fusion"): posed frames and point lists -> one voxel-grid cloud per
// instance, Utils::downsamplePointCloud (Utils.cpp:134-140) included.  ObjectCloudBuffers: the caller's device outputs, `capacity` records per
// instance; normal, colour, count and lin may be null.  fuseBounds writes VoxelGrid's data-derived box of every instance to device memory
// (int32 [n_instances][6]); the caller copies it to the host and passes it as `box`.  All three are asynchronous on the workspace stream.
struct ObjectCloudBuffers {
    int capacity = 0;
    float4 *xyz = nullptr, *normal = nullptr;
    uchar4 *colour = nullptr;
    uint32_t *count = nullptr;
    int32_t *lin = nullptr;
    int32_t *n_out = nullptr, *n_outside = nullptr, *status = nullptr;       // [n_instances] each
};
btba_fuse_segment frameSegment(int instance, const Matrix4f &pose_in_model, const float *depth_gpu, const float4 *normal_gpu, const uchar4 *color_gpu);
btba_fuse_segment pointSegment(int instance, const Matrix4f &pose, const float4 *xyz_gpu, int64_t n, const float4 *normal_gpu = nullptr,
                               const uchar4 *color_gpu = nullptr);
void fuseBounds(btba_workspace *ws, const btba_fuse_params &params, int n_instances, const std::vector<btba_fuse_segment> &segments, int H, int W,
                const Matrix3f &K, int32_t *box_dev);
void fuseFrames(btba_workspace *ws, const btba_fuse_params &params, int n_instances, const std::vector<btba_fuse_segment> &segments, int H, int W,
                const Matrix3f &K, const std::vector<int32_t> &box, const ObjectCloudBuffers &out);
void voxelDownsample(btba_workspace *ws, const btba_fuse_params &params, const std::vector<const float4 *> &xyz_gpu, const std::vector<int64_t> &n_points,
                     const std::vector<int32_t> &box, const ObjectCloudBuffers &out, const std::vector<const float4 *> &normal_gpu = {},
                     const std::vector<const uchar4 *> &color_gpu = {});

// Frame-to-model registration (include/btba.h, "frame-to-model registration"): point-to-plane ICP of frame and point-list segments (frameSegment /
// pointSegment with the INITIAL pose) against the cloud fuseFrames / voxelDownsample wrote -- fuse it with normalize_normals = 1.  registerIndex
// builds the cell index (int32 [V] of the caller, V from btba_fuse_layout) once per cloud; registerFrames writes pose_out_dev (float
// [n_items][12]), result_dev and, unless null, trace_dev ([n_items][params.n_iters]).  n_iters = 0 is the pose check.  Both asynchronous.
void registerIndex(btba_workspace *ws, int n_instances, const std::vector<int32_t> &box, const ObjectCloudBuffers &cloud, int32_t *cell_index_dev);
void registerFrames(btba_workspace *ws, const btba_register_params &params, int n_instances, const std::vector<btba_fuse_segment> &items, int H, int W,
                    const Matrix3f &K, const std::vector<int32_t> &box, const ObjectCloudBuffers &cloud, const int32_t *cell_index_dev, float *pose_out_dev,
                    btba_register_result *result_dev, btba_register_iter *trace_dev = nullptr);

// The device keyframe memory (include/btba.h, "device keyframe memory"): checkAndAddKeyframe and selectKeyFramesForBA for n_sessions tracking
// sessions at once, on device memory.  Owns the btba_keyframes handle, whose buffers free themselves; move-only.  Every per-session argument
// is a device array [n_sessions], `active` (int32, nonzero = take part) may be null: all sessions.  All calls but exportPools are asynchronous
// on the workspace stream.  rotationDistances is the memory's distance for n pose pairs (row-major 4 x 4 floats on the device).
struct KeyframeWindows {                 // device outputs of select, rows ordered by frame id; the caller's memory
    int32_t *n_window = nullptr;         // [S]
    int32_t *slot = nullptr;             // [S][max_BA]: the pool slot, -1 for the new frame
    int32_t *frame_id = nullptr;         // [S][max_BA]
    uint64_t *frame_key = nullptr;       // [S][max_BA]
    float *pose = nullptr;               // [S][max_BA][16]
    int32_t *newframe_index = nullptr;   // [S]
};
struct KeyframePools {                   // host copy of the pools
    std::vector<int32_t> count, overflow, frame_id;
    std::vector<uint64_t> frame_key;
    std::vector<float> poses;
};
class DeviceKeyframeMemory {
public:
    DeviceKeyframeMemory(btba_workspace *ws, int n_sessions, int capacity, int max_BA_frames, float min_rot_deg = 10.0f, int min_feat_num = 0);
    ~DeviceKeyframeMemory();
    DeviceKeyframeMemory(const DeviceKeyframeMemory &) = delete;
    DeviceKeyframeMemory &operator=(const DeviceKeyframeMemory &) = delete;
    DeviceKeyframeMemory(DeviceKeyframeMemory &&o) noexcept;
    void reset(int session = -1);
    void checkAndAddKeyframes(const float *pose_dev, const int32_t *frame_id_dev, const uint64_t *frame_key_dev, const int32_t *status_other_dev,
                              const int32_t *n_keypts_dev, int32_t *added_out_dev, const int32_t *active_dev = nullptr);
    void selectKeyFramesForBA(const float *newpose_dev, const int32_t *new_frame_id_dev, const uint64_t *new_frame_key_dev, const KeyframeWindows &out,
                              const int32_t *active_dev = nullptr);
    void writeback(const int32_t *n_window_dev, const int32_t *window_slot_dev, const float *pose_dev, const int32_t *active_dev = nullptr);
    KeyframePools exportPools();
    int n_sessions() const { return n_sessions_; }
    int capacity() const { return capacity_; }
    int max_BA_frames() const { return max_BA_; }
    float min_rot_deg;
    int min_feat_num;
private:
    btba_keyframes *kf_ = nullptr;
    int n_sessions_ = 0, capacity_ = 0, max_BA_ = 0;
};
void rotationDistances(btba_workspace *ws, int n, const float *A_dev, const float *B_dev, float *dist_out_dev);

// VOCap (eval_ycbineoat.py:54-81) in closed form, the same arithmetic as bundletrack_amd/evaluation.py::vocap_auc: the area under
// the accuracy-vs-threshold curve on [0, max_threshold] over max_threshold (0 without errors below the threshold).
double vocapAuc(const std::vector<double> &errors, double max_threshold = 0.1);

// Utils::solveRigidTransformBetweenPoints (Utils.cpp:180-214): the rigid transform points1 -> points2 (n x 3 each, xyz
// triples), identity when fewer than 3 points, a non-orthonormal V U^T or a non-finite result.
void solveRigidTransformBetweenPoints(const std::vector<float> &points1, const std::vector<float> &points2, Matrix4f &pose);

// `ff << std::setprecision(10) << ob_in_cam << std::endl` (Bundler.cpp:372-377) with Eigen's default IOFormat: %.10g
// coefficients, right-aligned to the widest one, one space between columns, one row per line.
std::string formatPoseTxt(const Matrix4f &ob_in_cam);

float rotationGeodesicDistance(const Matrix4f &A, const Matrix4f &B);           // rotation blocks only, radians (Utils.cpp:42-47)

struct Correspondences { std::vector<float> ptA_cam, ptB_cam; };                // xyz triples; A = the newer frame

struct Window {                                                                  // what optimizeGPU hands to optimizeFrames
    std::vector<std::shared_ptr<Frame>> frames;                                  // sorted by id: index 0 is never moved
    std::vector<EntryJ> global_corres;
    std::vector<int> n_match_per_pair;
    int n_edges_newframe = 0;
    bool run_ba = false;                                                         // false <=> newframe->_status = NO_BA (:343-347)
};
// Bundler.cpp:286-347.  matches: keyed by (newer frame id, older frame id) like _fm->_matches[{frameA, frameB}].
Window marshalWindow(std::vector<std::shared_ptr<Frame>> local_frames, const std::map<std::pair<int, int>, Correspondences> &matches,
                     const std::shared_ptr<Frame> &newframe, int min_fm_edges_newframe);

class KeyframeMemory {
public:
    std::vector<std::shared_ptr<Frame>> _keyframes;
    explicit KeyframeMemory(std::shared_ptr<Config> yml1) : yml(std::move(yml1)) {}
    bool checkAndAddKeyframe(const std::shared_ptr<Frame> &frame);                                     // Bundler.cpp:185-219
    std::vector<std::shared_ptr<Frame>> selectKeyFramesForBA(const std::shared_ptr<Frame> &newframe);  // :222-274, sorted by id
private:
    std::shared_ptr<Config> yml;
};

// The slice of SiftManager (src/FeatureManager.h:86-130) that Bundler calls.  Feature detection and matching themselves are out of
// scope (LF-Net over zmq, OpenCV): findCorres is the hook a tracker fills in; what the reference does with
// the matches afterwards is implemented here.
class FeatureManager {
public:
    std::map<std::pair<int, int>, Correspondences> _matches;        // _matches[{frameA, frameB}], keyed (newer id, older id)
    virtual ~FeatureManager() = default;
    virtual void detectFeature(const std::shared_ptr<Frame> & /*frame*/) {}
    // fills _matches[{frameA->_id, frameB->_id}] unless present (:176); may mark frameA FAIL
    virtual void findCorres(const std::shared_ptr<Frame> &frameA, const std::shared_ptr<Frame> &frameB) = 0;
    virtual void forgetFrame(const std::shared_ptr<Frame> &frame);                                                   // :142-170
    // Bundler::optimizeGPU's opt-in: a feature manager that runs a window's pairs (findCorres order) in one call does so and returns
    // true (GpuFeatureManager); the default does nothing and returns false, and the Bundler then calls findCorres pair by pair.
    virtual bool findCorresChain(const std::vector<std::pair<std::shared_ptr<Frame>, std::shared_ptr<Frame>>> & /*pairs*/) { return false; }
    int countInlierCorres(const std::shared_ptr<Frame> &frameA, const std::shared_ptr<Frame> &frameB) const;          // :746-758
    // :523-556: Kabsch of the matches moved into the model frame with the frames' current poses; identity below 5 matches
    virtual Matrix4f procrustesByCorrespondence(const std::shared_ptr<Frame> &frameA, const std::shared_ptr<Frame> &frameB);
    // :659-741 on btba_ransac_pairs (one call for all pairs; the reference's cuRAND triples and procrustesKernel hypotheses):
    // every pair's matches are replaced by their RANSAC inliers, or emptied when fewer than 5 survive.  Needs the GPU.
    void runRansacMultiPairGPU(btba_workspace *ws, const std::vector<std::pair<std::shared_ptr<Frame>, std::shared_ptr<Frame>>> &pairs,
                               int max_iter, float inlier_dist);
    // :370-437 on btba_match_pairs (one call for all pairs, in place of OpenCV's CUDA brute-force matcher): every pair's matches --
    // A -> B, then B -> A with feature_corres.mutual -- are APPENDED to _matches[{A, B}].  Needs the GPU and yml (the shipping
    // values when it is null); frames need _kpts_gpu, _feat_des_gpu, _feat_dim, _depth_gpu, _normal_gpu, _H, _W, _K.
    std::shared_ptr<Config> yml;
    void findCorresbyNNMultiPair(btba_workspace *ws, const std::vector<std::pair<std::shared_ptr<Frame>, std::shared_ptr<Frame>>> &pairs);
    // :247-288: one pair (A newer); a neighbouring pair left with fewer than 5 matches marks A FAIL
    void findCorresbyNN(btba_workspace *ws, const std::shared_ptr<Frame> &frameA, const std::shared_ptr<Frame> &frameB);
};

// Lfnet (src/FeatureManager.h:124-136) with the zmq round trip replaced by an in-process detector: detectFeature makes the
// detector's input on the device (prepareDetectorInputs into the caller's bgr / gray buffers), calls `detect` and maps the returned
// keypoints back in place (keypointsToImage); _kpts_gpu, _n_keypts, _feat_des_gpu and _feat_dim come from what `detect` returns,
// whose device memory it owns.  The buffers are written, and the keypoints read, on the workspace stream: a detector on another
// stream orders itself with it (btba_workspace_wait_stream / _signal_stream).  An exception from `detect` reaches Bundler::processNewFrame, which marks the frame FAIL (:108-117).
// findCorres stays the caller's hook, as in FeatureManager.
struct DetectedFeatures {
    float2 *kpts_dev = nullptr;                  // [n] keypoints (x, y) in detector pixels; overwritten with full-resolution pixels
    float *desc_dev = nullptr;                   // [n][dim] descriptors
    int n = 0, dim = 0;
};
class DetectorFeatureManager : public FeatureManager {
public:
    using DetectFn = std::function<DetectedFeatures(const uint8_t *bgr_dev, const float *gray_dev, int out_size)>;
    // bgr_dev: device uint8 [S][S][3], gray_dev: device float [S][S] (either may be null; the detector gets what is set)
    DetectorFeatureManager(btba_workspace *ws, DetectFn detect, uint8_t *bgr_dev, float *gray_dev, int out_size = 400)
        : ws_(ws), detect_(std::move(detect)), bgr_(bgr_dev), gray_(gray_dev), out_size_(out_size) {}
    void detectFeature(const std::shared_ptr<Frame> &frame) override;
private:
    btba_workspace *ws_;
    DetectFn detect_;
    uint8_t *bgr_;
    float *gray_;
    int out_size_;
};

// LF-Net's keypoint head between its two conv nets (inference.py::build_multi_scale_deep_detector_3DNMS and build_patch_extraction)
// on btba_lfnet_keypoints; the rules are in include/btba.h.  Every buffer is the caller's device memory.
btba_lfnet_params lfnetParams();                                                 // btba_lfnet_params_default
struct LfnetMapSet {                             // the score net's output for n frames
    std::vector<const float *> score_dev;        // [S] device float [n][h_s][w_s]
    std::vector<int32_t> map_h, map_w;           // [S]
    std::vector<float> scale_factors;            // [S]
};
struct LfnetBuffers {                            // per frame: what btba_lfnet_keypoints writes, sizes in include/btba.h
    float *max_heatmaps = nullptr, *max_scales = nullptr;            // [n][H][W]
    int32_t *kpts_xy = nullptr, *n_kpts = nullptr;                   // [n][top_k][2], [n]
    float *kpts = nullptr, *kpts_scale = nullptr, *kpts_ori = nullptr, *patches = nullptr;      // [n][top_k][2], [n][top_k], [n][top_k][2], [n][top_k][P][P]
};
// A, B and C for n_frames in one call.  Returns the keypoint counts (one host wait at the end); throws Error on a refusal.
std::vector<int> lfnetKeypoints(btba_workspace *ws, const btba_lfnet_params &params, int n_frames, int H, int W, const LfnetMapSet &maps,
                                const float *photo_dev, const float *ori_dev, const LfnetBuffers &out);

// The detector DetectorFeatureManager takes, around the caller's two conv nets:
//   score_net(gray_dev [S][S]) -> the score maps of one frame (LfnetMapSet) and ori_maps device float [S][S][2]
//   desc_net(patches_dev [m][P][P], m) -> descriptors device float [m][dim]
// with lfnetKeypoints in between; the keypoints returned are out.kpts (refined, in detector pixels).
class LfnetDetector {
public:
    using ScoreFn = std::function<LfnetMapSet(const float *gray_dev, int out_size, const float *&ori_dev)>;
    using DescFn = std::function<float *(const float *patches_dev, int m, int &dim)>;
    LfnetDetector(btba_workspace *ws, ScoreFn score_net, DescFn desc_net, const btba_lfnet_params &params, const LfnetBuffers &out)
        : ws_(ws), score_(std::move(score_net)), desc_(std::move(desc_net)), params_(params), out_(out) {}
    DetectedFeatures operator()(const uint8_t *bgr_dev, const float *gray_dev, int out_size) const;
private:
    btba_workspace *ws_;
    ScoreFn score_;
    DescFn desc_;
    btba_lfnet_params params_;
    LfnetBuffers out_;
};

// What LfnetDescriptor and LfnetScoreNet are built on: a model of the library on a workspace, created from a configuration and host
// arrays by `create` (named `where` in the Error of a refusal) and destroyed with the object by `destroy`; move-only.
template <class Config, class Model> class LfnetModelHolder {
public:
    LfnetModelHolder(const LfnetModelHolder &) = delete;
    LfnetModelHolder &operator=(const LfnetModelHolder &) = delete;
    LfnetModelHolder(LfnetModelHolder &&o) noexcept : ws_(o.ws_), config_(o.config_), model_(o.model_), destroy_(o.destroy_) { o.model_ = nullptr; }
    ~LfnetModelHolder() { destroy_(model_); }
    const Config &config() const { return config_; }
    const Model *model() const { return model_; }
protected:
    template <class Weights>
    LfnetModelHolder(btba_workspace *ws, const Config &config, const Weights &weights,
                     int (*create)(btba_workspace *, const Config *, const Weights *, Model **), void (*destroy)(Model *), const char *where)
        : ws_(ws), config_(config), destroy_(destroy)
    {
        const int rc = create(ws, &config, &weights, &model_);
        if (rc != BTBA_OK) throw Error(rc, where);
    }
    btba_workspace *ws_;
    Config config_;
    Model *model_ = nullptr;
    void (*destroy_)(Model *);
};

// LF-Net's descriptor net (models/simple_desc.py::get_model in inference) on btba_lfnet_descriptors; the rules are in include/btba.h.
btba_lfnet_desc_config lfnetDescConfig();                                        // btba_lfnet_desc_config_default
// patches_dev float [n_frames][slots][P][P] -> desc_dev float [n_frames][slots][out_dim]; n_kpts_dev int32 [n_frames] on the device or
// nullptr for all slots.  Asynchronous on the workspace stream; throws Error on a refusal.
void lfnetDescriptors(btba_workspace *ws, const btba_lfnet_desc_model *model, int n_frames, int slots, const float *patches_dev,
                      const int32_t *n_kpts_dev, float *desc_dev);
// A model on a workspace (created from host arrays in TensorFlow's layouts, destroyed with the object; move-only).  asDescNet gives
// the LfnetDetector::DescFn that writes into the caller's desc_dev [top_k][out_dim].
class LfnetDescriptor : public LfnetModelHolder<btba_lfnet_desc_config, btba_lfnet_desc_model> {
public:
    LfnetDescriptor(btba_workspace *ws, const btba_lfnet_desc_config &config, const btba_lfnet_desc_weights &weights)
        : LfnetModelHolder(ws, config, weights, btba_lfnet_desc_model_create, btba_lfnet_desc_model_destroy, "btba_lfnet_desc_model_create") {}
    void describe(int n_frames, int slots, const float *patches_dev, const int32_t *n_kpts_dev, float *desc_dev) const
    {
        lfnetDescriptors(ws_, model_, n_frames, slots, patches_dev, n_kpts_dev, desc_dev);
    }
    LfnetDetector::DescFn asDescNet(float *desc_dev) const;
};

// LF-Net's detector net (models/mso_resnet_detector.py::get_model in inference) on btba_lfnet_scores; the rules are in include/btba.h.
btba_lfnet_det_config lfnetDetConfig();                                          // btba_lfnet_det_config_default
std::vector<double> lfnetDetScales(double min_scale, double max_scale, int num_scales);      // btba_lfnet_det_scales
// A model on a workspace (created from host arrays in TensorFlow's layouts, destroyed with the object; move-only).  scores() fills the
// caller's maps.score_dev[j] (device float [n][map_h[j]][map_w[j]], sizes from mapSet) and ori_dev [n][H][W][2], asynchronously on the
// workspace stream.  asScoreNet gives the LfnetDetector::ScoreFn that writes one frame into the caller's buffers.
class LfnetScoreNet : public LfnetModelHolder<btba_lfnet_det_config, btba_lfnet_det_model> {
public:
    LfnetScoreNet(btba_workspace *ws, const btba_lfnet_det_config &config, const btba_lfnet_det_weights &weights)
        : LfnetModelHolder(ws, config, weights, btba_lfnet_det_model_create, btba_lfnet_det_model_destroy, "btba_lfnet_det_model_create") {}
    int padSize() const { return btba_lfnet_det_pad_size(model_); }
    // the map sizes and scale factors for H x W frames over the caller's per-scale buffers
    LfnetMapSet mapSet(int H, int W, const std::vector<float *> &score_dev) const;
    void scores(int n_frames, int H, int W, const float *photo_dev, const std::vector<float *> &score_dev, float *ori_dev) const;
    LfnetDetector::ScoreFn asScoreNet(std::vector<float *> score_dev, float *ori_dev) const;
};

// SiftManager::findCorres (FeatureManager.cpp:173-240) with its map points on btba_corres_chain: NN, propagation along the map
// points, RANSAC (ransac.max_iter / inlier_dist of yml), the map-point update and the FAIL gates for an ordered list of pairs in one
// call, the frames' map points in a btba_mappoints on `ws` (a frame is registered at its first pair, by _id; forgetFrame frees its
// slot).  Frames need _kpts_gpu, _feat_des_gpu, _feat_dim, _depth_gpu, _normal_gpu, _H, _W, _K.  _records keeps the btba_match
// records of every pair (propagated ones: dir = 2).  Needs the GPU; every call is synchronous.
class GpuFeatureManager : public FeatureManager {
public:
    std::map<std::pair<int, int>, std::vector<btba_match>> _records;
    explicit GpuFeatureManager(btba_workspace *ws, std::shared_ptr<Config> yml1 = nullptr);
    ~GpuFeatureManager() override;
    GpuFeatureManager(const GpuFeatureManager &) = delete;
    GpuFeatureManager &operator=(const GpuFeatureManager &) = delete;
    void findCorres(const std::shared_ptr<Frame> &frameA, const std::shared_ptr<Frame> &frameB) override;
    bool findCorresChain(const std::vector<std::pair<std::shared_ptr<Frame>, std::shared_ptr<Frame>>> &pairs) override;
    void forgetFrame(const std::shared_ptr<Frame> &frame) override;
private:
    btba_workspace *ws_;
    btba_mappoints *mp_ = nullptr;
    std::map<int, int32_t> slots_;                                  // frame id -> slot
};

// Bundler (src/Bundler.h, Bundler.cpp:56-377) from the point where a frame has its depth and normals on the device -- or, for a
// frame with _depth_code_gpu set and _ingested false, from its images: ingestFrames (default parameters) on the segmentation's
// workspace makes the maps first.  With `segmenter` and `mask_propagator` set, a frame with _bgr_gpu and no _mask_gpu then gets its mask
// from the video segmentation (run_video.py's loop body).  Then the
// segmentation by its mask when _mask_gpu is set (segmentationByMask on mask_ws, or on the workspace of the Bundler's own
// OptimizerGpu when mask_ws is null), pose initialisation from the previous frame, the sliding window, the keyframe subset, bundle adjustment, keyframe insertion,
// the pose file.  `optimize` defaults to one persistent OptimizerGpu (the reference constructs a new one per call, :349);
// tests inject a CPU stand-in with the same signature.
class Bundler {
public:
    using OptimizeFn = std::function<void(const std::vector<EntryJ> &, const std::vector<int> &, int, int, int, const std::vector<float *> &,
                                          const std::vector<uchar4 *> &, const std::vector<float4 *> &, std::vector<Matrix4f> &, const Matrix3f &)>;
    std::shared_ptr<Config> yml;
    std::shared_ptr<FeatureManager> _fm;
    std::deque<std::shared_ptr<Frame>> _frames;
    std::vector<std::shared_ptr<Frame>> _local_frames;
    std::shared_ptr<Frame> _newframe;
    bool _need_reinit = false;
    KeyframeMemory memory;                                          // _keyframes + checkAndAddKeyframe + selectKeyFramesForBA
    Matrix3f K{};
    int H = 0, W = 0;
    int n_ba_calls = 0;
    Window last_window;                                             // what the last optimizeGPU marshalled
    btba_workspace *mask_ws = nullptr;                              // the caller's workspace for the segmentation (not owned)
    // The video segmentation's backbone (the caller's own model, or VosBackbone::asSegmenter on btba_vos_features): normalised RGB float
    // [3][H][W] on the device -> features float [C][Hd][Wd] written to features_out_dev.  With it and a mask_propagator set (both off by default) a frame with _bgr_gpu and no _mask_gpu gets its mask
    // from the propagation; a frame that brings its mask while the propagator is empty is the annotated first frame.  rgb_dev is the
    // caller's float [3][H][W] buffer the normalised image goes to.
    using SegmentFn = std::function<void(const float *rgb_dev, float *features_out_dev)>;
    SegmentFn segmenter;
    std::shared_ptr<MaskPropagator> mask_propagator;
    float *rgb_dev = nullptr;

    Bundler(std::shared_ptr<Config> yml1, std::shared_ptr<FeatureManager> fm, const Matrix3f &K1, int H1, int W1, OptimizeFn optimize = {});
    void processNewFrame(std::shared_ptr<Frame> frame);             // :56-183
    void optimizeGPU();                                             // :279-359
    void saveNewframeResult();                                      // :362-377: <pose_dir>/<_id_str>.txt = inverse(pose_in_model), 10 digits
    const std::vector<std::shared_ptr<Frame>> &keyframes() const { return memory._keyframes; }

private:
    OptimizeFn optimize_;
    std::unique_ptr<OptimizerGpu> own_opt_;                         // created at the first BA call when no OptimizeFn was given
};

// The video segmentation's backbone (modeling/network.py::VOSNet in eval mode) on btba_vos_features; the rules are in include/btba.h.
btba_vos_net_config vosNetConfig();                                              // btba_vos_net_config_default
// A model on a workspace (created from host arrays in PyTorch's layouts, one record per convolution in the forward order of
// include/btba.h; destroyed with the object; move-only).  features() takes rgb_dev float [n][3][H][W] to features_out_dev float
// [n][256][Hd][Wd], asynchronously on the workspace stream.  asSegmenter gives the Bundler::SegmentFn for frames of H x W.
class VosBackbone {
public:
    VosBackbone(btba_workspace *ws, const btba_vos_net_config &config, const std::vector<btba_vos_net_layer> &layers);
    VosBackbone(const VosBackbone &) = delete;
    VosBackbone &operator=(const VosBackbone &) = delete;
    VosBackbone(VosBackbone &&o) noexcept : ws_(o.ws_), config_(o.config_), model_(o.model_) { o.model_ = nullptr; }
    ~VosBackbone() { btba_vos_net_model_destroy(model_); }
    const btba_vos_net_config &config() const { return config_; }
    const btba_vos_net_model *model() const { return model_; }
    void features(int n_frames, int H, int W, const float *rgb_dev, float *features_out_dev) const;
    Bundler::SegmentFn asSegmenter(int H, int W) const;
private:
    btba_workspace *ws_;
    btba_vos_net_config config_;
    btba_vos_net_model *model_ = nullptr;
};

// Eigen's inverse() for a general 4x4, computed in double (used for the pose files)
Matrix4f inverse(const Matrix4f &M);

// One bundle-adjustment call as a file (the layout is documented in bundletrack_amd/problem_io.py, which writes and reads
// the same bytes): what Bundler::optimizeGPU hands to OptimizerGpu::optimizeFrames, with the frames on the HOST -- the
// caller uploads them (hipMalloc + hipMemcpy, as Frame's constructor does, src/Frame.cpp:68-70,107-149).
struct ProblemDump {
    int n_frames = 0, H = 0, W = 0;
    float image_downscale = 4.0f;
    float K[9] = {};                                  // row-major
    std::vector<EntryJ> corr;                         // pair-major
    std::vector<int> n_match_per_pair;                // P = n (n - 1) / 2 segment lengths
    std::vector<float> poses_init;                    // n x 16, row-major, camera -> model
    std::vector<double> poses_gt;                     // n x 16 or empty
    std::vector<float> depth;                         // n x H x W
    std::vector<float> normals;                       // n x H x W x 4
};
ProblemDump loadProblem(const std::string &path);                    // throws btba::Error(BTBA_EINVAL) on a malformed file
void saveProblem(const std::string &path, const ProblemDump &pb);

}  // namespace btba
