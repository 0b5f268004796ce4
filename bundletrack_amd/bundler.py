"""Host-side caller logic either side of the optimiser boundary (A0 and 8(f) rank 2).

Restates, in numpy, the parts of src/Bundler.cpp a drop-in user needs around the hot path:
  * `marshal_window`            Bundler::optimizeGPU's marshalling      (Bundler.cpp:286-347)
  * `check_and_add_keyframe`    Bundler::checkAndAddKeyframe            (Bundler.cpp:185-219)
  * `select_keyframes_for_ba`   Bundler::selectKeyFramesForBA           (Bundler.cpp:222-274)
  * `rotation_geodesic_distance` Utils::rotationGeodesicDistance        (Utils.cpp:42-47)
Feature detection, matching and RANSAC (FeatureManager.*) stay out of scope: `matches` arrive
as arrays of 3-D point pairs, which is exactly what `Correspondence._ptA_cam/_ptB_cam` carry.
"""
from __future__ import annotations

import ctypes
import ctypes.util
from dataclasses import dataclass, field

import numpy as np

from ._lib import ENTRYJ_DTYPE

# std::acos(float) of the reference is the C library's acosf; numpy's float32 arccos is its own vector routine and differs from it in the
# last bit for about one argument in five -- enough to flip a greedy choice between near-equal candidates
_acosf = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6").acosf
_acosf.argtypes, _acosf.restype = [ctypes.c_float], ctypes.c_float


def rotation_geodesic_distance(R1: np.ndarray, R2: np.ndarray) -> float:
    """acos(clamp((tr(R1 R2^T) - 1) / 2)) in fp32 like the Eigen::Matrix3f original (Utils.cpp:42-47): diagonal entry i of
    R1 R2^T is the dot product of the two i-th rows, each summed left to right in float and then the three of them (no BLAS
    call whose summation order or FMA use depends on the host; oracle/btba_oracle_keyframes.c sums the same way)."""
    R1 = np.asarray(R1, np.float32)
    R2 = np.asarray(R2, np.float32)
    prod = R1 * R2                                            # float32 products, each rounded once
    dots = (prod[:, 0] + prod[:, 1]) + prod[:, 2]
    trace = (dots[0] + dots[1]) + dots[2]
    tmp = np.float32((trace - np.float32(1.0)) / 2.0)
    tmp = max(min(np.float32(1.0), tmp), np.float32(-1.0))
    return float(_acosf(float(tmp)))


@dataclass
class FrameRef:
    """The fields of `Frame` (src/Frame.h:45-96) the BA caller touches."""
    id: int
    pose_in_model: np.ndarray            # [4,4] camera -> model
    status: str = "OTHER"                # Frame::Status {FAIL, NO_BA, OTHER}, Frame.h:48-53
    n_keypts: int = 0
    roi: tuple = (0.0, 1e9, 0.0, 1e9)    # (umin, umax, vmin, vmax) of the segmentation mask, Frame.h:81
    depth_gpu: object = None
    normal_gpu: object = None
    color_gpu: object = None
    kpts_gpu: object = None              # [n, 2] float32 CUDA tensor: keypoints (x, y) in full-resolution pixels (Frame::_keypts)
    desc_gpu: object = None              # [n, D] float32 CUDA tensor: their descriptors (Frame::_feat_des_gpu)
    mask_gpu: object = None              # [H, W] uint8 CUDA tensor: the raw object mask, nonzero = foreground (the mask PNG)
    fg_mask_gpu: object = None           # [H, W] uint8 CUDA tensor: the final 0 / 1 mask segmentation made of it (Frame::_fg_mask)
    depth_code_gpu: object = None        # [H, W] uint16 / int16 CUDA tensor: the depth PNG's millimetre codes; ingest makes depth_gpu, normal_gpu of it
    bgr_gpu: object = None               # [H, W, 3] uint8 CUDA tensor: the colour image as imread gives it; ingest makes color_gpu of it

    def __hash__(self):
        return hash(self.id)


@dataclass
class KeyframeMemory:
    """The "memory" of the memory-augmented pose graph: the keyframe pool and the BA subset."""
    min_rot_deg: float = 10.0            # keyframe.min_rot      (config_ycbineoat.yml:36)
    min_feat_num: int = 0                # keyframe.min_feat_num (:35)
    max_BA_frames: int = 15              # bundle.max_BA_frames  (:27)
    keyframes: list = field(default_factory=list)

    def check_and_add_keyframe(self, frame: FrameRef) -> bool:
        """Bundler.cpp:185-219: frame 0 always; otherwise only status OTHER, enough keypoints, and a
        rotation >= min_rot degrees away from EVERY existing keyframe."""
        if frame.id == 0:
            self.keyframes.append(frame)
            return True
        if frame.status != "OTHER":
            return False
        if frame.n_keypts < self.min_feat_num:
            return False
        for kf in self.keyframes:
            rot_diff = rotation_geodesic_distance(frame.pose_in_model[:3, :3], kf.pose_in_model[:3, :3])
            rot_diff = np.float32(np.float64(np.float32(rot_diff) * np.float32(180.0)) / np.pi)     # product in float, division in double (:208)
            if rot_diff < self.min_rot_deg:
                return False
        self.keyframes.append(frame)
        return True

    def select_keyframes_for_ba(self, newframe: FrameRef) -> list:
        """Bundler.cpp:222-274 ("greedy_rot"): the new frame plus, if the pool does not fit, keyframe 0
        and then repeatedly the keyframe with the SMALLEST summed geodesic rotation distance to the
        already chosen set.  (The reference keeps the chosen set in a std::set of shared_ptr, i.e. in
        pointer order; the result is sorted by frame id afterwards -- Bundler.cpp:286 -- so only the
        summation order of cum_dist depends on it; here the set is iterated in frame-id order: what an
        allocator that hands out ascending addresses gives the reference.)"""
        chosen = [newframe]
        if len(self.keyframes) + len(chosen) <= self.max_BA_frames:
            for kf in self.keyframes:
                if kf not in chosen:
                    chosen.append(kf)
            return sorted(chosen, key=lambda f: f.id)
        if self.keyframes[0] not in chosen:
            chosen.append(self.keyframes[0])
        while len(chosen) < self.max_BA_frames:
            best, best_kf = np.finfo(np.float32).max, None
            for kf in self.keyframes:
                if kf in chosen:
                    continue
                cum = np.float32(0)
                for f in sorted(chosen, key=lambda f: f.id):
                    cum = np.float32(cum + np.float32(rotation_geodesic_distance(kf.pose_in_model[:3, :3], f.pose_in_model[:3, :3])))
                if cum < best:
                    best, best_kf = cum, kf
            if best_kf is None:
                break
            chosen.append(best_kf)
        return sorted(chosen, key=lambda f: f.id)


@dataclass
class Window:
    """What optimizeGPU hands to OptimizerGpu::optimizeFrames."""
    frames: list
    corr: np.ndarray                  # ENTRYJ_DTYPE, pair-major
    n_match_per_pair: np.ndarray
    n_edges_newframe: int
    run_ba: bool                      # False <=> Frame::NO_BA (Bundler.cpp:343-347)


def marshal_window(local_frames, matches, newframe, min_fm_edges_newframe: int = 5) -> Window:
    """Bundler::optimizeGPU up to the optimiser call (Bundler.cpp:286-347).

    local_frames: FrameRef list (any order; sorted by id here like :286, so index 0 = oldest = fixed).
    matches: dict {(id_A, id_B): (ptA_cam [m,3], ptB_cam [m,3])} keyed by (later frame id, earlier
    frame id) like `_fm->_matches[{frameA, frameB}]` with frameA = local_frames[j], frameB =
    local_frames[i], i<j.  EntryJ{imgIdx_i=i, imgIdx_j=j, pos_i=ptB_cam, pos_j=ptA_cam} (:311-316)."""
    frames = sorted(local_frames, key=lambda f: f.id)
    blocks, counts, n_edges = [], [], 0
    for i in range(len(frames)):
        for j in range(i + 1, len(frames)):
            fa, fb = frames[j], frames[i]
            ptA, ptB = matches.get((fa.id, fb.id), (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32)))
            m = len(ptA)
            blk = np.zeros(m, ENTRYJ_DTYPE)
            blk["imgIdx_i"], blk["imgIdx_j"] = i, j
            blk["pos_i"], blk["pos_j"] = np.asarray(ptB, np.float32).reshape(m, 3), np.asarray(ptA, np.float32).reshape(m, 3)
            blocks.append(blk)
            counts.append(m)
            if fa.id == newframe.id or fb.id == newframe.id:
                n_edges += m
    corr = np.concatenate(blocks) if blocks else np.zeros(0, ENTRYJ_DTYPE)
    run = n_edges > min_fm_edges_newframe
    if not run:
        newframe.status = "NO_BA"
    return Window(frames=frames, corr=corr, n_match_per_pair=np.asarray(counts, np.int32), n_edges_newframe=n_edges, run_ba=run)


class DeviceWindow:
    """A Window assembled on the device (window.marshal_windows): the same fields, with `corr` downloaded on first use."""

    def __init__(self, frames, n_match_per_pair, n_edges_newframe, run_ba, layout, corr_dev=None, pair_offsets_dev=None):
        self.frames, self.n_match_per_pair = frames, n_match_per_pair
        self.n_edges_newframe, self.run_ba, self.layout = n_edges_newframe, run_ba, layout
        self.corr_dev, self.pair_offsets_dev = corr_dev, pair_offsets_dev          # uint8 [1, stride, 32], int32 [1, P + 1] CUDA
        self._corr = None

    @property
    def corr(self) -> np.ndarray:
        if self._corr is None:
            n = int(self.n_match_per_pair.sum())
            self._corr = (self.corr_dev[0, :n].cpu().numpy().view(ENTRYJ_DTYPE).reshape(-1).copy() if n and self.corr_dev is not None
                          else np.zeros(0, ENTRYJ_DTYPE))
        return self._corr


# ---------------------------------------------------------------------------------------------------------
# The rest of Bundler's BA-facing slice: Kabsch initialisation, the per-frame driver, the pose-file format.
# Feature detection / matching / RANSAC (LF-Net, SiftGPU, cuda_ransac) stay behind `feature_manager`.
# ---------------------------------------------------------------------------------------------------------

def solve_rigid_transform_between_points(points1: np.ndarray, points2: np.ndarray) -> np.ndarray:
    """Utils::solveRigidTransformBetweenPoints (src/Utils.cpp:180-214): Kabsch, points1 -> points2, fp32.
    Identity when V U^T is not orthonormal or the result is not finite; a reflection flips V's last column."""
    p1 = np.asarray(points1, np.float32).reshape(-1, 3)
    p2 = np.asarray(points2, np.float32).reshape(-1, 3)
    pose = np.eye(4, dtype=np.float32)
    if p1.shape[0] < 3 or p1.shape != p2.shape:
        return pose
    m1, m2 = p1.mean(0, dtype=np.float32), p2.mean(0, dtype=np.float32)
    S = (p1 - m1).T @ (p2 - m2)
    if not np.isfinite(S).all():            # Eigen's JacobiSVD would return NaNs and the isApprox test below would fail
        return pose
    U, _, Vt = np.linalg.svd(S.astype(np.float32))
    V = Vt.T
    R = V @ U.T
    if not np.allclose(R.T @ R, np.eye(3, dtype=np.float32), rtol=1e-5, atol=1e-5):       # Eigen isApprox, float precision
        return pose
    if np.linalg.det(R) < 0:
        V = V.copy()
        V[:, 2] = -V[:, 2]
        R = V @ U.T
    pose[:3, :3] = R
    pose[:3, 3] = m2 - R @ m1
    if not np.isfinite(pose).all():
        return np.eye(4, dtype=np.float32)
    return pose


def procrustes_by_correspondence(matches: dict, frameA, frameB) -> np.ndarray:
    """FeatureManager::procrustesByCorrespondence of the C++ host layer (src/FeatureManager.cpp:523-556): Kabsch of
    matches[(A.id, B.id)] moved into the model frame with the frames' current poses (fp32, T_r0 x + T_r1 y + T_r2 z + T_r3 in that
    order), identity below 5 matches."""
    ptA, ptB = matches.get((frameA.id, frameB.id), (np.zeros((0, 3), np.float32),) * 2)
    ptA, ptB = np.asarray(ptA, np.float32).reshape(-1, 3), np.asarray(ptB, np.float32).reshape(-1, 3)
    if len(ptA) < 5:
        return np.eye(4, dtype=np.float32)

    def move(p, T):
        T = np.asarray(T, np.float32)
        return np.stack([((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + T[r, 3] for r in range(3)], 1)
    return solve_rigid_transform_between_points(move(ptA, frameA.pose_in_model), move(ptB, frameB.pose_in_model))


def format_pose_txt(ob_in_cam: np.ndarray) -> str:
    """`ff << std::setprecision(10) << ob_in_cam << std::endl` (Bundler.cpp:372-377) with Eigen's default
    IOFormat: coefficients in %.10g, every column padded to the widest coefficient, single-space separator."""
    M = np.asarray(ob_in_cam, np.float32).reshape(4, 4)
    cells = [[format(float(v), ".10g") for v in row] for row in M]
    width = max(len(c) for row in cells for c in row)
    return "\n".join(" ".join(c.rjust(width) for c in row) for row in cells) + "\n"


def save_pose_txt(path: str, pose_in_model: np.ndarray) -> None:
    """saveNewframeResult's pose file: poses/<id_str>.txt holds ob_in_cam = inverse(camera -> model)."""
    ob_in_cam = np.linalg.inv(np.asarray(pose_in_model, np.float32)).astype(np.float32)
    with open(path, "w") as f:
        f.write(format_pose_txt(ob_in_cam))


def load_pose_txt(path: str) -> np.ndarray:
    """What scripts/eval_ycbineoat.py:124-144 does with the file (np.loadtxt -> 4x4)."""
    return np.loadtxt(path).reshape(4, 4)


class Bundler:
    """Bundler::processNewFrame (src/Bundler.cpp:52-183) from the point where a frame has depth, normals and features --
    or, for a frame that carries only `depth_code_gpu` (and `bgr_gpu`), from its images: Bundler.ingest then makes depth_gpu,
    normal_gpu and color_gpu first (ingest.ingest_frames, what Frame's constructor does).  With a `segmenter` (the video
    segmentation's backbone, a callable: the caller's torch model, or btba_vos_features as vos_net.VosBackbone) and a `mask_propagator` (vos.MaskPropagator) a frame with `bgr_gpu` and no `mask_gpu` gets
    its mask from the propagation (Bundler.propagate_mask); off by default.  Then the segmentation by its mask when `mask_gpu` is set (segmentation.apply_masks on `mask_workspace` or the optimiser's
    workspace; the ROI gate then sees the real ROI), feature detection when a `detector` is given (Bundler.detect: the
    detector's input and the keypoints' way back on the GPU, the detector itself a callable; an exception from it marks the
    frame FAIL), pose initialisation from the previous frame, sliding window, keyframe subset, bundle adjustment through an
    injected `optimizer` (anything with OptimizerGpu.optimizeFrames' signature) and keyframe insertion.

    feature_manager must offer (the slice of SiftManager the caller uses):
        find_corres(frameA, frameB)        -> None; fills matches[(frameA.id, frameB.id)] = (ptA_cam, ptB_cam), A newer
        matches                            -> dict as above
        procrustes_by_correspondence(frameA, frameB) -> 4x4 model-frame offset (FeatureManager.cpp:523-556)
        forget_frame(frame)                -> None
    and may offer find_corres_chain([(frameA, frameB), ...]) (correspondence.GpuFeatureManager): optimize_gpu then hands it the
    window's pairs in find_corres order in one call.

    device_window (off by default): with a feature manager that keeps its records on the device (device_segments / device_records /
    procrustes_by_correspondence_device, as GpuFeatureManager does) the initial pose comes from btba_procrustes_pairs and the window
    is assembled by btba_marshal_windows and solved from device memory (BatchSolver.solve_zn on per-frame compact caches kept by
    frame id); the gate, last_window, n_ba_calls and the status handling are the host path's.  A feature manager without device
    records takes the host path silently.
    """

    def __init__(self, optimizer, feature_manager, K, H, W, *, window_size=2, max_BA_frames=15, min_rot_deg=10.0,
                 min_feat_num=0, min_fm_edges_newframe=5, pose_dir=None, persistent_frame_cache=False,
                 mask_largest_component_hull=False, mask_dilate=5, mask_workspace=None, detector=None, detector_out_size=400,
                 device_window=False, segmenter=None, mask_propagator=None, memory=None):
        self.opt, self.fm = optimizer, feature_manager
        if (segmenter is None) != (mask_propagator is None):
            raise ValueError("Bundler: segmenter and mask_propagator go together")
        self.segmenter = segmenter                                               # None (default): frames arrive with mask_gpu set, as before
        self.mask_propagator = mask_propagator                                   # vos.MaskPropagator: the video's propagation state
        self.device_window = bool(device_window)
        self.last_procrustes_err = None                                          # device_window: err of the last initial pose (FeatureManager.cpp:550)
        self._zn_cache: dict = {}                                                # device_window: frame id -> (depth ptr, normal ptr, zn [Hd, Wd, 4])
        self._batch_solver = None
        self.detector = detector                                                 # None: frames arrive with kpts_gpu / desc_gpu set
        self.detector_out_size = int(detector_out_size)                          # Lfnet::detectFeature's H_input = W_input = 400
        self.mask_largest_component_hull = bool(mask_largest_component_hull)     # the reference's `data_dir contains "NOCS"` (Frame.cpp:255,280)
        self.mask_dilate = int(mask_dilate)                                      # MORPH_RECT 5 x 5 (Frame.cpp:310)
        self.mask_workspace = mask_workspace                                     # None: the optimiser's workspace
        self.K, self.H, self.W = np.asarray(K, np.float32), int(H), int(W)
        self.window_size = int(window_size)                        # bundle.window_size (config_ycbineoat.yml:26 ships 2)
        self.min_fm_edges_newframe = int(min_fm_edges_newframe)    # bundle.min_fm_edges_newframe
        # memory: anything with KeyframeMemory's interface (keyframes, check_and_add_keyframe, select_keyframes_for_ba), e.g. keyframes.KeyframeSession,
        # built by the caller with its own gates; None (default): the host memory, as before
        self.memory = memory if memory is not None else KeyframeMemory(min_rot_deg=min_rot_deg, min_feat_num=min_feat_num, max_BA_frames=max_BA_frames)
        self.frames: list = []                                     # _frames (deque)
        self.local_frames: list = []
        self.newframe = None
        self.need_reinit = False
        self.pose_dir = pose_dir
        self.persistent_frame_cache = bool(persistent_frame_cache)     # hand Frame ids to the optimiser as cache keys
        if self.persistent_frame_cache and getattr(optimizer, "workspace", None) is not None:
            from .optimizer import frame_cache_clear
            frame_cache_clear(optimizer.workspace)                     # frame ids restart at 0 with every tracking session
        self.n_ba_calls = 0
        self.last_window = None

    @property
    def keyframes(self):
        return self.memory.keyframes

    def reconstruct(self, leaf=0.005, min_points=1, normalize_normals=False, want_colour=None):
        """The object the session tracked: self.keyframes (their masked depth, normal and colour maps at their bundle-adjusted
        pose_in_model) fused into one voxel-grid cloud on the optimiser's workspace (fusion.fuse_frames; an ObjectCloud of one instance).
        Colour is fused when every keyframe has a colour map (want_colour None).  normalize_normals: unit mean normals, what
        register_to_model needs of its model.  One host synchronisation: the data-derived box."""
        from .fusion import frame_segment, fuse_frames
        ws = getattr(self.opt, "workspace", None)
        if ws is None:
            raise RuntimeError("Bundler.reconstruct needs an optimizer with a workspace")
        return fuse_frames(ws, [frame_segment(kf) for kf in self.keyframes], 1, self.K, leaf=leaf, min_points=min_points,
                           normalize_normals=normalize_normals, want_colour=want_colour)

    def register_to_model(self, frames=None, cloud=None, **params):
        """Point-to-plane registration of frames against the fused object (registration.register_frames): each frame's masked depth and
        normal maps, from its current pose_in_model.  frames: a FrameRef or a list of them (default: the newest frame); cloud: an ObjectCloud
        or a registration.ModelIndex (default: self.reconstruct(normalize_normals=True, want_colour=False)).  Returns the Registration -- refined poses,
        status, fitness, rms -- and changes no state: whether to adopt a pose is the caller's decision.  n_iters=0 is the pose check."""
        from .fusion import frame_segment
        from .registration import register_frames
        ws = getattr(self.opt, "workspace", None)
        if ws is None:
            raise RuntimeError("Bundler.register_to_model needs an optimizer with a workspace")
        if frames is None:
            frames = [self.frames[-1]] if self.frames else []
        elif isinstance(frames, FrameRef):
            frames = [frames]
        if cloud is None:
            cloud = self.reconstruct(normalize_normals=True, want_colour=False)
        segments = [frame_segment(f) for f in frames]
        for s in segments:
            s.colour = None
        return register_frames(ws, cloud, segments, self.K, **params)

    def process_new_frame(self, frame: FrameRef) -> None:
        self.newframe = frame
        last = self.frames[-1] if self.frames else None
        if last is not None:
            frame.id = last.id + 1
            frame.pose_in_model = np.array(last.pose_in_model, np.float32)             # :78-79
        if frame.depth_gpu is None and frame.depth_code_gpu is not None:               # Frame's constructor (Frame.cpp:45-89), minus the imreads
            self.ingest(frame)
        if self.segmenter is not None and frame.bgr_gpu is not None and (frame.mask_gpu is None or self.mask_propagator.n_frames == 0):
            self.propagate_mask(frame)                                                 # run_video.py: the mask file's content, made here
        if frame.mask_gpu is not None:                                                 # :80/:84 segmentationByMaskFile (minus the PNG read)
            self.segment(frame)
        if frame.roi[1] - frame.roi[0] < 10 or frame.roi[3] - frame.roi[2] < 10:        # :88-93: empty cloud -> FAIL and a plain return
            frame.status = "FAIL"
            return
        if frame.status == "FAIL":                                                     # :96-101
            self.fm.forget_frame(frame)
            self.need_reinit = True
            return
        if self.detector is not None:                                                  # :103-117 detectFeature; an exception marks FAIL
            try:
                self.detect(frame)
            except Exception:
                frame.status = "FAIL"
                self.need_reinit = True
                self.fm.forget_frame(frame)
                return
        if last is not None:
            self.fm.find_corres(frame, last)                                           # :122
            if frame.status == "FAIL":
                self.need_reinit = True
                self.fm.forget_frame(frame)
                return
            if self._device_records():
                offset, self.last_procrustes_err = self.fm.procrustes_by_correspondence_device(frame, last)
            else:
                offset = self.fm.procrustes_by_correspondence(frame, last)             # :134-136
            frame.pose_in_model = (np.asarray(offset, np.float32) @ frame.pose_in_model).astype(np.float32)
        if len(self.frames) >= self.window_size + 3:                                   # :150-158
            if self.frames[0] not in self.keyframes:
                self.fm.forget_frame(self.frames[0])
            self.frames.pop(0)
        self.frames.append(frame)
        if frame.id == 0:
            self.memory.check_and_add_keyframe(frame)
            return
        self.local_frames = self.memory.select_keyframes_for_ba(frame)                 # :168
        self.optimize_gpu()                                                            # :169
        if frame.status == "FAIL":
            self.fm.forget_frame(frame)
            self.frames.pop()
            self._evict_cached(frame)                  # its id is handed out again to the next frame (last.id + 1)
            self.need_reinit = True
            return
        self.memory.check_and_add_keyframe(frame)
        if self.pose_dir is not None:
            self.save_newframe_result()

    def ingest(self, frame: FrameRef) -> None:
        """Frame's constructor on the GPU (btba_ingest_frames): frame.depth_gpu, normal_gpu and (with bgr_gpu) color_gpu made of
        frame.depth_code_gpu and frame.bgr_gpu, on the workspace `segment` uses."""
        from .ingest import ingest_frames
        ingest_frames(self._workspace("ingest"), [frame], K=self.K)

    def propagate_mask(self, frame: FrameRef) -> None:
        """run_video.py's loop body around the injected backbone: segmenter(float32 [1, 3, H, W] normalised RGB) -> features
        [C, Hd, Wd] (or [1, C, Hd, Wd]).  A frame that brings its mask while the propagator is empty is the annotated first frame
        (MaskPropagator.start); a frame without one gets frame.mask_gpu from MaskPropagator.step."""
        from .vos import normalize_inputs
        feats = self.segmenter(normalize_inputs(self._workspace("propagate_mask"), [frame.bgr_gpu]))
        if feats.dim() == 4:
            feats = feats[0]
        if frame.mask_gpu is not None:
            self.mask_propagator.start(frame.mask_gpu, feats)
        else:
            frame.mask_gpu = self.mask_propagator.step(feats)

    def segment(self, frame: FrameRef) -> None:
        """Frame::segmentationByMaskFile on the GPU (btba_apply_masks): frame.depth_gpu, normal_gpu, color_gpu zeroed outside
        the final mask in place, frame.roi and frame.fg_mask_gpu set."""
        from .segmentation import apply_masks
        ws = self._workspace("segment")
        apply_masks(ws, [frame], [frame.mask_gpu], largest_component_hull=self.mask_largest_component_hull, dilate=self.mask_dilate)

    def detect(self, frame: FrameRef) -> None:
        """Lfnet::detectFeature with rot_deg = 0 around the injected detector: the detector's input made on the GPU
        (detection.prepare_detector_inputs on frame.color_gpu and frame.roi), detector(bgr [1,S,S,3] uint8, gray [1,1,S,S] float32)
        -> (kpts [m,2], desc [m,D]) float32 CUDA tensors in detector pixels, the keypoints mapped back to full-resolution pixels
        (detection.keypoints_to_image).  Sets frame.kpts_gpu, desc_gpu and n_keypts."""
        import torch
        from .detection import keypoints_to_image, prepare_detector_inputs
        ws = self._workspace("detect")
        bgr, gray = prepare_detector_inputs(ws, [frame], out_size=self.detector_out_size)
        kpts, desc = self.detector(bgr, gray)
        kpts = kpts.to(device=bgr.device, dtype=torch.float32).reshape(-1, 2).contiguous()
        desc = desc.to(device=bgr.device, dtype=torch.float32).reshape(kpts.shape[0], -1).contiguous()
        keypoints_to_image(ws, [frame], [kpts], out_size=self.detector_out_size)
        frame.desc_gpu = desc

    def _workspace(self, what: str):
        ws = self.mask_workspace if self.mask_workspace is not None else getattr(self.opt, "workspace", None)
        if ws is None:
            raise RuntimeError(f"Bundler.{what} needs a workspace: pass mask_workspace= or an optimizer with one")
        return ws

    def _evict_cached(self, frame) -> None:
        """A frame dropped after BA has cached it must not leave its (z, n) cache behind under an id the next frame reuses."""
        if self.persistent_frame_cache and getattr(self.opt, "workspace", None) is not None:
            from .optimizer import frame_cache_evict
            frame_cache_evict(self.opt.workspace, frame.id)

    def optimize_gpu(self) -> None:
        """Bundler::optimizeGPU (:279-359): match every pair of the window, marshal, gate, optimise, write back."""
        frames = sorted(self.local_frames, key=lambda f: f.id)
        chain = getattr(self.fm, "find_corres_chain", None)         # a feature manager that runs the window's pairs as one device chain
        if chain is not None:
            chain([(frames[j], frames[i]) for i in range(len(frames)) for j in range(i + 1, len(frames))])
        else:
            for i in range(len(frames)):
                for j in range(i + 1, len(frames)):
                    self.fm.find_corres(frames[j], frames[i])
        if self._device_records():
            self._optimize_from_device(frames)
            return
        win = marshal_window(frames, self.fm.matches, self.newframe, self.min_fm_edges_newframe)
        self.last_window = win
        if not win.run_ba:
            return
        poses = np.stack([np.asarray(f.pose_in_model, np.float32) for f in win.frames])
        extra = {"frame_keys": [f.id for f in win.frames]} if self.persistent_frame_cache else {}
        self.opt.optimizeFrames(win.corr, win.n_match_per_pair, len(win.frames), self.H, self.W,
                                [f.depth_gpu for f in win.frames], [f.color_gpu for f in win.frames],
                                [f.normal_gpu for f in win.frames], poses, self.K, **extra)
        self.n_ba_calls += 1
        for f, T in zip(win.frames, poses):
            f.pose_in_model = np.array(T, np.float32)

    def _device_records(self) -> bool:
        return (self.device_window and getattr(self.opt, "workspace", None) is not None and hasattr(self.fm, "device_segments")
                and hasattr(self.fm, "procrustes_by_correspondence_device") and self.fm.device_records() is not None)

    def assemble_window_on_device(self, frames) -> DeviceWindow:
        """marshal_window's result from the feature manager's device records (window.window_layout + window.marshal_windows):
        frames sorted by id.  Marks the new frame NO_BA when the gate fails, like marshal_window."""
        from .window import marshal_windows, window_layout
        n = len(frames)
        segs = [self.fm.device_segments.get((frames[j].id, frames[i].id), (0, 0)) for i in range(n) for j in range(i + 1, n)]
        counts = np.array([c for _, c in segs], np.int32)
        new_index = next(k for k, f in enumerate(frames) if f.id == self.newframe.id)
        lay = window_layout(counts[None], n, new_index, self.min_fm_edges_newframe)
        run = bool(lay.run_ba[0])
        win = DeviceWindow(frames, counts, int(lay.n_edges_newframe[0]), run, lay)
        if not run:
            self.newframe.status = "NO_BA"
        if run or counts.sum():
            win.corr_dev, win.pair_offsets_dev, _ = marshal_windows(self.opt.workspace, self.fm.device_records(), np.asarray(segs, np.int64)[None], n, lay)
        return win

    def _window_caches(self, frames):
        """Compact (z, n) caches of the window's frames [1, N, Hd, Wd, 4], each built once per frame id and pair of maps."""
        import torch
        from .optimizer import build_cache_zn
        ws = self.opt.workspace
        keep = {f.id for f in frames} | {f.id for f in self.frames} | {f.id for f in self.keyframes}
        for fid in [k for k in self._zn_cache if k not in keep]:
            del self._zn_cache[fid]
        for f in frames:
            tag = (f.depth_gpu.data_ptr(), f.normal_gpu.data_ptr())
            if f.id not in self._zn_cache or self._zn_cache[f.id][0] != tag:
                zn, _, _ = build_cache_zn(ws, [f.depth_gpu], [f.normal_gpu], self.H, self.W, self.K, float(self.opt.params.image_downscale))
                self._zn_cache[f.id] = (tag, zn[0])
        return torch.stack([self._zn_cache[f.id][1] for f in frames])[None]

    def _optimize_from_device(self, frames) -> None:
        """optimize_gpu from the marshalling on, on device memory."""
        import ctypes
        import torch
        from ._lib import BTBA_ENUMERIC, BtbaError, Params
        from .optimizer import BatchSolver
        win = self.assemble_window_on_device(frames)
        self.last_window = win
        if not win.run_ba:
            return
        if self._batch_solver is None:
            self._batch_solver = BatchSolver(workspace=self.opt.workspace)
        prm = Params()
        ctypes.memmove(ctypes.byref(prm), ctypes.byref(self.opt.params), ctypes.sizeof(Params))
        self._batch_solver.params = prm
        zn = self._window_caches(frames)
        poses_dev = torch.from_numpy(np.stack([np.asarray(f.pose_in_model, np.float32) for f in frames])[None].copy()).to(zn.device)
        self._batch_solver.solve_zn(zn, self.H, self.W, self.K, win.corr_dev, win.pair_offsets_dev, win.layout.max_corr_per_pair, poses_dev)
        poses = poses_dev[0].cpu().numpy()
        if not np.isfinite(poses).all():
            raise BtbaError(BTBA_ENUMERIC, "btba_solve_batch_zn")
        self.n_ba_calls += 1
        for f, T in zip(frames, poses):
            f.pose_in_model = np.array(T, np.float32)

    def save_newframe_result(self) -> None:
        import os
        os.makedirs(self.pose_dir, exist_ok=True)
        name = getattr(self.newframe, "id_str", None) or "%04d" % self.newframe.id
        save_pose_txt(os.path.join(self.pose_dir, name + ".txt"), self.newframe.pose_in_model)
