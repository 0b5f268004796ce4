"""Keyframe fusion and voxel-grid downsampling on the MI355X (btba_fuse_frames, btba_voxel_downsample): posed keyframes -> one cloud.

What a session ends with -- Bundler.keyframes, each with depth_gpu / normal_gpu / color_gpu and a bundle-adjusted pose_in_model --
becomes one voxel-grid cloud per object; the same kernels are Utils::downsamplePointCloud (src/Utils.cpp:134-140, pcl::VoxelGrid) for
any cloud.  Every voxel sum is an integer, so the output bytes do not depend on execution order, batch position or segment order.
The exact rules are in include/btba.h ("keyframe fusion"); the voxel rule is restated from PCL's public header and unverified
against a PCL run."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from ._lib import FUSE_FRAME, FUSE_OVERFLOW, FUSE_POINTS, FuseSegment, check, fuse_params, lib


@dataclass
class Segment:
    """One input of fuse_frames: a posed frame (depth [H,W] float32, normal [H,W,4] float32, colour [H,W,4] uint8 (B, G, R, 0)) or, with
    xyz set, a point list (xyz [n,4] float32, normal [n,4] or None, colour [n,4] or None).  pose: [4,4] camera -> model."""
    instance: int
    pose: object
    depth: object = None
    normal: object = None
    colour: object = None
    xyz: object = None


def frame_segment(frame, instance=0) -> Segment:
    """A FrameRef-like object (depth_gpu, normal_gpu, color_gpu, pose_in_model) as a frame segment."""
    return Segment(instance, frame.pose_in_model, depth=frame.depth_gpu, normal=frame.normal_gpu, colour=getattr(frame, "color_gpu", None))


@dataclass
class ObjectCloud:
    """The clouds of one call: CUDA tensors padded to `capacity` records per instance.  n_out may exceed capacity (status then has
    FUSE_OVERFLOW set); everything is asynchronous on the workspace stream until instance() / counts() read n_out back."""
    xyz: object            # float32 [B, capacity, 4], w = 1
    normal: object         # float32 [B, capacity, 4], w = 0, or None
    colour: object         # uint8 [B, capacity, 4], or None
    count: object          # int32 [B, capacity] (the uint32 point counts)
    lin: object            # int32 [B, capacity]: ix + dims_x (iy + dims_y iz)
    n_out: object          # int32 [B]
    n_outside: object      # int32 [B]
    status: object         # int32 [B]
    box: np.ndarray        # int32 [B, 6] (min_b, dims), host
    leaf: float

    def counts(self) -> np.ndarray:
        """n_out on the host (synchronises)."""
        return self.n_out.cpu().numpy()

    def instance(self, b: int) -> dict:
        """Instance b's records as CUDA views trimmed to n_out[b] (synchronises); ValueError when the capacity was too small."""
        n, st = int(self.n_out[b].item()), int(self.status[b].item())
        if st & FUSE_OVERFLOW:
            raise ValueError(f"instance {b}: {n} voxels exceed the capacity {self.xyz.shape[1]}")
        return {k: getattr(self, k)[b, :n] for k in ("xyz", "normal", "colour", "count", "lin") if getattr(self, k) is not None}


def _segment_array(segments, n_instances):
    """(ctypes array, H, W, has_frames, points per instance, keep-alive list) of Segment objects, with the Python layer's own checks."""
    import torch
    from .optimizer import _dev_ptr
    arr = (FuseSegment * max(len(segments), 1))()
    H = W = 0
    pts = [0] * n_instances
    keep = []
    for k, s in enumerate(segments):
        if not 0 <= int(s.instance) < n_instances:
            raise ValueError(f"segment {k}: instance {s.instance} outside 0 .. {n_instances - 1}")
        g = arr[k]
        g.instance = int(s.instance)
        pose = np.ascontiguousarray(s.pose, np.float32).reshape(16)
        for q in range(16):
            g.pose[q] = pose[q]
        frame = s.xyz is None
        geom = s.depth if frame else s.xyz
        if geom is None or geom.dtype != torch.float32:
            raise ValueError(f"segment {k}: needs a float32 depth map or point list")
        if frame:
            h, w = (int(v) for v in geom.shape[:2])
            if geom.dim() != 2 or (H and (h, w) != (H, W)):
                raise ValueError(f"segment {k}: every depth map must be [H, W] of one size")
            H, W, n = h, w, h * w
            g.kind = FUSE_FRAME
        else:
            if geom.dim() != 2 or geom.shape[1] != 4:
                raise ValueError(f"segment {k}: a point list is [n, 4] float32")
            n = int(geom.shape[0])
            g.kind, g.n = FUSE_POINTS, n
        for name, t, dt in (("normal", s.normal, torch.float32), ("colour", s.colour, torch.uint8)):
            if t is not None and (t.dtype != dt or t.numel() != 4 * n):
                raise ValueError(f"segment {k}: {name} must be {dt} with 4 values per element of the segment")
        g.geom = _dev_ptr(geom, f"segment {k} geometry") if n else None
        g.normal = _dev_ptr(s.normal, f"segment {k} normal") if n else None
        g.colour = _dev_ptr(s.colour, f"segment {k} colour") if n else None
        pts[g.instance] += n
        keep += [geom, s.normal, s.colour]
    return arr, H, W, pts, keep


def _K(K, has_frames):
    if K is None:
        if has_frames:
            raise ValueError("frame segments need the intrinsics K")
        return None, None
    Kf = np.ascontiguousarray(K, np.float32).reshape(9)
    return Kf, Kf.ctypes.data


def fuse_layout(box):
    """btba_fuse_layout (host only): box int32 [B, 6] -> (voxel_offsets int64 [B + 1], scratch bytes); BtbaError (BTBA_EINVAL) for a negative
    side or more than FUSE_MAX_VOXELS voxels."""
    box = np.ascontiguousarray(box, np.int32).reshape(-1, 6)
    off = np.zeros(box.shape[0] + 1, np.int64)
    nbytes = C.c_int64(0)
    check(lib().btba_fuse_layout(box.shape[0], box.ctypes.data, off.ctypes.data, C.byref(nbytes)), "btba_fuse_layout")
    return off, int(nbytes.value)


def fuse_bounds(ws, segments, n_instances, K=None, *, leaf=0.005, require_normals=True):
    """btba_fuse_bounds: VoxelGrid's data-derived box of every instance, a CUDA int32 [n_instances, 6] = (min_b, dims); asynchronous."""
    import torch
    arr, H, W, _, keep = _segment_array(segments, n_instances)
    Kf, Kp = _K(K, H > 0)
    prm = fuse_params(leaf=float(leaf), require_normals=int(bool(require_normals)))
    box = torch.empty((n_instances, 6), dtype=torch.int32, device="cuda")
    check(lib().btba_fuse_bounds(ws.handle, C.byref(prm), n_instances, len(segments), C.cast(arr, C.c_void_p), H, W, Kp, box.data_ptr()), "btba_fuse_bounds")
    return box


def _outputs(n_instances, capacity, want_normals, want_colour):
    import torch
    new = lambda shape, dt: torch.empty(shape, dtype=dt, device="cuda")
    return ObjectCloud(xyz=new((n_instances, capacity, 4), torch.float32), normal=new((n_instances, capacity, 4), torch.float32) if want_normals else None,
                       colour=new((n_instances, capacity, 4), torch.uint8) if want_colour else None, count=new((n_instances, capacity), torch.int32),
                       lin=new((n_instances, capacity), torch.int32), n_out=new((n_instances,), torch.int32), n_outside=new((n_instances,), torch.int32),
                       status=new((n_instances,), torch.int32), box=None, leaf=0.0)


def _capacity(box, pts):
    """What no instance can exceed: its voxels, and its points."""
    vox = np.prod(np.asarray(box, np.int64).reshape(-1, 6)[:, 3:], axis=1)
    return max(1, int(max(min(int(v), int(p)) for v, p in zip(vox, pts))))


def fuse_frames(ws, segments, n_instances=None, K=None, *, leaf=0.005, min_points=1, require_normals=True, normalize_normals=False,
                box=None, capacity=None, want_normals=True, want_colour=None) -> ObjectCloud:
    """btba_fuse_frames on Segment objects (frame_segment(f) for a FrameRef).  box: int32 [n_instances, 6] (min_b, dims) on the host; None
    runs btba_fuse_bounds first and reads its six ints per instance back -- the ONE host synchronisation of this path; with a box given the
    call is asynchronous on the workspace stream.  capacity: records per instance (None: min(voxels, points) of the largest instance, which
    none can exceed).  want_colour None: colour is fused when every segment brings a colour map."""
    segments = list(segments)
    if n_instances is None:
        n_instances = 1 + max((int(s.instance) for s in segments), default=0)
    arr, H, W, pts, keep = _segment_array(segments, n_instances)
    Kf, Kp = _K(K, H > 0)
    if want_colour is None:
        want_colour = bool(segments) and all(s.colour is not None for s in segments)
    prm = fuse_params(leaf=float(leaf), min_points=int(min_points), require_normals=int(bool(require_normals)), normalize_normals=int(bool(normalize_normals)))
    if box is None:
        box = fuse_bounds(ws, segments, n_instances, K, leaf=leaf, require_normals=require_normals).cpu().numpy()      # synchronises
    box = np.ascontiguousarray(box, np.int32).reshape(n_instances, 6)
    if capacity is None:
        capacity = _capacity(box, pts)
    out = _outputs(n_instances, int(capacity), want_normals, want_colour)
    out.box, out.leaf = box, float(leaf)
    p = lambda t: None if t is None else t.data_ptr()
    check(lib().btba_fuse_frames(ws.handle, C.byref(prm), n_instances, len(segments), C.cast(arr, C.c_void_p), H, W, Kp, box.ctypes.data, int(capacity),
                                 p(out.xyz), p(out.normal), p(out.colour), p(out.count), p(out.lin), p(out.n_out), p(out.n_outside), p(out.status)),
          "btba_fuse_frames")
    return out


def voxel_downsample(ws, xyz, normal=None, colour=None, *, leaf=0.015, min_points=1, normalize_normals=False, box=None, capacity=None) -> ObjectCloud:
    """btba_voxel_downsample (Utils::downsamplePointCloud): xyz a CUDA float32 [n, 4] cloud, or a list of them, one per instance; normal /
    colour alike or None.  box None: the data-derived box, as pcl::VoxelGrid takes it (one host synchronisation, see fuse_frames)."""
    import torch
    from .optimizer import _dev_ptr
    single = torch.is_tensor(xyz)
    xyz = [xyz] if single else list(xyz)
    B = len(xyz)
    normal = [normal] * B if (normal is None or single) else list(normal)
    colour = [colour] * B if (colour is None or single) else list(colour)
    segs = [Segment(b, np.eye(4, dtype=np.float32), xyz=xyz[b], normal=normal[b], colour=colour[b]) for b in range(B)]
    _segment_array(segs, B)                                  # the Python layer's checks
    if box is None:
        box = fuse_bounds(ws, segs, B, leaf=leaf).cpu().numpy()
    box = np.ascontiguousarray(box, np.int32).reshape(B, 6)
    n_pts = np.array([int(x.shape[0]) for x in xyz], np.int64)
    if capacity is None:
        capacity = _capacity(box, n_pts)
    want_normals, want_colour = any(n is not None for n in normal), all(c is not None for c in colour)
    out = _outputs(B, int(capacity), want_normals, want_colour)
    out.box, out.leaf = box, float(leaf)
    prm = fuse_params(leaf=float(leaf), min_points=int(min_points), normalize_normals=int(bool(normalize_normals)))

    def table(ts, what):
        arr = (C.c_void_p * B)()
        for b, t in enumerate(ts):
            arr[b] = _dev_ptr(t, f"instance {b} {what}") if t is not None and t.numel() else None
        return C.cast(arr, C.c_void_p)

    p = lambda t: None if t is None else t.data_ptr()
    check(lib().btba_voxel_downsample(ws.handle, C.byref(prm), B, table(xyz, "xyz"), table(normal, "normal") if want_normals else None,
                                      table(colour, "colour") if want_colour else None, n_pts.ctypes.data, box.ctypes.data, int(capacity),
                                      p(out.xyz), p(out.normal), p(out.colour), p(out.count), p(out.lin), p(out.n_out), p(out.n_outside), p(out.status)),
          "btba_voxel_downsample")
    return out
