"""Descriptor matching with the tracker's geometric gate on the MI355X (btba_match_pairs) and the caller logic around it.

Mirrors SiftManager::findCorresbyNNMultiPair (src/FeatureManager.cpp:370-437): for every frame pair the k = 5 nearest
descriptors in both directions, the first neighbour that passes the pixel / depth / distance / normal gate (pruneMatches,
:290-339), A -> B matches then B -> A matches (collectMutualMatches, :341-368).  The reference runs OpenCV's CUDA
brute-force matcher, which has no ROCm build; here one call matches every pair of a tracker step or of a batch of windows.
The output feeds `ransac.run_ransac_multi_pair` (host dict) or `ransac.ransac_packed_device` (model-frame points that never
leave the device)."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

import numpy as np

from ._lib import MATCH_DTYPE, check, lib, match_params

_MATCH_WORDS = MATCH_DTYPE.itemsize // 4


def params_from_config(cfg: dict | None = None, **overrides):
    """btba_match_params from a config_ycbineoat.yml-shaped dict (feature_corres.mutual, max_dist_neighbor, max_normal_neighbor
    (degrees), max_dist_no_neighbor, max_normal_no_neighbor); missing keys keep the shipping values."""
    p = match_params(**overrides)
    fc = (cfg or {}).get("feature_corres", {})
    if "mutual" in fc:
        p.mutual = int(bool(fc["mutual"]))
    for key in ("neighbor", "no_neighbor"):
        if f"max_dist_{key}" in fc:
            setattr(p, f"max_dist_{key}", float(fc[f"max_dist_{key}"]))
        if f"max_normal_{key}" in fc:            # std::cos(float / 180.0 * M_PI) in double, stored as float (FeatureManager.cpp:252-255)
            setattr(p, f"cos_max_normal_{key}", float(np.float32(math.cos(float(np.float32(fc[f"max_normal_{key}"])) / 180.0 * math.pi))))
    return p


@dataclass
class MatchResult:
    per_pair: list                  # one MATCH_DTYPE array per pair (host copies)
    n_out: np.ndarray               # int32 [n_pairs]
    offsets: np.ndarray             # int64 [n_pairs + 1]: pair p owns records offsets[p] .. offsets[p + 1] - 1
    matches_dev: object = None      # device_resident: int32 CUDA tensor [capacity, 10] (the btba_match records)
    ptsA_dev: object = None         # device_resident: float32 CUDA tensors [capacity, 4], model-frame (x, y, z, 1)
    ptsB_dev: object = None
    ptsA: np.ndarray | None = None  # host form: float32 [total, 4]
    ptsB: np.ndarray | None = None


def _dims(frames):
    D = None
    for f in frames:
        if f.desc_gpu is not None and f.desc_gpu.shape[0] > 0:
            if D is not None and f.desc_gpu.shape[1] != D:
                raise ValueError("all frames' descriptors must have the same dimension")
            D = int(f.desc_gpu.shape[1])
    return D if D is not None else 4


def _frame_tables(frames, pairs, K):
    """The per-frame host tables btba_match_pairs and btba_corres_chain take: (n_kpts int32 [n], pairs int32 [P, 2], the desc /
    kpts / depth / normal pointer arrays (an empty or missing tensor = NULL), poses float32 [n, 16], ids int32 [n], K float32 [9])."""
    from .optimizer import _dev_ptr
    n_kpts = np.array([0 if f.kpts_gpu is None else int(f.kpts_gpu.shape[0]) for f in frames], np.int32)
    pr = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))

    def ptrs(attr):
        arr = (C.c_void_p * max(len(frames), 1))()
        for k, f in enumerate(frames):
            t = getattr(f, attr)
            arr[k] = _dev_ptr(t, f"frame {k} {attr}") if (t is not None and t.numel() > 0) else None
        return arr

    poses = np.ascontiguousarray(np.stack([np.asarray(f.pose_in_model, np.float32).reshape(16) for f in frames]), np.float32)
    ids = np.array([int(f.id) for f in frames], np.int32)
    Kf = np.ascontiguousarray(np.asarray(K, np.float32).reshape(9))
    return n_kpts, pr, tuple(ptrs(a) for a in ("desc_gpu", "kpts_gpu", "depth_gpu", "normal_gpu")), poses, ids, Kf


def match_pairs(ws, frames, pairs, params=None, *, K, H: int, W: int, device_resident: bool = True, want_points: bool = True) -> MatchResult:
    """btba_match_pairs.  frames: FrameRef-like objects with id, pose_in_model [4,4], kpts_gpu [n,2], desc_gpu [n,D] (float32 CUDA;
    None or empty = no keypoints), depth_gpu [H,W] and normal_gpu [H,W,4] (btba_depth_to_normals' format).  pairs: [(ia, ib)]
    indices into frames, A first.  K: [3,3] full-resolution intrinsics.  device_resident: the records and model-frame points stay
    on the device (and are copied to the host once for per_pair); otherwise the call writes host buffers."""
    import torch
    from .optimizer import _dev_ptr
    prm = params if params is not None else match_params()
    n = len(frames)
    D = _dims(frames)
    n_kpts, pr, (desc, kpts, depth, normal), poses, ids, Kf = _frame_tables(frames, pairs, K)
    cap = C.c_int64(0)
    check(lib().btba_match_capacity(C.byref(prm), n, int(H), int(W), D, n_kpts.ctypes.data, pr.shape[0], pr.ctypes.data, C.byref(cap)),
          "btba_match_capacity")
    cap = int(cap.value)
    n_out = np.zeros(max(pr.shape[0], 1), np.int32)
    res = MatchResult(per_pair=[], n_out=n_out[: pr.shape[0]], offsets=np.zeros(pr.shape[0] + 1, np.int64))
    if device_resident:
        dev = next((f.depth_gpu.device for f in frames if f.depth_gpu is not None), torch.device("cuda"))
        res.matches_dev = torch.zeros((max(cap, 1), _MATCH_WORDS), dtype=torch.int32, device=dev)
        if want_points:
            res.ptsA_dev = torch.zeros((max(cap, 1), 4), dtype=torch.float32, device=dev)
            res.ptsB_dev = torch.zeros((max(cap, 1), 4), dtype=torch.float32, device=dev)
        out_p, pa_p, pb_p = res.matches_dev.data_ptr(), _dev_ptr(res.ptsA_dev), _dev_ptr(res.ptsB_dev)
    else:
        host = np.zeros(max(cap, 1), MATCH_DTYPE)
        if want_points:
            res.ptsA, res.ptsB = np.zeros((max(cap, 1), 4), np.float32), np.zeros((max(cap, 1), 4), np.float32)
        out_p = host.ctypes.data
        pa_p = res.ptsA.ctypes.data if want_points else None
        pb_p = res.ptsB.ctypes.data if want_points else None
    check(lib().btba_match_pairs(ws.handle, C.byref(prm), int(bool(device_resident)), n, int(H), int(W), Kf.ctypes.data, C.cast(desc, C.c_void_p), D,
                                 C.cast(kpts, C.c_void_p), n_kpts.ctypes.data, C.cast(depth, C.c_void_p), C.cast(normal, C.c_void_p),
                                 poses.ctypes.data, ids.ctypes.data, pr.shape[0], pr.ctypes.data, out_p, pa_p, pb_p, n_out.ctypes.data),
          "btba_match_pairs")
    res.offsets[1:] = np.cumsum(res.n_out)
    total = int(res.offsets[-1])
    if device_resident:
        host = res.matches_dev[:total].cpu().numpy().view(MATCH_DTYPE).reshape(-1) if total else np.zeros(0, MATCH_DTYPE)
    else:
        host = host[:total]
        if want_points:
            res.ptsA, res.ptsB = res.ptsA[:total], res.ptsB[:total]
    res.per_pair = [host[res.offsets[p]:res.offsets[p + 1]].copy() for p in range(pr.shape[0])]
    return res


def find_corres_by_nn_multi_pair(ws, pairs, matches: dict, cfg: dict | None = None, *, K, H: int, W: int) -> MatchResult:
    """SiftManager::findCorresbyNNMultiPair (FeatureManager.cpp:370-437).  pairs: [(frameA, frameB)] FrameRefs, A newer; every
    pair's matches are APPENDED to matches[(A.id, B.id)] = (ptA_cam [n,3], ptB_cam [n,3]) -- the dict run_ransac_multi_pair
    consumes.  cfg: config_ycbineoat.yml-shaped dict (feature_corres.*) or None for the shipping values."""
    frames, index = [], {}
    for fa, fb in pairs:
        for f in (fa, fb):
            if id(f) not in index:
                index[id(f)] = len(frames)
                frames.append(f)
    idx = [(index[id(fa)], index[id(fb)]) for fa, fb in pairs]
    res = match_pairs(ws, frames, idx, params_from_config(cfg), K=K, H=H, W=W, device_resident=True, want_points=False)
    for (fa, fb), m in zip(pairs, res.per_pair):
        key = (fa.id, fb.id)
        old_a, old_b = matches.get(key, (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32)))
        matches[key] = (np.concatenate([np.asarray(old_a, np.float32).reshape(-1, 3), m["ptA_cam"]]),
                        np.concatenate([np.asarray(old_b, np.float32).reshape(-1, 3), m["ptB_cam"]]))
    return res
