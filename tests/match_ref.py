"""Test-side references for btba_match_pairs: the CPU restatement (tests/cpp/match_host.cpp, bit-exact contract) and an
independent fp64 numpy transliteration of the reference's matching (FeatureManager.cpp:247-368).  Frames are plain host
objects here: id, pose (4x4), kpts [n,2], desc [n,D], depth [H,W], normal [H,W,4]."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from dataclasses import dataclass

import numpy as np

from bundletrack_amd._lib import MATCH_DTYPE

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@dataclass
class HostFrame:
    id: int
    pose: np.ndarray
    kpts: np.ndarray
    desc: np.ndarray
    depth: np.ndarray
    normal: np.ndarray


def _build(name: str, srcs: list, extra: list) -> str:
    so = os.path.join(HERE, "cpp", name)
    deps = srcs + [os.path.join(ROOT, "include", "btba.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-march=native", "-pthread", "-fPIC", "-shared", "-fvisibility=hidden",
                               "-o", so] + srcs + extra)
    return so


_host = None


def host_lib():
    """tests/cpp/libmatch_host.so (built on first use with g++ -O2 -ffp-contract=off)."""
    global _host
    if _host is None:
        _host = C.CDLL(_build("libmatch_host.so", [os.path.join(HERE, "cpp", "match_host.cpp")], []))
        _host.match_host.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_int]
    return _host


def restate(frames, pairs, prm, K, H, W):
    """match_host: (per-pair MATCH_DTYPE arrays, ptsA [T,4], ptsB [T,4], n_out)."""
    n = len(frames)
    keep = []                       # keeps the contiguous copies alive during the call

    def arr(vals):
        a = (C.c_void_p * n)()
        for k, v in enumerate(vals):
            v = np.ascontiguousarray(v, np.float32)
            keep.append(v)
            a[k] = v.ctypes.data if v.size else None
        return a

    D = next((f.desc.shape[1] for f in frames if f.desc.size), 4)
    n_kpts = np.array([f.kpts.shape[0] for f in frames], np.int32)
    pr = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))
    cap = int(sum(n_kpts[a] + (n_kpts[b] if prm.mutual else 0) for a, b in pr))
    out = np.zeros(max(cap, 1), MATCH_DTYPE)
    pa, pb = np.zeros((max(cap, 1), 4), np.float32), np.zeros((max(cap, 1), 4), np.float32)
    n_out = np.zeros(max(len(pr), 1), np.int32)
    poses = np.ascontiguousarray(np.stack([np.asarray(f.pose, np.float32).reshape(16) for f in frames]))
    ids = np.array([f.id for f in frames], np.int32)
    Kf = np.ascontiguousarray(np.asarray(K, np.float32).reshape(9))
    host_lib().match_host(C.byref(prm), n, H, W, Kf.ctypes.data, arr([f.desc for f in frames]), D, arr([f.kpts for f in frames]), n_kpts.ctypes.data,
                          arr([f.depth for f in frames]), arr([f.normal for f in frames]), poses.ctypes.data, ids.ctypes.data, len(pr), pr.ctypes.data,
                          out.ctypes.data, pa.ctypes.data, pb.ctypes.data, n_out.ctypes.data, min(16, os.cpu_count() or 1))
    off = np.concatenate([[0], np.cumsum(n_out[: len(pr)])])
    return [out[off[p]:off[p + 1]] for p in range(len(pr))], pa[: off[-1]], pb[: off[-1]], n_out[: len(pr)]


def numpy_fp64(frames, pairs, cfg, K, H, W, k=5, mutual=True, min_z=0.1):
    """The reference's findCorresbyNN restated in float64 numpy (distances, camera points, transforms, gate): per pair a list of
    (idx_a, idx_b, dir) and, per query, the fp64 neighbour list used (for the near-tie accounting)."""
    Kd = np.asarray(K, np.float64)
    out = []
    for a, b in pairs:
        fa, fb = frames[a], frames[b]
        neighbor = abs(fa.id - fb.id) == 1
        md = cfg["max_dist_neighbor" if neighbor else "max_dist_no_neighbor"]
        cm = cfg["cos_neighbor" if neighbor else "cos_no_neighbor"]
        res, lists = [], []
        for d, (fq, ft) in enumerate([(fa, fb), (fb, fa)][: 2 if mutual else 1]):
            if fq.kpts.shape[0] == 0 or ft.kpts.shape[0] == 0:
                continue
            q, t = fq.desc.astype(np.float64), ft.desc.astype(np.float64)
            d2 = (q * q).sum(1)[:, None] + (t * t).sum(1)[None, :] - 2.0 * q @ t.T
            for i in range(q.shape[0]):
                order = np.lexsort((np.arange(t.shape[0]), d2[i]))[:k]
                lists.append((d, i, d2[i][np.lexsort((np.arange(t.shape[0]), d2[i]))[: k + 1]]))
                for j in order:
                    ok, Pq, Nq = _lookup64(fq, fq.kpts[i], Kd, H, W, min_z)
                    ok2, Pt, Nt = _lookup64(ft, ft.kpts[j], Kd, H, W, min_z)
                    if not (ok and ok2):
                        continue
                    if np.linalg.norm(Pq - Pt) > md:
                        continue
                    if _normalized(Nq) @ _normalized(Nt) < cm:
                        continue
                    res.append((i, int(j), 0) if d == 0 else (int(j), i, 1))
                    break
        out.append((res, lists))
    return out


def _normalized(n):
    s = np.linalg.norm(n)
    return n / s if s > 0 else n


def _lookup64(f, kp, Kd, H, W, min_z):
    u, v = np.floor(np.abs(kp.astype(np.float64)) + 0.5) * np.sign(kp)          # round half away from zero
    if not (0 <= u < W and 0 <= v < H):
        return False, None, None
    x, y = int(u), int(v)
    z = float(f.depth[y, x])
    if z < 0.1:
        return False, None, None
    p = np.array([(x - Kd[0, 2]) * z / Kd[0, 0], (y - Kd[1, 2]) * z / Kd[1, 1], z])
    if p[2] < min_z:
        return False, None, None
    T = np.asarray(f.pose, np.float64)
    return True, T[:3, :3] @ p + T[:3, 3], T[:3, :3] @ f.normal[y, x, :3].astype(np.float64)


def scene_frames(pb, kp, pose_key="gt"):
    """HostFrames of a synthetic.make_problem scene with synthetic.make_keypoints keypoints."""
    poses = pb.poses_gt if pose_key == "gt" else pb.poses_init
    return [HostFrame(k, np.asarray(poses[k], np.float32), kp.kpts[k], kp.desc[k], pb.depth[k], pb.normals[k]) for k in range(len(kp.kpts))]
