"""Window assembly on the MI355X (btba_window_layout, btba_marshal_windows, btba_procrustes_pairs; include/btba.h).

The two steps between correspondence.find_corres_chain and BatchSolver.solve_zn that bundler.marshal_window and
bundler.procrustes_by_correspondence do on the host: the btba_match records a chain leaves on the device become the solver's
pair-major EntryJ array (Bundler::optimizeGPU, src/Bundler.cpp:286-347) and every new frame's initial pose
(SiftManager::procrustesByCorrespondence, src/FeatureManager.cpp:523-557) without a download, a numpy pass and an upload.
tests/window_ref.py is the plain-numpy form of the rules."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from ._lib import check, lib


@dataclass
class WindowLayout:
    corr_stride: int                # the largest window total, in entries
    max_corr_per_pair: int
    pair_offsets: np.ndarray        # uint32 [n_windows, P + 1]
    n_edges_newframe: np.ndarray    # int64 [n_windows]
    run_ba: np.ndarray              # bool [n_windows]: n_edges_newframe > min_fm_edges_newframe


def window_layout(seg_counts, n_frames: int, newframe_index, min_fm_edges_newframe: int = 5) -> WindowLayout:
    """btba_window_layout (host-only).  seg_counts: int [n_windows, P] matches per canonical pair (0,1) (0,2) .. (N-2,N-1);
    newframe_index: one index per window (or one int for all)."""
    n_frames = int(n_frames)
    P = max(n_frames * (n_frames - 1) // 2, 0)
    cnt = np.ascontiguousarray(np.asarray(seg_counts, np.int32).reshape(-1, P) if P else np.zeros((1, 0), np.int32))
    nw = cnt.shape[0]
    nf = np.ascontiguousarray(np.broadcast_to(np.asarray(newframe_index, np.int32).reshape(-1), (nw,)))
    stride, longest = C.c_int64(0), C.c_uint32(0)
    off = np.zeros((nw, P + 1), np.uint32)
    edges = np.zeros(nw, np.int64)
    run = np.zeros(nw, np.int32)
    check(lib().btba_window_layout(nw, n_frames, cnt.ctypes.data, nf.ctypes.data, int(min_fm_edges_newframe), C.byref(stride), C.byref(longest),
                                   off.ctypes.data, edges.ctypes.data, run.ctypes.data), "btba_window_layout")
    return WindowLayout(int(stride.value), int(longest.value), off, edges, run.astype(bool))


def marshal_windows(ws, matches_dev, segments, n_frames: int, layout: WindowLayout, *, corr24: bool = False, out=None):
    """btba_marshal_windows.  matches_dev: int32 CUDA tensor [n_records, 10] (btba_match records; ChainResult.matches_dev);
    segments: int [n_windows, P, 2] = (first record, count), host or CUDA; layout: window_layout of the same counts.
    Returns (corr_dev uint8 [n_windows, stride, 32], pair_offsets_dev int32 [n_windows, P + 1], corr24_dev or None), all CUDA and
    zero-initialised where the call writes nothing; `out` = a tuple from an earlier call of the same shapes is reused as is.
    Asynchronous on the workspace stream."""
    import torch
    from .optimizer import _dev_ptr
    n_frames = int(n_frames)
    P = n_frames * (n_frames - 1) // 2
    dev = matches_dev.device
    if torch.is_tensor(segments):
        seg = segments.to(device=dev, dtype=torch.int32).reshape(-1, P, 2).contiguous()
    else:
        seg = torch.from_numpy(np.ascontiguousarray(np.asarray(segments, np.int64).reshape(-1, P, 2).astype(np.int32))).to(dev)
    nw = int(seg.shape[0])
    stride = max(int(layout.corr_stride), 1)
    if out is not None:
        corr, off, c24 = out
    else:
        corr = torch.zeros((nw, stride, 32), dtype=torch.uint8, device=dev)
        off = torch.zeros((nw, P + 1), dtype=torch.int32, device=dev)
        c24 = torch.zeros((-(-(nw * stride) // 64), 3, 64, 2), dtype=torch.float32, device=dev) if corr24 else None
    n_records = int(matches_dev.shape[0]) if matches_dev.numel() else 0
    check(lib().btba_marshal_windows(ws.handle, nw, n_frames, _dev_ptr(matches_dev, "matches_dev") if n_records else None, n_records,
                                     _dev_ptr(seg, "segments"), int(layout.max_corr_per_pair), stride, _dev_ptr(corr, "corr_dev"),
                                     _dev_ptr(off, "pair_offsets_dev"), _dev_ptr(c24, "corr24_dev")), "btba_marshal_windows")
    return corr, off, c24


def procrustes_pairs(ws, matches_dev, segments, posesA, posesB, *, want_moments: bool = False, device_resident: bool = False):
    """btba_procrustes_pairs.  segments: host int [n_pairs, 2] = (first record, count); posesA / posesB: [n_pairs, 4, 4] camera ->
    model of the newer and the older frame (numpy, or float32 CUDA tensors with device_resident).  Returns (pose [n_pairs, 4, 4],
    err [n_pairs], moments float64 [n_pairs, 16] or None): numpy, or CUDA tensors with device_resident."""
    import torch
    from .optimizer import _dev_ptr
    seg = np.ascontiguousarray(np.asarray(segments, np.int64).reshape(-1, 2).astype(np.int32))
    n = seg.shape[0]
    n_records = int(matches_dev.shape[0]) if matches_dev is not None and matches_dev.numel() else 0
    mptr = _dev_ptr(matches_dev, "matches_dev") if n_records else None
    if device_resident:
        dev = posesA.device
        pa, pb = posesA.reshape(n, 16).contiguous(), posesB.reshape(n, 16).contiguous()
        pose = torch.zeros((max(n, 1), 16), dtype=torch.float32, device=dev)
        err = torch.zeros((max(n, 1),), dtype=torch.float32, device=dev)
        mom = torch.zeros((max(n, 1), 16), dtype=torch.float64, device=dev) if want_moments else None
        check(lib().btba_procrustes_pairs(ws.handle, 1, n, mptr, n_records, seg.ctypes.data, _dev_ptr(pa, "posesA"), _dev_ptr(pb, "posesB"),
                                          pose.data_ptr(), err.data_ptr(), mom.data_ptr() if mom is not None else None), "btba_procrustes_pairs")
        return pose[:n].reshape(n, 4, 4), err[:n], (mom[:n] if mom is not None else None)
    pa = np.ascontiguousarray(np.asarray(posesA, np.float32).reshape(n, 16))
    pb = np.ascontiguousarray(np.asarray(posesB, np.float32).reshape(n, 16))
    pose = np.zeros((max(n, 1), 16), np.float32)
    err = np.zeros(max(n, 1), np.float32)
    mom = np.zeros((max(n, 1), 16), np.float64) if want_moments else None
    check(lib().btba_procrustes_pairs(ws.handle, 0, n, mptr, n_records, seg.ctypes.data, pa.ctypes.data, pb.ctypes.data, pose.ctypes.data,
                                      err.ctypes.data, mom.ctypes.data if mom is not None else None), "btba_procrustes_pairs")
    return pose[:n].reshape(n, 4, 4), err[:n], (mom[:n] if mom is not None else None)
