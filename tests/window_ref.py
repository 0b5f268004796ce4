"""Independent restatement of the window assembly (include/btba.h, "window assembly"): numpy only, no code shared with the package.

  marshal          btba_match segments -> pair-major EntryJ, pair offsets, the new frame's edge count and the BA gate
  pack24           the 24-byte plane layout btba_pack_correspondences24 documents
  model_points     a_k = TA ptA_cam, b_k = TB ptB_cam in uncontracted fp32
  moments          n, m1, m2, S in fp64 in the fixed order: 256 slots as strided row adds, then the tree (exact in numpy)
  kabsch           the rotation by numpy's fp64 SVD (V U^T, last column of V flipped for det < 0), t = m2 - R m1
  procrustes       one pair: pose (fp64 and rounded once to fp32), err, moments, and the conditioning of S: the second singular
                   value >= 1e-3 of the first, and -- what decides whether the PROPER optimum is unique, the eigenvalue gap of
                   Horn's matrix -- s2 + sign(det S) s3 >= 1e-3 s1 as well (the same thing unless S is close to a reflection)
"""
import numpy as np

ENTRYJ = np.dtype([("imgIdx_i", "<u4"), ("imgIdx_j", "<u4"), ("pos_i", "<f4", (3,)), ("pos_j", "<f4", (3,))])
MATCH = np.dtype([("idx_a", "<i4"), ("idx_b", "<i4"), ("dist", "<f4"), ("dir", "<i4"), ("ptA_cam", "<f4", (3,)), ("ptB_cam", "<f4", (3,))])
SLOTS = 256
MIN_POINTS = 5


def canonical_pairs(n_frames):
    return [(i, j) for i in range(n_frames) for j in range(i + 1, n_frames)]


def marshal(records, segments, n_frames, newframe_index, min_fm_edges_newframe=5):
    """records: MATCH array; segments: [(first record, count)] per canonical pair.  Returns (corr ENTRYJ, offsets uint32 [P + 1],
    n_edges_newframe, run_ba)."""
    pairs = canonical_pairs(n_frames)
    assert len(segments) == len(pairs)
    total = sum(int(c) for _, c in segments)
    corr = np.zeros(total, ENTRYJ)
    offsets = np.zeros(len(pairs) + 1, np.uint32)
    at = edges = 0
    for p, ((i, j), (first, count)) in enumerate(zip(pairs, segments)):
        offsets[p] = at
        for k in range(int(count)):
            r = records[int(first) + k]
            corr[at]["imgIdx_i"], corr[at]["imgIdx_j"] = i, j
            corr[at]["pos_i"] = r["ptB_cam"]
            corr[at]["pos_j"] = r["ptA_cam"]
            at += 1
        if newframe_index in (i, j):
            edges += int(count)
    offsets[len(pairs)] = at
    return corr, offsets, edges, edges > min_fm_edges_newframe


def pack24(corr_blocks, stride):
    """corr_blocks: one ENTRYJ array per window (its written entries); entry E = w * stride + e has its k-th float2 at float2 index
    (E // 64) * 192 + k * 64 + E % 64.  Returns (words uint32 [groups * 384], written bool mask of the same shape)."""
    groups = -(-(len(corr_blocks) * stride) // 64)
    words = np.zeros(groups * 384, np.uint32)
    written = np.zeros(groups * 384, bool)
    for w, blk in enumerate(corr_blocks):
        six = np.concatenate([blk["pos_i"], blk["pos_j"]], axis=1).view(np.uint32).reshape(-1, 6)
        for e in range(len(blk)):
            E = w * stride + e
            for k in range(3):
                at = 2 * ((E // 64) * 192 + k * 64 + E % 64)
                words[at:at + 2] = six[e, 2 * k:2 * k + 2]
                written[at:at + 2] = True
    return words, written


def _move(T, p):
    T = np.asarray(T, np.float32).reshape(4, 4)
    p = np.asarray(p, np.float32).reshape(-1, 3)
    cols = []
    for r in range(3):
        v = np.float32(T[r, 0]) * p[:, 0]
        v = v + np.float32(T[r, 1]) * p[:, 1]
        v = v + np.float32(T[r, 2]) * p[:, 2]
        cols.append(v + np.float32(T[r, 3]))
    return np.stack(cols, 1).astype(np.float32)


def model_points(records, TA, TB):
    return _move(TA, records["ptA_cam"]), _move(TB, records["ptB_cam"])


def slot_tree_sum(terms):
    """terms float64 [n, ...]: slot l sums rows l, l + 256, .. in ascending order from +0; then s = 128 .. 1: acc[l] += acc[l + s]."""
    terms = np.asarray(terms, np.float64)
    acc = np.zeros((SLOTS,) + terms.shape[1:], np.float64)
    for k0 in range(0, terms.shape[0], SLOTS):
        row = terms[k0:k0 + SLOTS]
        acc[:row.shape[0]] = acc[:row.shape[0]] + row
    s = SLOTS // 2
    while s >= 1:
        acc[:s] = acc[:s] + acc[s:2 * s]
        s //= 2
    return acc[0]


def moments(a, b):
    """(n, m1, m2, S) as float64 [16]; (n, 0, .., 0) below 5 points."""
    n = a.shape[0]
    out = np.zeros(16, np.float64)
    out[0] = n
    if n < MIN_POINTS:
        return out
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    m1 = slot_tree_sum(a64) / np.float64(n)
    m2 = slot_tree_sum(b64) / np.float64(n)
    da, db = a64 - m1, b64 - m2
    S = slot_tree_sum(da[:, :, None] * db[:, None, :])
    out[1:4], out[4:7], out[7:16] = m1, m2, S.reshape(9)
    return out


def kabsch(mom):
    """fp64 (R, t, singular values, sign of det S) from the moments: R maximises tr(R S) over proper rotations."""
    m1, m2, S = mom[1:4], mom[4:7], mom[7:16].reshape(3, 3)
    U, sv, Vt = np.linalg.svd(S)
    V = Vt.T
    if np.linalg.det(V @ U.T) < 0:
        V = V.copy()
        V[:, 2] = -V[:, 2]
    R = V @ U.T
    return R, m2 - R @ m1, sv, (1.0 if np.linalg.det(S) >= 0 else -1.0)


def procrustes(records, TA, TB):
    """dict: pose (float32 4x4), pose64, err, moments, well_conditioned (second singular value >= 1e-3 of the first)."""
    a, b = model_points(records, TA, TB)
    mom = moments(a, b)
    out = {"moments": mom, "pose": np.eye(4, dtype=np.float32), "pose64": np.eye(4), "err": 0.0, "well_conditioned": False, "a": a, "b": b}
    if a.shape[0] < MIN_POINTS or not np.isfinite(mom).all():
        return out
    R, t, sv, sign = kabsch(mom)
    P = np.eye(4)
    P[:3, :3], P[:3, 3] = R, t
    if not np.isfinite(P.astype(np.float32)).all():
        return out
    d = a.astype(np.float64) @ R.T + t - b.astype(np.float64)
    out.update(pose=P.astype(np.float32), pose64=P, err=float(np.sqrt((d * d).sum()) / a.shape[0]),
               well_conditioned=bool(sv[0] > 0 and sv[1] >= 1e-3 * sv[0] and sv[1] + sign * sv[2] >= 1e-3 * sv[0]))
    return out
