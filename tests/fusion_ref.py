"""btba_fuse_frames / btba_fuse_bounds / btba_voxel_downsample restated in numpy (include/btba.h, "keyframe fusion"): float32 products
and sums in the stated order, np.floor, np.rint on float64, Python integer sums.  Every output is meant to equal the device's byte for
byte.  The voxel rule is pcl::VoxelGrid::applyFilter's, restated from PCL's published header and unverified against a PCL run.

A segment is a dict: {"instance": b, "pose": [4,4] float32 camera -> model} with either "depth" [H,W] float32 (a frame; "normal"
[H,W,4] float32 or None, "colour" [H,W,4] uint8 or None) or "xyz" [n,4] float32 (a point list; "normal" [n,4] or None, "colour" [n,4] or
None)."""
import numpy as np

F = np.float32
MAX_COORD = F(65536.0)
SCALE = 1048576.0       # 2^20


def kinv4(oracle, K):
    """The Kinv of btba_depth_to_normals: the fp32 cofactor inverse of the 4 x 4 embedding of K (the CPU oracle's mat4_inverse)."""
    K4 = np.eye(4, dtype=F)
    K4[:3, :3] = np.asarray(K, F)
    return np.ascontiguousarray(oracle.mat4_inverse(K4), F).reshape(16)


def backproject(depth, Ki):
    """btba_image.hpp::backproject on every pixel: ([H*W, 3] float32, keep [H*W]) with keep = (double)d >= 0.1."""
    d = np.ascontiguousarray(depth, F)
    H, W = d.shape
    y, x = np.divmod(np.arange(H * W), W)
    d = d.reshape(-1)
    with np.errstate(invalid="ignore", over="ignore"):
        keep = d.astype(np.float64) >= 0.1
        vx, vy = x.astype(F) * d, y.astype(F) * d
        row = lambda r: ((Ki[4 * r] * vx + Ki[4 * r + 1] * vy) + Ki[4 * r + 2] * d) + Ki[4 * r + 3] * d
        return np.stack([row(0), row(1), row(3)], 1).astype(F), keep


def segment_points(seg, Ki, require_normals=True):
    """The surviving points of one segment in the model frame: (p [m,3] float32, n [m,3] float32, colour [m,3] uint8 or None)."""
    T = np.asarray(seg["pose"], F).reshape(4, 4)
    nmap, cmap = seg.get("normal"), seg.get("colour")
    if seg.get("depth") is not None:
        c, keep = backproject(seg["depth"], Ki)
        nq = np.zeros_like(c) if nmap is None else np.asarray(nmap, F).reshape(-1, 4)[:, :3]
        if require_normals and nmap is not None:
            keep = keep & ~((nq[:, 0] == 0) & (nq[:, 1] == 0) & (nq[:, 2] == 0))
    else:
        c = np.asarray(seg["xyz"], F).reshape(-1, 4)[:, :3]
        keep = np.isfinite(c).all(1)
        nq = np.zeros_like(c) if nmap is None else np.asarray(nmap, F).reshape(-1, 4)[:, :3]
    c, nq = c[keep], nq[keep]
    with np.errstate(invalid="ignore", over="ignore"):
        p = np.stack([((T[r, 0] * c[:, 0] + T[r, 1] * c[:, 1]) + T[r, 2] * c[:, 2]) + T[r, 3] for r in range(3)], 1).astype(F)
        n = np.stack([(T[r, 0] * nq[:, 0] + T[r, 1] * nq[:, 1]) + T[r, 2] * nq[:, 2] for r in range(3)], 1).astype(F)
        bad = ~(np.abs(n) < MAX_COORD).all(1)
    n[bad] = 0
    col = None if cmap is None else np.asarray(cmap, np.uint8).reshape(-1, 4)[keep][:, :3]
    return p, n, col


def cells(p, leaf):
    """(cell [m,3] int64 = floorf(p * inv_leaf), representable [m] = every |p_a| < 2^16)."""
    inv_leaf = F(1.0) / F(leaf)
    with np.errstate(invalid="ignore", over="ignore"):
        ok = (np.abs(p) < MAX_COORD).all(1)
        c = np.floor(np.where(ok[:, None], p, F(0)) * inv_leaf)
    return c.astype(np.int64), ok


def bounds(segments, n_instances, Ki, leaf, require_normals=True):
    """btba_fuse_bounds: int32 [n_instances, 6] = (min_b, dims); six zeros without a surviving representable point."""
    lo = [None] * n_instances
    hi = [None] * n_instances
    for seg in segments:
        p, _, _ = segment_points(seg, Ki, require_normals)
        c, ok = cells(p, leaf)
        c = c[ok]
        if len(c) == 0:
            continue
        b = seg["instance"]
        lo[b] = c.min(0) if lo[b] is None else np.minimum(lo[b], c.min(0))
        hi[b] = c.max(0) if hi[b] is None else np.maximum(hi[b], c.max(0))
    box = np.zeros((n_instances, 6), np.int32)
    for b in range(n_instances):
        if lo[b] is not None:
            box[b, :3], box[b, 3:] = lo[b], hi[b] - lo[b] + 1
    return box


def fuse(segments, n_instances, Ki, box, leaf, min_points=1, require_normals=True, normalize_normals=False, with_colour=True):
    """btba_fuse_frames: per instance a dict of xyz [k,4] float32, normal [k,4] float32, colour [k,4] uint8 (with_colour), count [k] uint32,
    lin [k] int32, n_out, n_outside -- without a capacity: all qualifying voxels."""
    box = np.asarray(box, np.int64).reshape(n_instances, 6)
    acc = [dict() for _ in range(n_instances)]            # lin -> [n, sx, sy, sz, nx, ny, nz, c0, c1, c2] in Python integers
    n_outside = [0] * n_instances
    for seg in segments:
        b = seg["instance"]
        p, n, col = segment_points(seg, Ki, require_normals)
        c, ok = cells(p, leaf)
        i = c - box[b, :3]
        inside = ok & (i >= 0).all(1) & (i < box[b, 3:]).all(1)
        n_outside[b] += int((~inside).sum())
        lin = i[:, 0] + box[b, 3] * (i[:, 1] + box[b, 4] * i[:, 2])
        qp = np.rint(p.astype(np.float64) * SCALE)
        qn = np.rint(n.astype(np.float64) * SCALE)
        for k in np.flatnonzero(inside):
            a = acc[b].setdefault(int(lin[k]), [0] * 10)
            a[0] += 1
            for j in range(3):
                a[1 + j] += int(qp[k, j])
                a[4 + j] += int(qn[k, j])
                if with_colour:
                    a[7 + j] += int(col[k, j])
    out = []
    for b in range(n_instances):
        lins = sorted(l for l, a in acc[b].items() if a[0] >= min_points)
        k = len(lins)
        xyz, nrm = np.zeros((k, 4), F), np.zeros((k, 4), F)
        colour, count = np.zeros((k, 4), np.uint8), np.zeros(k, np.uint32)
        for r, l in enumerate(lins):
            a = acc[b][l]
            cnt = a[0]
            count[r] = cnt
            xyz[r] = [F(np.float64(float(a[1 + j])) / SCALE / np.float64(cnt)) for j in range(3)] + [F(1)]
            m = np.array([F(np.float64(float(a[4 + j])) / SCALE / np.float64(cnt)) for j in range(3)], F)
            if normalize_normals:
                length = np.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2])
                m = m / length if length > 0 else np.zeros(3, F)
            nrm[r, :3] = m
            if with_colour:
                colour[r, :3] = [(2 * a[7 + j] + cnt) // (2 * cnt) for j in range(3)]
        d = {"xyz": xyz, "normal": nrm, "count": count, "lin": np.array(lins, np.int32).reshape(k), "n_out": k, "n_outside": n_outside[b]}
        if with_colour:
            d["colour"] = colour
        out.append(d)
    return out


def voxel_downsample(xyz, leaf, normal=None, colour=None, box=None, **kw):
    """btba_voxel_downsample of one cloud: fuse() of one point-list segment with the identity pose; box None = the data-derived box."""
    seg = [{"instance": 0, "pose": np.eye(4, dtype=F), "xyz": xyz, "normal": normal, "colour": colour}]
    if box is None:
        box = bounds(seg, 1, None, leaf)
    return fuse(seg, 1, None, box, leaf, with_colour=colour is not None, **kw)[0], box


# ---- the synthetic object of the tests: a sphere seen from poses around it ------------------------------------------------------

def look_at_pose(cam_pos):
    """camera -> model: the camera at cam_pos (model frame), its z axis through the model origin."""
    cam_pos = np.asarray(cam_pos, np.float64)
    z = -cam_pos / np.linalg.norm(cam_pos)
    x = np.cross([0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    T = np.eye(4)
    T[:3, 0], T[:3, 1], T[:3, 2], T[:3, 3] = x, y, z, cam_pos
    return T.astype(F)


def sphere_frame(pose, K, H, W, radius=0.12, seed=0):
    """Depth, analytic normals (zero on a band of rows, as a frame's rim has them) and random colour of a sphere at the model origin."""
    T = np.asarray(pose, np.float64)
    centre = -T[:3, :3].T @ T[:3, 3]                      # the model origin in the camera frame
    v, u = np.mgrid[0:H, 0:W]
    Kd = np.asarray(K, np.float64)
    ray = np.stack([(u - Kd[0, 2]) / Kd[0, 0], (v - Kd[1, 2]) / Kd[1, 1], np.ones((H, W))], -1)
    a = (ray * ray).sum(-1)
    bq = (ray * centre).sum(-1)
    disc = bq * bq - a * (centre @ centre - radius * radius)
    hit = disc > 0
    t = (bq - np.sqrt(np.where(hit, disc, 0))) / a
    depth = np.where(hit, t, 0.0).astype(F)
    normal = np.zeros((H, W, 4), F)
    normal[..., :3] = np.where(hit[..., None], (ray * t[..., None] - centre) / radius, 0.0)
    normal[H // 2] = 0                                    # valid depth, no normal: what require_normals decides about
    colour = np.zeros((H, W, 4), np.uint8)
    colour[..., :3] = np.random.default_rng(seed).integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    return depth, normal, colour


def small_K(H, W):
    return np.array([[W * 0.95, 0, (W - 1) / 2], [0, W * 0.95, (H - 1) / 2], [0, 0, 1]], F)


def sphere_segments(cam_positions, instance, K, H, W, seed=0, radius=0.12):
    segs = []
    for k, c in enumerate(cam_positions):
        pose = look_at_pose(c)
        d, n, col = sphere_frame(pose, K, H, W, radius, seed=seed + k)
        segs.append({"instance": instance, "pose": pose, "depth": d, "normal": n, "colour": col})
    return segs


THREE_VIEWS = [(0.0, 0.0, -0.5), (0.3, 0.1, -0.4), (-0.25, -0.2, -0.38)]
