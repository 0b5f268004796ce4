"""Test-side restatement of btba_apply_masks (include/btba.h) in numpy and Python integers: 8-connected labelling with
components numbered by their first pixel in raster order, the largest-component rule with its tie break, Andrew's monotone
chain over the component's run ends, the closed-hull fill by integer cross products, the zero-border dilation, the
invalidation and the ROI.  It shares no code with the kernels (bundletrack_amd/csrc/btba_mask.hpp): runs instead of a pixel
forest, all run ends sorted by (x, y) instead of per-row extremes in (y, x) order, a per-pixel half-plane test instead of
per-row spans."""
from __future__ import annotations

import numpy as np


def runs_of(fg: np.ndarray):
    """[(y, x_start, x_end)] of every horizontal run of foreground pixels, in raster order."""
    out = []
    for y in range(fg.shape[0]):
        row = np.concatenate([[0], fg[y].astype(np.int8), [0]])
        d = np.diff(row)
        for a, b in zip(np.flatnonzero(d == 1), np.flatnonzero(d == -1) - 1):
            out.append((y, int(a), int(b)))
    return out


def label8(fg: np.ndarray):
    """(labels, runs, run_comp): labels [H, W] int64, 0 off the mask and 1, 2, ... numbered by each component's first pixel
    in raster order (scipy.ndimage.label's and OpenCV's numbering)."""
    fg = np.asarray(fg) != 0
    runs = runs_of(fg)
    parent = list(range(len(runs)))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    by_row: dict = {}
    for i, (y, a, b) in enumerate(runs):
        for j in by_row.get(y - 1, []):                      # 8-connected: the runs overlap after widening one by a pixel each side
            _, c, d = runs[j]
            if c <= b + 1 and a <= d + 1:
                ri, rj = find(i), find(j)
                if ri != rj:
                    parent[max(ri, rj)] = min(ri, rj)       # the root is the component's first run in raster order
        by_row.setdefault(y, []).append(i)
    roots = [find(i) for i in range(len(runs))]
    number = {}
    for r in roots:                                          # raster order of the first runs
        if r not in number:
            number[r] = len(number) + 1
    labels = np.zeros(fg.shape, np.int64)
    run_comp = []
    for (y, a, b), r in zip(runs, roots):
        labels[y, a:b + 1] = number[r]
        run_comp.append(number[r])
    return labels, runs, run_comp


def largest_component(fg: np.ndarray):
    """(label of the winner or 0, labels, runs, run_comp): most pixels, ties to the lowest label (the first in raster order)."""
    labels, runs, run_comp = label8(fg)
    if not runs:
        return 0, labels, runs, run_comp
    sizes: dict = {}
    for (y, a, b), c in zip(runs, run_comp):
        sizes[c] = sizes.get(c, 0) + (b - a + 1)
    best = max(sizes, key=lambda c: (sizes[c], -c))
    return best, labels, runs, run_comp


def cross(o, a, b) -> int:
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def monotone_chain(points):
    """Andrew's monotone chain on integer (x, y) points: the strictly convex vertices counter-clockwise (collinear points
    dropped); one point for a single point, two for a segment."""
    pts = sorted(set((int(x), int(y)) for x, y in points))
    if len(pts) <= 1:
        return pts
    lower, upper = [], []
    for p in pts:
        while len(lower) >= 2 and cross(lower[-2], lower[-1], p) <= 0:
            lower.pop()
        lower.append(p)
    for p in reversed(pts):
        while len(upper) >= 2 and cross(upper[-2], upper[-1], p) <= 0:
            upper.pop()
        upper.append(p)
    return lower[:-1] + upper[:-1]


def fill_hull(hull, H: int, W: int) -> np.ndarray:
    """1 where the integer point (x, y) lies in the closed convex polygon `hull` (counter-clockwise in x, y), else 0."""
    out = np.zeros((H, W), np.uint8)
    if not hull:
        return out
    hx, hy = [p[0] for p in hull], [p[1] for p in hull]
    ys, xs = np.mgrid[0:H, 0:W].astype(np.int64)
    inside = (xs >= min(hx)) & (xs <= max(hx)) & (ys >= min(hy)) & (ys <= max(hy))
    for k in range(len(hull)):
        (ax, ay), (bx, by) = hull[k], hull[(k + 1) % len(hull)]
        inside &= (bx - ax) * (ys - ay) - (by - ay) * (xs - ax) >= 0
    out[inside] = 1
    return out


def hull_of_largest(fg: np.ndarray):
    """(M0, hull vertices, winner's pixel mask) of the hull path."""
    fg = np.asarray(fg) != 0
    best, labels, runs, run_comp = largest_component(fg)
    if best == 0:
        return np.zeros(fg.shape, np.uint8), [], np.zeros(fg.shape, bool)
    ends = []
    for (y, a, b), c in zip(runs, run_comp):
        if c == best:
            ends += [(a, y), (b, y)]
    hull = monotone_chain(ends)
    return fill_hull(hull, *fg.shape), hull, labels == best


def dilate(m0: np.ndarray, d: int) -> np.ndarray:
    """OR over the d x d square centred at each pixel; outside the image counts as 0."""
    r = d // 2
    H, W = m0.shape
    p = np.zeros((H + 2 * r, W + 2 * r), np.uint8)
    p[r:r + H, r:r + W] = m0 != 0
    h = np.zeros((H + 2 * r, W), np.uint8)
    for k in range(d):
        h |= p[:, k:k + W]
    out = np.zeros((H, W), np.uint8)
    for k in range(d):
        out |= h[k:k + H]
    return out


def final_mask(mask: np.ndarray, hull: bool, d: int) -> np.ndarray:
    m0 = hull_of_largest(mask)[0] if hull else (np.asarray(mask) != 0).astype(np.uint8)
    return dilate(m0, d)


def roi_of(M: np.ndarray) -> np.ndarray:
    """The reference's loop (Frame.cpp:359-372) from (9999, 0, 9999, 0)."""
    ys, xs = np.nonzero(M)
    if xs.size == 0:
        return np.array([9999, 0, 9999, 0], np.float32)
    return np.array([min(9999, xs.min()), max(0, xs.max()), min(9999, ys.min()), max(0, ys.max())], np.float32)


def restate(mask, depth, normal, color, *, hull: bool, d: int):
    """(M, depth, normal, color or None, roi) of one frame: btba_apply_masks' outputs."""
    M = final_mask(mask, hull, d)
    off = M == 0
    depth, normal = np.array(depth, np.float32, copy=True), np.array(normal, np.float32, copy=True)
    depth[off] = 0
    normal[off] = 0
    if color is not None:
        color = np.array(color, np.uint8, copy=True)
        color[off] = 0
    return M, depth, normal, color, roi_of(M)
