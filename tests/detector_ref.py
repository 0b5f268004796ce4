"""CPU restatement of the detector front end's rules (include/btba.h, "detector front end"): numpy and Python integers, no code
shared with the product.  The crop builds the padded square as an array; the resize computes every weight with numpy's float32 /
float64 scalar arithmetic and blends whole rows at once; the grey step divides with numpy; the transform is Eigen's cofactor
inverse spelled out in float32 scalars.  Both vertical forms of OpenCV's fixed-point resize are available."""
import numpy as np

F32 = np.float32


def crop_square(color, roi):
    """The zero-padded square I [side, side, 3] (int64, B G R) of a uchar4 colour map [H, W, 4] and a ROI."""
    umin, umax, vmin, vmax = (float(v) for v in roi)
    wc, hc = int(F32(umax) - F32(umin)), int(F32(vmax) - F32(vmin))
    side = max(wc, hc)
    sq = np.zeros((side, side, 3), np.int64)
    sq[:hc, :wc] = color[int(vmin):int(vmin) + hc, int(umin):int(umin) + wc, :3]
    return sq


def axis_coeffs(S, side, columns):
    """Per output index: the two source indices and the two 11-bit weights of cv::resize's INTER_LINEAR setup."""
    inv = S / side                              # Python floats are IEEE doubles: (double)S / side
    scale = 1.0 / inv
    i0, i1, w0, w1 = [], [], [], []
    for d in range(S):
        f = F32((d + 0.5) * scale - 0.5)        # two rounded double operations, then to float
        s = int(np.floor(f))
        f = F32(f - F32(s))
        if columns:
            if s < 0:
                f, s = F32(0), 0
            if s >= side - 1:
                f, s = F32(0), side - 1
            a, b = s, s + 1 if s + 1 < side else s
        else:
            a, b = min(max(s, 0), side - 1), min(max(s + 1, 0), side - 1)
        i0.append(a)
        i1.append(b)
        w0.append(int(np.rint(F32(F32(1) - f) * F32(2048))))
        w1.append(int(np.rint(f * F32(2048))))
    return np.array(i0), np.array(i1), np.array(w0, np.int64), np.array(w1, np.int64)


def resize(sq, S, form="simd"):
    """cv::resize of the square to S x S (uint8 [S, S, 3]).  form: "simd" (VResizeLinearVec_32s8u) or "scalar"."""
    side = sq.shape[0]
    if side == 2 * S:                           # INTER_AREA, 2 x 2 box
        s = sq[0::2, 0::2] + sq[0::2, 1::2] + sq[1::2, 0::2] + sq[1::2, 1::2]
        return ((s + 2) >> 2).astype(np.uint8)
    x0, x1, a0, a1 = axis_coeffs(S, side, True)
    y0, y1, b0, b1 = axis_coeffs(S, side, False)
    h = sq[:, x0] * a0[None, :, None] + sq[:, x1] * a1[None, :, None]          # [side, S, 3] horizontal sums
    h0, h1 = h[y0], h[y1]
    B0, B1 = b0[:, None, None], b1[:, None, None]
    if form == "simd":
        out = ((((h0 >> 4) * B0) >> 16) + (((h1 >> 4) * B1) >> 16) + 2) >> 2
    else:
        out = (h0 * B0 + h1 * B1 + (1 << 21)) >> 22
    return np.clip(out, 0, 255).astype(np.uint8)


def grey(bgr):
    """OpenCV 4 RGB2GRAY applied to B G R bytes (the server's call), then / 255 in float32."""
    b, g, r = (bgr[..., k].astype(np.int64) for k in range(3))
    y = (9798 * b + 19235 * g + 3735 * r + 16384) >> 15
    return y.astype(np.float32) / np.float32(255)


def inputs(color, roi, S=400, form="simd"):
    """(bgr [S, S, 3] uint8, gray [S, S] float32) of one frame."""
    bgr = resize(crop_square(color, roi), S, form)
    return bgr, grey(bgr)


def transform(roi, S=400):
    """(fwd, bwd) float32 [3, 3]: Lfnet::detectFeature's forward transform and Eigen's cofactor inverse of it."""
    umin, umax, vmin, vmax = (F32(v) for v in roi)
    side = max(int(umax - umin), int(vmax - vmin))
    s = F32(F32(S) / F32(side))
    su, sv = F32(s * umin), F32(s * vmin)
    fwd = np.array([[s, 0, F32(0) - su], [0, s, F32(0) - sv], [0, 0, 1]], np.float32)
    det = F32(s * s)
    invdet = F32(F32(1) / det)
    r00 = F32(s * invdet)
    bwd = np.array([[r00, 0, F32(F32(su * s) * invdet)], [0, r00, F32(F32(sv * s) * invdet)], [0, 0, F32(det * invdet)]], np.float32)
    return fwd, bwd


def keypoints_to_image(kpts, roi, S=400):
    """float32 [n, 2]: (fl(fl(r00 kx) + r02), fl(fl(r11 ky) + r12))."""
    _, b = transform(roi, S)
    k = np.asarray(kpts, np.float32).reshape(-1, 2)
    x = (k[:, 0] * b[0, 0]).astype(np.float32) + b[0, 2]
    y = (k[:, 1] * b[1, 1]).astype(np.float32) + b[1, 2]
    return np.stack([x, y], 1).astype(np.float32)
