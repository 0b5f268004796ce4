"""btba_ingest_frames restated in numpy (include/btba.h, "frame ingest"): the depth decode and the colour pack, exact, and the
chain that follows them through the CPU oracle's process_depth / depth_to_normals."""
import numpy as np


def decode_depth(codes):
    """Utils::readDepthImage (src/Utils.cpp:50-69): (float)((double)(float)u * 0.001), 0 when (double)d < 0.1."""
    u = np.asarray(codes).view(np.uint16) if np.asarray(codes).dtype == np.int16 else np.asarray(codes, np.uint16)
    d = (u.astype(np.float32).astype(np.float64) * 0.001).astype(np.float32)
    d[d.astype(np.float64) < 0.1] = 0.0
    return d


def decode_depth_float_shortcut(codes):
    """The product taken in float, u * 0.001f: NOT the rule (it differs in the last bit for most codes); kept for the guard."""
    d = np.asarray(codes, np.uint16).astype(np.float32) * np.float32(0.001)
    d[d.astype(np.float64) < 0.1] = 0.0
    return d


def pack_color(bgr):
    """Frame::updateColorGPU (src/Frame.cpp:114-127): [H, W, 3] BGR bytes -> [H, W, 4] (B, G, R, 0)."""
    bgr = np.asarray(bgr, np.uint8)
    out = np.zeros(bgr.shape[:2] + (4,), np.uint8)
    out[..., :3] = bgr
    return out


def restate(oracle, codes, bgr, K, depth_params=()):
    """Frame's constructor after the imreads on the CPU oracle: (raw, depth, normals, xyz, colour)."""
    raw = decode_depth(codes)
    depth = oracle.process_depth(raw, *depth_params)
    normals, xyz = oracle.depth_to_normals(depth, K)
    return raw, depth, normals, xyz, None if bgr is None else pack_color(bgr)


def metres_to_codes(depth):
    """A float depth map quantised to the millimetre codes a 16-bit depth PNG holds."""
    return np.clip(np.rint(np.asarray(depth, np.float64) * 1000.0), 0, 65535).astype(np.uint16)
