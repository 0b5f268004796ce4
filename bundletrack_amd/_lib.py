"""ctypes binding of libbtba.so (the C ABI of include/btba.h).

The HIP library is the product; this module only loads it.  It fails loudly when the
library is missing -- there is no CPU fallback anywhere in the package.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_PKG)
LIB_PATH = os.path.join(_PKG, "libbtba.so")
SRC_DIR = os.path.join(_PKG, "csrc")
HEADER = os.path.join(_ROOT, "include", "btba.h")

BTBA_OK, BTBA_EINVAL, BTBA_EHIP, BTBA_ENUMERIC, BTBA_ENOMEM, BTBA_ESCHED = 0, 1, 2, 3, 4, 5
PAIRS_TARGET_LOWER, PAIRS_TARGET_MORE_VALID, PAIRS_EXPLICIT, PAIRS_TARGET_HIGHER = 0, 1, 2, 3
REDUCE_DETERMINISTIC, REDUCE_ATOMIC = 0, 1
RANSAC_REFERENCE_SVD, RANSAC_HORN = 0, 1
RANSAC_DRAW_HASH = 0x100      # ORed into `hypothesis`: counter-hash sample triples instead of the reference's cuRAND XORWOW stream
FLAG_TRACE, FLAG_TIME_KERNELS = 1, 2
FLAG_OVERLAP, FLAG_NO_FUSE, FLAG_KEYED_CORR, FLAG_FLOAT4_CACHE, FLAG_NO_COMPACTION, FLAG_COMPACTION, FLAG_TIME_SAMPLED = 32, 64, 4096, 256, 512, 1024, 2048
OPT_DENSE_ORDER, OPT_TILE_MAJOR, OPT_BLOCK_WALK, OPT_BLOCK_SKIP, OPT_BIG_ASSEMBLY, OPT_OVERLAP_GROUPS, OPT_OVERLAP_EQUAL_PRIO, OPT_KEYED_CORR_MIN_BYTES, OPT_SPARSE_TAIL = 1, 2, 3, 4, 5, 6, 7, 8, 9
OPT_CHAIN, OPT_CHAIN_SPARSE_PERIOD, OPT_CHAIN_TIMEOUT_MS = 10, 11, 12      # retired with the chained launch: validated and ignored
OPT_COUNT_LIVE, OPT_RELAYOUT, OPT_CORR_NONTEMPORAL, OPT_SOLVE_SMALL = 13, 14, 15, 16

ENTRYJ_DTYPE = np.dtype(
    [("imgIdx_i", "<u4"), ("imgIdx_j", "<u4"), ("pos_i", "<f4", (3,)), ("pos_j", "<f4", (3,))]
)

EXPORTED_SYMBOLS = [
    "btba_params_default", "btba_strerror", "btba_last_hip_error", "btba_version",
    "btba_workspace_create", "btba_workspace_create_on_stream", "btba_workspace_destroy", "btba_workspace_sync",
    "btba_workspace_wait_stream", "btba_workspace_signal_stream", "btba_workspace_set_option", "btba_workspace_live_blocks",
    "btba_optimize_frames", "btba_optimize_frames_keyed", "btba_frame_cache_clear", "btba_frame_cache_evict", "btba_ransac_pairs", "btba_ransac_pairs_ex", "btba_ransac_reference_uniforms", "btba_build_cache", "btba_solve_batch", "btba_solve_cached", "btba_collect_stats",
    "btba_trace_layout_get", "btba_bucket_correspondences",
    "btba_matrices_to_poses", "btba_poses_to_matrices",
    "btba_process_depth", "btba_depth_to_normals", "btba_ingest_params_default", "btba_ingest_frames",
     "btba_vos_params_default", "btba_vos_sample_frames", "btba_vos_first_labels", "btba_vos_propagate", "btba_vos_masks", "btba_vos_inputs",
    "btba_vos_net_config_default", "btba_vos_net_layer_count", "btba_vos_net_model_create", "btba_vos_net_model_destroy", "btba_vos_net_out_size", "btba_vos_features",
    "btba_build_cache_zn", "btba_pack_zn", "btba_solve_batch_zn", "btba_zn_block_ranges", "btba_zn_valid_lists", "btba_solve_batch_zn_aux", "btba_pack_correspondences24",
    "btba_match_params_default", "btba_match_capacity", "btba_match_pairs",
    "btba_lfnet_params_default", "btba_lfnet_heatmaps", "btba_lfnet_select", "btba_lfnet_crops", "btba_lfnet_keypoints",
    "btba_lfnet_desc_config_default", "btba_lfnet_desc_model_create", "btba_lfnet_desc_model_destroy", "btba_lfnet_descriptors",
    "btba_lfnet_det_config_default", "btba_lfnet_det_scales", "btba_lfnet_det_model_create", "btba_lfnet_det_model_destroy", "btba_lfnet_det_map_size",
    "btba_lfnet_det_map_sizes", "btba_lfnet_det_pad_size", "btba_lfnet_scores",
    "btba_mask_params_default", "btba_apply_masks",
    "btba_detector_params_default", "btba_detector_transform", "btba_detector_inputs", "btba_detector_keypoints_to_image",
    "btba_pose_errors", "btba_nocs_params_default", "btba_nocs_errors",
    "btba_mappoints_create", "btba_mappoints_destroy", "btba_mappoints_register_frame", "btba_mappoints_forget_frame", "btba_mappoints_export",
    "btba_corres_params_default", "btba_corres_chain_capacity", "btba_corres_chain",
    "btba_window_layout", "btba_marshal_windows", "btba_procrustes_pairs",
    "btba_linearize_batch_zn_aux", "btba_pose_covariances", "btba_objective_batch_zn_aux",
    "btba_fuse_params_default", "btba_fuse_layout", "btba_fuse_bounds", "btba_fuse_frames", "btba_voxel_downsample",
    "btba_register_params_default", "btba_register_index", "btba_register_frames", "btba_register_associate",
    "btba_keyframes_create", "btba_keyframes_destroy", "btba_keyframes_reset", "btba_keyframes_check_add", "btba_keyframes_select",
    "btba_keyframes_writeback", "btba_keyframes_export", "btba_rotation_distances",
]
FUSE_FRAME, FUSE_POINTS, FUSE_OVERFLOW, FUSE_MAX_VOXELS = 0, 1, 1, 1 << 24
REG_CONVERGED, REG_MAX_ITERS, REG_DEGENERATE, REG_TOO_FEW, REG_SKIPPED = 0, 1, 2, 3, 4
REG_STATUS_NAMES = ("CONVERGED", "MAX_ITERS", "DEGENERATE", "TOO_FEW", "SKIPPED")

# btba_register_iter / btba_register_result (include/btba.h): 344 and 32 bytes
REGISTER_ITER_DTYPE = np.dtype(
    [("n_valid", "<i4"), ("n_matched", "<i4"), ("n_beyond", "<i4"), ("status", "<i4"), ("cost", "<f8"), ("H", "<f8", (21,)), ("g", "<f8", (6,)),
     ("xi", "<f8", (6,)), ("pivot_ratio", "<f8"), ("pose", "<f4", (12,))]
)
REGISTER_RESULT_DTYPE = np.dtype(
    [("status", "<i4"), ("iters_done", "<i4"), ("n_valid", "<i4"), ("n_matched", "<i4"), ("n_beyond", "<i4"), ("reserved", "<i4"), ("cost", "<f8")]
)

# btba_objective_pair / btba_objective_total (include/btba.h): 40 and 64 bytes
OBJECTIVE_PAIR_DTYPE = np.dtype(
    [("sum_sq", "<f8"), ("sum_rho", "<f8"), ("max_abs", "<f8"), ("count", "<i4"), ("n_outlier", "<i4"), ("worst", "<i4"), ("reserved", "<i4")]
)
OBJECTIVE_TOTAL_DTYPE = np.dtype(
    [("objective", "<f8"), ("sparse_rho", "<f8"), ("dense_rho", "<f8"), ("sparse_sq", "<f8"), ("dense_wsq", "<f8"),
     ("n_sparse", "<i8"), ("n_dense", "<i8"), ("n_residuals", "<i8")]
)

# btba_match (include/btba.h): one descriptor match, 40 bytes
MATCH_DTYPE = np.dtype(
    [("idx_a", "<i4"), ("idx_b", "<i4"), ("dist", "<f4"), ("dir", "<i4"), ("ptA_cam", "<f4", (3,)), ("ptB_cam", "<f4", (3,))]
)


class Params(C.Structure):
    _fields_ = [
        ("n_gn_iters", C.c_int32), ("n_pcg_iters", C.c_int32),
        ("robust_delta", C.c_float), ("dense_dist_thresh", C.c_float), ("dense_normal_thresh", C.c_float),
        ("depth_min", C.c_float), ("depth_max", C.c_float),
        ("weight_sparse", C.c_float), ("weight_dense_depth", C.c_float), ("image_downscale", C.c_float),
        ("pair_policy", C.c_int32), ("dense_tiles", C.c_int32), ("sparse_chunks", C.c_int32), ("flags", C.c_int32), ("reduction_mode", C.c_int32),
        ("weights_sparse_per_iter", C.c_void_p), ("weights_dense_per_iter", C.c_void_p),      # host float[n_gn_iters] or NULL (the scalars)
        ("n_weights_per_iter", C.c_int32),                                                     # their length (must equal n_gn_iters when either is set)
    ]


class MatchParams(C.Structure):
    """btba_match_params (include/btba.h)."""
    _fields_ = [("k", C.c_int32), ("mutual", C.c_int32), ("max_dist_neighbor", C.c_float), ("cos_max_normal_neighbor", C.c_float),
                ("max_dist_no_neighbor", C.c_float), ("cos_max_normal_no_neighbor", C.c_float), ("min_z", C.c_float)]


class MaskParams(C.Structure):
    """btba_mask_params (include/btba.h)."""
    _fields_ = [("largest_component_hull", C.c_int32), ("dilate", C.c_int32)]


class IngestParams(C.Structure):
    """btba_ingest_params (include/btba.h)."""
    _fields_ = [("depth_format", C.c_int32), ("erode_radius", C.c_int32), ("erode_diff", C.c_float), ("erode_ratio", C.c_float),
                ("bf_radius", C.c_int32), ("sigma_d", C.c_float), ("sigma_r", C.c_float)]


class VosParams(C.Structure):
    """btba_vos_params (include/btba.h)."""
    _fields_ = [("ref_num", C.c_int32), ("range", C.c_int32), ("sigma_dense", C.c_float), ("sigma_sparse", C.c_float), ("temperature", C.c_float),
                ("continuous_frames", C.c_int32), ("sparse_after", C.c_int32)]


class VosNetConfig(C.Structure):
    """btba_vos_net_config (include/btba.h)."""
    _fields_ = [("block", C.c_int32), ("layers", C.c_int32 * 4), ("bn_eps", C.c_float)]


class VosNetLayer(C.Structure):
    """btba_vos_net_layer (include/btba.h)."""
    _fields_ = [(n, C.c_void_p) for n in ("weight", "bn_weight", "bn_bias", "running_mean", "running_var")]


class LfnetParams(C.Structure):
    """btba_lfnet_params (include/btba.h)."""
    _fields_ = [("sm_ksize", C.c_int32), ("com_strength", C.c_float), ("score_com_strength", C.c_float), ("scale_com_strength", C.c_float),
                ("nms_thresh", C.c_float), ("nms_ksize", C.c_int32), ("top_k", C.c_int32), ("pad_size", C.c_int32), ("crop_radius", C.c_int32),
                ("soft_kpts", C.c_int32), ("kp_loc_size", C.c_int32), ("do_softmax_kp_refine", C.c_int32), ("kp_com_strength", C.c_float),
                ("patch_size", C.c_int32)]


class LfnetDescConfig(C.Structure):
    """btba_lfnet_desc_config (include/btba.h)."""
    _fields_ = [("patch_size", C.c_int32), ("depth", C.c_int32), ("channels", C.c_int32), ("fc_dim", C.c_int32), ("out_dim", C.c_int32),
                ("activation", C.c_int32), ("leaky_alpha", C.c_float), ("norm", C.c_int32), ("bn_eps", C.c_float)]


class LfnetDescLayer(C.Structure):
    """btba_lfnet_desc_layer (include/btba.h): host float arrays, NULL where the layer has none."""
    _fields_ = [(n, C.c_void_p) for n in ("weights", "biases", "gamma", "beta", "moving_mean", "moving_variance")]


class LfnetDescWeights(C.Structure):
    """btba_lfnet_desc_weights (include/btba.h)."""
    _fields_ = [("conv", LfnetDescLayer * 4), ("fc1", LfnetDescLayer), ("fc2", LfnetDescLayer)]


class LfnetDetConfig(C.Structure):
    """btba_lfnet_det_config (include/btba.h)."""
    _fields_ = [("channels", C.c_int32), ("ksize", C.c_int32), ("blocks", C.c_int32), ("num_scales", C.c_int32),
                ("scale_factors", C.c_double * 16), ("activation", C.c_int32), ("leaky_alpha", C.c_float), ("bn_eps", C.c_float)]


class LfnetDetBlock(C.Structure):
    """btba_lfnet_det_block (include/btba.h)."""
    _fields_ = [("pre_bn", LfnetDescLayer), ("conv1", LfnetDescLayer), ("conv2", LfnetDescLayer)]


class LfnetDetWeights(C.Structure):
    """btba_lfnet_det_weights (include/btba.h)."""
    _fields_ = [("init_conv", LfnetDescLayer), ("block", LfnetDetBlock * 8), ("fin_bn", LfnetDescLayer), ("score_conv", LfnetDescLayer * 16),
                ("ori_conv", LfnetDescLayer)]


class DetectorParams(C.Structure):
    """btba_detector_params (include/btba.h)."""
    _fields_ = [("out_size", C.c_int32)]


class NocsParams(C.Structure):
    """btba_nocs_params (include/btba.h)."""
    _fields_ = [("rot_thresh_deg", C.c_double), ("shift_thresh", C.c_double), ("iou_thresh", C.c_double), ("n_sym_steps", C.c_int32),
                ("flip_z180_pred", C.c_int32), ("normalize_columns", C.c_int32), ("clamp_acos", C.c_int32)]


class Stats(C.Structure):
    _fields_ = [
        ("n_instances", C.c_int32), ("n_frames", C.c_int32), ("n_pairs", C.c_int32), ("n_dense_pairs", C.c_int32),
        ("n_corr", C.c_int64),
        ("dense_tiles", C.c_int32), ("sparse_chunks", C.c_int32),
        ("ms_total", C.c_float), ("ms_upload", C.c_float), ("ms_cache", C.c_float), ("ms_solve", C.c_float),
        ("ms_dense_sweep", C.c_float), ("ms_sparse_sweep", C.c_float), ("ms_system_solve", C.c_float),
        ("n_dense_launches", C.c_int32), ("n_sparse_launches", C.c_int32), ("n_solve_launches", C.c_int32),
        ("bytes_dense_alg", C.c_int64), ("bytes_sparse_alg", C.c_int64),
        ("fused_sweeps", C.c_int32), ("cache_frames_built", C.c_int32), ("corr_pairs_uploaded", C.c_int32),
        ("chain_iterations", C.c_int32),
    ]

    def as_dict(self):
        return {f[0]: getattr(self, f[0]) for f in self._fields_}


class ZnAux(C.Structure):
    """btba_zn_aux (include/btba.h): device pointers to data derived from compact caches alone."""
    _fields_ = [("block_ranges", C.c_void_p), ("valid_lists", C.c_void_p), ("valid_counts", C.c_void_p), ("corr24", C.c_void_p)]


class TraceLayout(C.Structure):
    _fields_ = [(n, C.c_int64) for n in
                ("record_floats", "off_x", "off_T", "off_rhs", "off_precond", "off_pcg", "off_delta", "off_dense_pair", "off_A", "off_clk")]


class CorresParams(C.Structure):
    """btba_corres_params (include/btba.h): the RANSAC settings of btba_corres_chain."""
    _fields_ = [("n_trials", C.c_int32), ("dist_thres", C.c_float), ("hypothesis", C.c_int32), ("pad", C.c_int32), ("seed", C.c_uint64)]


class FuseParams(C.Structure):
    """btba_fuse_params (include/btba.h)."""
    _fields_ = [("leaf", C.c_float), ("min_points", C.c_int32), ("require_normals", C.c_int32), ("normalize_normals", C.c_int32)]


class FuseSegment(C.Structure):
    """btba_fuse_segment (include/btba.h): 104 bytes."""
    _fields_ = [("kind", C.c_int32), ("instance", C.c_int32), ("n", C.c_int64), ("geom", C.c_void_p), ("normal", C.c_void_p),
                ("colour", C.c_void_p), ("pose", C.c_float * 16)]


class RegisterParams(C.Structure):
    """btba_register_params (include/btba.h): 44 bytes."""
    _fields_ = [("leaf", C.c_float), ("search_radius", C.c_int32), ("max_dist", C.c_float), ("min_cos", C.c_float), ("huber_delta", C.c_float),
                ("n_iters", C.c_int32), ("eps_rot", C.c_float), ("eps_trans", C.c_float), ("min_matches", C.c_int32), ("require_normals", C.c_int32),
                ("reserved", C.c_int32)]


class BtbaError(RuntimeError):
    def __init__(self, status: int, where: str):
        self.status = status
        msg = lib().btba_strerror(status).decode() if _lib is not None else str(status)
        extra = f" (hipError {lib().btba_last_hip_error()})" if status == BTBA_EHIP else ""
        super().__init__(f"{where}: {msg}{extra}")


# The hipcc flags of libbtba.so, shared with the test-only device probe (tests/hip/btba_probe.hip) so that both compile the product's
# device functions identically.  -fno-slp-vectorize: the SLP pass packs neighbouring fp32 operations into v_pk_{mul,add,fma}_f32, which
# issue at half rate on gfx950 and need register-pair shuffling (v_mov) around them; measured -14 % on the dense sweep, -7 % on the
# sparse sweep without it.
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-slp-vectorize", "-Wno-pass-failed", "-fPIC", "-shared", "-fvisibility=hidden"]


def build(force: bool = False, verbose: bool = False, out: str | None = None, extra_flags=()) -> str:
    """Compile the HIP extension in-tree for gfx950 (hipcc cross-compiles without a GPU).

    Every csrc/*.hip is one translation unit: compiled concurrently into build/<library name>/ beside the library, then linked.
    `out` (another library path) and `extra_flags` (compile flags such as -save-temps or -DBTBA_REFERENCE_ORDER; temporaries land in
    the object directory) are for developer A/B builds.  Anything in csrc/ or include/btba.h newer than the library rebuilds all of it.
    """
    out = os.path.abspath(out or LIB_PATH)
    srcs = [os.path.join(SRC_DIR, f) for f in os.listdir(SRC_DIR)] + [HEADER]
    newest = max(os.path.getmtime(s) for s in srcs)
    if not force and os.path.exists(out) and os.path.getmtime(out) >= newest:
        return out
    units = sorted(s for s in srcs if s.endswith(".hip"))
    obj_dir = os.path.join(os.path.dirname(out), "build", os.path.splitext(os.path.basename(out))[0])
    os.makedirs(obj_dir, exist_ok=True)
    objs = [os.path.join(obj_dir, os.path.splitext(os.path.basename(u))[0] + ".o") for u in units]

    def run(cmd):
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd, cwd=obj_dir)

    compile_flags = [f for f in HIPCC_FLAGS if f != "-shared"] + list(extra_flags)
    jobs = min(len(units), 16, os.cpu_count() or 1, int(os.environ.get("MAX_JOBS") or 16))
    with ThreadPoolExecutor(max(jobs, 1)) as pool:
        list(pool.map(run, [["hipcc"] + compile_flags + ["-c", "-o", o, u] for u, o in zip(units, objs)]))
    run(["hipcc"] + HIPCC_FLAGS + ["-o", out] + objs)
    return out


HOST_DRIVER = os.path.join(_ROOT, "tests", "cpp", "host_driver")
LFNET_DESC_DRIVER = os.path.join(_ROOT, "tests", "cpp", "liblfnet_desc_driver.so")
LFNET_DET_DRIVER = os.path.join(_ROOT, "tests", "cpp", "liblfnet_det_driver.so")
VOS_NET_DRIVER = os.path.join(_ROOT, "tests", "cpp", "libvos_net_driver.so")


def build_driver(name: str, shared: bool = True, force: bool = False, verbose: bool = False) -> str:
    """Compile tests/cpp/<name>.cpp together with the C++ host layer (bundletrack_amd/cpp) against libbtba.so: the shared library
    tests/cpp/lib<name>.so, or with shared=False the program tests/cpp/<name>.  Rebuilt when older than a source, a header or the library."""
    cpp = os.path.join(_ROOT, "tests", "cpp")
    out = os.path.join(cpp, f"lib{name}.so" if shared else name)
    srcs = [os.path.join(cpp, name + ".cpp"), os.path.join(_PKG, "cpp", "btba_host.cpp")]
    deps = srcs + [os.path.join(_PKG, "cpp", "btba_host.hpp"), HEADER, LIB_PATH]
    if not force and os.path.exists(out) and os.path.getmtime(out) >= max(os.path.getmtime(d) for d in deps):
        return out
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include")]
    cmd += (["-fPIC", "-shared"] if shared else []) + ["-o", out] + srcs
    cmd += ["-L" + _PKG, "-lbtba", "-L" + os.path.join(rocm, "lib"), "-lamdhip64",
            "-Wl,-rpath," + _PKG, "-Wl,-rpath,$ORIGIN/../../bundletrack_amd", "-Wl,-rpath," + os.path.join(rocm, "lib")]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return out


def build_host_cpp(force: bool = False, verbose: bool = False) -> str:
    """Compile the C++ host layer's test program (tests/cpp/host_driver) and the three nets' ctypes drivers."""
    build_driver("lfnet_desc_driver", force=force, verbose=verbose)
    build_driver("lfnet_det_driver", force=force, verbose=verbose)
    build_driver("vos_net_driver", force=force, verbose=verbose)
    return build_driver("host_driver", shared=False, force=force, verbose=verbose)


_lib = None


def lib() -> C.CDLL:
    """Load libbtba.so; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        path = os.environ.get("BTBA_LIB_PATH", LIB_PATH)      # developer A/B of kernel builds; still no fallback
        if not os.path.exists(path):
            raise ImportError(
                f"{path} is missing: the HIP extension has not been built. "
                "Run `python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc). There is no CPU fallback.")
        # torch first: libbtba.so is linked against /opt/rocm's libamdhip64, torch brings its own copy under the same soname.  Whichever is
        # loaded first becomes THE HIP runtime of the process; with libbtba.so first, torch's kernels and ours meet a runtime torch was not
        # built for and the first launch fails with hipErrorNoDevice (seen with build() followed by smoke() in one process).
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(path)
        # the structs below mirror ONE version of include/btba.h: a library built from another one must not be called (btba.h: BTBA_VERSION)
        import re
        header_version = int(re.search(r"#define BTBA_VERSION (\d+)", open(HEADER).read()).group(1))
        if "BTBA_LIB_PATH" not in os.environ and L.btba_version() != header_version:
            raise ImportError(f"{path} is version {L.btba_version()}, include/btba.h is {header_version}: rebuild (python -c 'import __graft_entry__ as g; g.build()')")
        L.btba_strerror.restype = C.c_char_p
        L.btba_strerror.argtypes = [C.c_int]
        for name in EXPORTED_SYMBOLS:
            if "BTBA_LIB_PATH" in os.environ and name in ("btba_workspace_set_option", "btba_pack_correspondences24", "btba_workspace_live_blocks") and not hasattr(L, name):
                continue               # developer A/B against a build from before version 103
            getattr(L, name)           # AttributeError if the ABI and the header drift apart
        L.btba_workspace_create.argtypes = [C.POINTER(C.c_void_p), C.c_void_p]
        L.btba_workspace_create_on_stream.argtypes = [C.POINTER(C.c_void_p), C.c_void_p]
        L.btba_workspace_destroy.argtypes = [C.c_void_p]
        L.btba_workspace_destroy.restype = None
        L.btba_workspace_sync.argtypes = [C.c_void_p]
        if hasattr(L, "btba_workspace_set_option"):
            L.btba_workspace_set_option.argtypes = [C.c_void_p, C.c_int, C.c_int64]
        if hasattr(L, "btba_workspace_live_blocks"):
            L.btba_workspace_live_blocks.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        L.btba_workspace_wait_stream.argtypes = [C.c_void_p, C.c_void_p]
        L.btba_workspace_signal_stream.argtypes = [C.c_void_p, C.c_void_p]
        L.btba_collect_stats.argtypes = [C.c_void_p, C.POINTER(Stats)]
        L.btba_optimize_frames.argtypes = [
            C.c_void_p, C.POINTER(Params), C.c_int, C.c_int, C.c_int, C.c_void_p,
            C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(Stats)]
        L.btba_optimize_frames_keyed.argtypes = [
            C.c_void_p, C.POINTER(Params), C.c_int, C.c_int, C.c_int, C.c_void_p,
            C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(Stats)]
        L.btba_frame_cache_clear.argtypes = [C.c_void_p]
        L.btba_frame_cache_evict.argtypes = [C.c_void_p, C.c_uint64]
        L.btba_solve_cached.argtypes = [
            C.c_void_p, C.POINTER(Params), C.c_int, C.c_int, C.c_int, C.c_void_p,
            C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.btba_build_cache.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_float,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.btba_solve_batch.argtypes = [
            C.c_void_p, C.POINTER(Params), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
            C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.btba_trace_layout_get.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(TraceLayout)]
        L.btba_trace_layout_get.restype = None
        L.btba_bucket_correspondences.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p]
        L.btba_matrices_to_poses.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.btba_poses_to_matrices.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.btba_build_cache_zn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.btba_pack_zn.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.btba_solve_batch_zn.argtypes = [C.c_void_p, C.POINTER(Params), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_int64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.btba_zn_block_ranges.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        if hasattr(L, "btba_pack_correspondences24"):
            L.btba_pack_correspondences24.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        L.btba_zn_valid_lists.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.btba_solve_batch_zn_aux.argtypes = [C.c_void_p, C.POINTER(Params), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(ZnAux),
                                              C.c_void_p, C.c_int64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.btba_process_depth.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_int, C.c_float, C.c_float]
        L.btba_depth_to_normals.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.btba_ingest_params_default.argtypes = [C.POINTER(IngestParams)]
        L.btba_ingest_params_default.restype = None
        L.btba_ingest_frames.argtypes = [C.c_void_p, C.POINTER(IngestParams), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.btba_vos_params_default.argtypes = [C.POINTER(VosParams)]
        L.btba_vos_params_default.restype = None
        L.btba_vos_sample_frames.argtypes = [C.POINTER(VosParams), C.c_int, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.btba_vos_first_labels.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.btba_vos_propagate.argtypes = [C.c_void_p, C.POINTER(VosParams), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.btba_vos_masks.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.btba_vos_inputs.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.btba_lfnet_params_default.argtypes = [C.POINTER(LfnetParams)]
        L.btba_lfnet_params_default.restype = None
        L.btba_lfnet_heatmaps.argtypes = [C.c_void_p, C.POINTER(LfnetParams), C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 6
        L.btba_lfnet_select.argtypes = [C.c_void_p, C.POINTER(LfnetParams), C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 3
        L.btba_lfnet_crops.argtypes = [C.c_void_p, C.POINTER(LfnetParams), C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 10
        L.btba_lfnet_keypoints.argtypes = [C.c_void_p, C.POINTER(LfnetParams), C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 15
        L.btba_lfnet_desc_config_default.argtypes = [C.POINTER(LfnetDescConfig)]
        L.btba_lfnet_desc_config_default.restype = None
        L.btba_lfnet_desc_model_create.argtypes = [C.c_void_p, C.POINTER(LfnetDescConfig), C.POINTER(LfnetDescWeights), C.POINTER(C.c_void_p)]
        L.btba_lfnet_desc_model_destroy.argtypes = [C.c_void_p]
        L.btba_lfnet_desc_model_destroy.restype = None
        L.btba_lfnet_descriptors.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.btba_vos_net_config_default.argtypes = [C.POINTER(VosNetConfig)]
        L.btba_vos_net_config_default.restype = None
        L.btba_vos_net_layer_count.argtypes = [C.POINTER(VosNetConfig)]
        L.btba_vos_net_model_create.argtypes = [C.c_void_p, C.POINTER(VosNetConfig), C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
        L.btba_vos_net_model_destroy.argtypes = [C.c_void_p]
        L.btba_vos_net_model_destroy.restype = None
        L.btba_vos_net_out_size.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.btba_vos_features.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.btba_lfnet_det_config_default.argtypes = [C.POINTER(LfnetDetConfig)]
        L.btba_lfnet_det_config_default.restype = None
        L.btba_lfnet_det_scales.argtypes = [C.c_double, C.c_double, C.c_int, C.c_void_p]
        L.btba_lfnet_det_model_create.argtypes = [C.c_void_p, C.POINTER(LfnetDetConfig), C.POINTER(LfnetDetWeights), C.POINTER(C.c_void_p)]
        L.btba_lfnet_det_model_destroy.argtypes = [C.c_void_p]
        L.btba_lfnet_det_model_destroy.restype = None
        L.btba_lfnet_det_map_size.argtypes = [C.c_double, C.c_int]
        L.btba_lfnet_det_map_sizes.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.btba_lfnet_det_pad_size.argtypes = [C.c_void_p]
        L.btba_lfnet_scores.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.btba_match_params_default.argtypes = [C.POINTER(MatchParams)]
        L.btba_match_params_default.restype = None
        L.btba_match_capacity.argtypes = [C.POINTER(MatchParams), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int64)]
        L.btba_match_pairs.argtypes = [C.c_void_p, C.POINTER(MatchParams), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.btba_mask_params_default.argtypes = [C.POINTER(MaskParams)]
        L.btba_mask_params_default.restype = None
        L.btba_apply_masks.argtypes = [C.c_void_p, C.POINTER(MaskParams), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p]
        L.btba_detector_params_default.argtypes = [C.POINTER(DetectorParams)]
        L.btba_detector_params_default.restype = None
        L.btba_detector_transform.argtypes = [C.POINTER(DetectorParams), C.c_void_p, C.c_void_p, C.c_void_p]
        L.btba_detector_inputs.argtypes = [C.c_void_p, C.POINTER(DetectorParams), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p]
        L.btba_detector_keypoints_to_image.argtypes = [C.c_void_p, C.POINTER(DetectorParams), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                       C.c_void_p]
        L.btba_pose_errors.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p]
        L.btba_nocs_params_default.argtypes = [C.POINTER(NocsParams)]
        L.btba_nocs_params_default.restype = None
        L.btba_nocs_errors.argtypes = [C.c_void_p, C.POINTER(NocsParams), C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.btba_mappoints_create.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        L.btba_mappoints_destroy.argtypes = [C.c_void_p]
        L.btba_mappoints_destroy.restype = None
        L.btba_mappoints_register_frame.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int32)]
        L.btba_mappoints_forget_frame.argtypes = [C.c_void_p, C.c_int32]
        L.btba_mappoints_export.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.btba_corres_params_default.argtypes = [C.POINTER(CorresParams)]
        L.btba_corres_params_default.restype = None
        L.btba_corres_chain_capacity.argtypes = L.btba_match_capacity.argtypes
        L.btba_corres_chain.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(MatchParams), C.POINTER(CorresParams), C.c_int, C.c_int, C.c_int, C.c_int,
                                        C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.btba_window_layout.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_uint32),
                                         C.c_void_p, C.c_void_p, C.c_void_p]
        L.btba_marshal_windows.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_uint32, C.c_int64,
                                           C.c_void_p, C.c_void_p, C.c_void_p]
        L.btba_procrustes_pairs.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p]
        L.btba_linearize_batch_zn_aux.argtypes = [C.c_void_p, C.POINTER(Params), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(ZnAux),
                                                  C.c_void_p, C.c_int64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.btba_pose_covariances.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.btba_objective_batch_zn_aux.argtypes = [C.c_void_p, C.POINTER(Params), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(ZnAux),
                                                  C.c_void_p, C.c_int64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.btba_fuse_params_default.argtypes = [C.POINTER(FuseParams)]
        L.btba_fuse_params_default.restype = None
        L.btba_fuse_layout.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
        L.btba_fuse_bounds.argtypes = [C.c_void_p, C.POINTER(FuseParams), C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.btba_fuse_frames.argtypes = [C.c_void_p, C.POINTER(FuseParams), C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 8
        L.btba_voxel_downsample.argtypes = [C.c_void_p, C.POINTER(FuseParams), C.c_int] + [C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 8
        L.btba_register_params_default.argtypes = [C.POINTER(RegisterParams)]
        L.btba_register_params_default.restype = None
        L.btba_register_index.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.btba_register_frames.argtypes = [C.c_void_p, C.POINTER(RegisterParams), C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                           C.c_int] + [C.c_void_p] * 6
        L.btba_register_associate.argtypes = [C.c_void_p, C.POINTER(RegisterParams), C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                              C.c_int] + [C.c_void_p] * 4
        L.btba_keyframes_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.btba_keyframes_destroy.argtypes = [C.c_void_p]
        L.btba_keyframes_destroy.restype = None
        L.btba_keyframes_reset.argtypes = [C.c_void_p, C.c_int]
        L.btba_keyframes_check_add.argtypes = [C.c_void_p, C.c_float, C.c_int] + [C.c_void_p] * 7
        L.btba_keyframes_select.argtypes = [C.c_void_p] * 11
        L.btba_keyframes_writeback.argtypes = [C.c_void_p] * 5
        L.btba_keyframes_export.argtypes = [C.c_void_p] * 6
        L.btba_rotation_distances.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib = L
    return _lib


def check(status: int, where: str) -> None:
    if status != BTBA_OK:
        raise BtbaError(status, where)


def _params(cls, default_fn: str, kw: dict):
    """A `cls` filled by the library's `default_fn`, then fields overridden from kw (AttributeError on an unknown field)."""
    p = cls()
    getattr(lib(), default_fn)(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def default_params(**kw) -> Params:
    return _params(Params, "btba_params_default", kw)


def match_params(**kw) -> MatchParams:
    """btba_match_params_default with fields overridden by keyword."""
    return _params(MatchParams, "btba_match_params_default", kw)


def corres_params(**kw) -> CorresParams:
    """btba_corres_params_default with fields overridden by keyword."""
    return _params(CorresParams, "btba_corres_params_default", kw)


def mask_params(**kw) -> MaskParams:
    """btba_mask_params_default with fields overridden by keyword."""
    return _params(MaskParams, "btba_mask_params_default", kw)


def ingest_params(**kw) -> IngestParams:
    """btba_ingest_params_default with fields overridden by keyword."""
    return _params(IngestParams, "btba_ingest_params_default", kw)


def vos_params(**kw) -> VosParams:
    """btba_vos_params_default with fields overridden by keyword."""
    return _params(VosParams, "btba_vos_params_default", kw)


def vos_net_config(**kw) -> VosNetConfig:
    """btba_vos_net_config_default with fields overridden by keyword; layers: a sequence of four block counts."""
    layers = kw.pop("layers", None)
    p = _params(VosNetConfig, "btba_vos_net_config_default", kw)
    if layers is not None:
        layers = [int(v) for v in layers]
        if len(layers) != 4:
            raise ValueError("four block counts")
        for i in range(4):
            p.layers[i] = layers[i]
    return p


def lfnet_params(**kw) -> LfnetParams:
    """btba_lfnet_params_default with fields overridden by keyword."""
    return _params(LfnetParams, "btba_lfnet_params_default", kw)


def lfnet_desc_config(**kw) -> LfnetDescConfig:
    """btba_lfnet_desc_config_default with fields overridden by keyword."""
    return _params(LfnetDescConfig, "btba_lfnet_desc_config_default", kw)


def lfnet_det_config(**kw) -> LfnetDetConfig:
    """btba_lfnet_det_config_default with fields overridden by keyword; scale_factors: a sequence, which also sets num_scales."""
    sf = kw.pop("scale_factors", None)
    p = _params(LfnetDetConfig, "btba_lfnet_det_config_default", kw)
    if sf is not None:
        sf = [float(s) for s in sf]
        if not 1 <= len(sf) <= 16:
            raise ValueError("1 .. 16 scale factors")
        p.num_scales = len(sf)
        for i in range(16):
            p.scale_factors[i] = sf[i] if i < len(sf) else 0.0
    return p


def detector_params(**kw) -> DetectorParams:
    """btba_detector_params_default with fields overridden by keyword."""
    return _params(DetectorParams, "btba_detector_params_default", kw)


def nocs_params(**kw) -> NocsParams:
    """btba_nocs_params_default with fields overridden by keyword."""
    return _params(NocsParams, "btba_nocs_params_default", kw)


def fuse_params(**kw) -> FuseParams:
    """btba_fuse_params_default with fields overridden by keyword."""
    return _params(FuseParams, "btba_fuse_params_default", kw)


def register_params(**kw) -> RegisterParams:
    """btba_register_params_default with fields overridden by keyword."""
    return _params(RegisterParams, "btba_register_params_default", kw)


def declared_symbols() -> list[str]:
    """Function names declared in include/btba.h (used by the ABI test)."""
    import re
    txt = open(HEADER).read()
    return sorted(set(re.findall(r"^BTBA_API[^;]*?\b(btba_[a-z_0-9]+)\s*\(", txt, flags=re.M)))


def bucket_correspondences(corr: np.ndarray, n_frames: int):
    """Host helper: stable bucketing of EntryJ by canonical frame pair -> (sorted, offsets[P+1])."""
    corr = np.ascontiguousarray(corr, ENTRYJ_DTYPE)
    P = n_frames * (n_frames - 1) // 2
    out = np.zeros(max(corr.shape[0], 1), ENTRYJ_DTYPE)
    off = np.zeros(P + 1, np.uint32)
    check(lib().btba_bucket_correspondences(corr.ctypes.data, corr.shape[0], n_frames, out.ctypes.data, off.ctypes.data),
          "btba_bucket_correspondences")
    return out[: int(off[P])], off
