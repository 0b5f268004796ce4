"""Build and load tests/hip/libbtba_probe.so (tests/hip/btba_probe.hip): the product's device functions, one element per thread.

Staleness rule of the tests/cpp drivers: rebuilt when it is missing or older than its sources (the probe, the product headers it includes and
the flags in bundletrack_amd/_lib.py) and hipcc is on PATH; otherwise the existing file is used; neither possible is an error."""
import ctypes as C
import os
import shutil
import subprocess

from bundletrack_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hip", "btba_probe.hip")
SO = os.path.join(HERE, "hip", "libbtba_probe.so")
DEPS = [SRC] + [os.path.join(_lib.SRC_DIR, h) for h in ("btba_device.hpp", "btba_svd3.hpp", "btba_solve_phases.hpp", "btba_kernels.hpp", "btba_sweep_layout.hpp")] + [os.path.abspath(_lib.__file__)]

# name -> argument types (device pointers as c_void_p); every launcher returns the hipError_t
SIGNATURES = {
    "probe_pose_to_matrix": [C.c_int, C.c_void_p, C.c_void_p, C.c_int],
    "probe_matrix_to_pose": [C.c_int, C.c_void_p, C.c_void_p, C.c_int],
    "probe_exp_rotation": [C.c_int, C.c_void_p, C.c_void_p, C.c_int],
    "probe_ln_rotation": [C.c_int, C.c_void_p, C.c_void_p, C.c_int],
    "probe_update": [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int],
    "probe_div": [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int],
    "probe_sqrt": [C.c_int, C.c_void_p, C.c_void_p, C.c_int],
    "probe_mat_inverse": [C.c_void_p, C.c_void_p, C.c_int],
    "probe_inverse16": [C.c_int, C.c_void_p, C.c_void_p, C.c_int],
    "probe_huber_weight": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int],
    "probe_sincos": [C.c_void_p, C.c_void_p, C.c_int],
    "probe_sweep": [C.c_int, C.c_uint32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int],
    "probe_rsqrt": [C.c_int, C.c_void_p, C.c_void_p, C.c_int],
    "probe_svd": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int],
    "probe_procrustes": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int],
    "probe_wave_sum": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int],
    "probe_wave_fold": [C.c_int, C.c_void_p, C.c_void_p, C.c_int],
    "probe_block_reduce": [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int],
}
SWEEP_SINCOS, SWEEP_SQRT_SCALE_IEEE, SWEEP_SQRT_SCALE_FAST, SWEEP_RCP_ULP, SWEEP_SQRT_ULP = range(5)


def compile_probe(out: str) -> str:
    subprocess.check_call(["hipcc"] + _lib.HIPCC_FLAGS + ["-o", out, SRC])
    return out


def build() -> str:
    stale = not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(d) for d in DEPS)
    if stale and shutil.which("hipcc"):
        return compile_probe(SO)
    if not os.path.exists(SO):
        raise RuntimeError(f"{SO} is missing and hipcc is not on PATH to build it from {SRC}")
    return SO


def load(path: str = None) -> C.CDLL:
    # torch first, for the reason bundletrack_amd._lib.lib() gives: the first HIP runtime loaded is the process's
    import torch  # noqa: F401
    L = C.CDLL(path or build())
    for name, argtypes in SIGNATURES.items():
        f = getattr(L, name)
        f.argtypes = argtypes
        f.restype = C.c_int
    return L


SVD3_HOST_SO = os.path.join(HERE, "cpp", "libsvd3_host.so")


def svd3_host() -> C.CDLL:
    """The g++ build of btba_svd3.hpp (tests/cpp/svd3_host.cpp), rebuilt when stale like tests/test_oracle_ransac.py does."""
    src = os.path.join(HERE, "cpp", "svd3_host.cpp")
    hdr = os.path.join(_lib.SRC_DIR, "btba_svd3.hpp")
    if not os.path.exists(SVD3_HOST_SO) or os.path.getmtime(SVD3_HOST_SO) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-fvisibility=hidden", "-Wno-unknown-pragmas",
                               "-o", SVD3_HOST_SO, src])
    L = C.CDLL(SVD3_HOST_SO)
    for name in ("rsqrt_rn_host", "rsqrt_refined_host"):
        getattr(L, name).argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.svd3_batch_host.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.procrustes_batch_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    for name in ("rsqrt_rn_host", "rsqrt_refined_host", "svd3_batch_host", "procrustes_batch_host"):
        getattr(L, name).restype = None
    return L
