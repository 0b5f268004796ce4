// btba_probe.hip -- test-only device probe of the product's small device functions (tests/test_gpu_device_math.py).
//
// It includes the product headers unchanged and is compiled with the flags of libbtba.so (bundletrack_amd/_lib.py: HIPCC_FLAGS),
// so every function below runs exactly as the kernels run it.  Nothing is restated here: each kernel calls one product function
// per element (one wave per case for the reductions, sixteen lanes per matrix for the solve kernels' inverse).
//
// Every launcher takes device pointers (torch tensors on cuda:0), launches, synchronises and returns the hipError_t.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../bundletrack_amd/csrc/btba_device.hpp"
#include "../../bundletrack_amd/csrc/btba_solve_phases.hpp"
#include "../../bundletrack_amd/csrc/btba_svd3.hpp"

using namespace btba;

#define PROBE_API extern "C" __attribute__((visibility("default")))

namespace {

constexpr int kProbeBlock = 256;
inline unsigned n_blocks(int64_t n) { return (unsigned)((n + kProbeBlock - 1) / kProbeBlock); }
inline int finish() { hipError_t e = hipGetLastError(); if (e != hipSuccess) return (int)e; return (int)hipDeviceSynchronize(); }
__device__ __forceinline__ int64_t gid() { return (int64_t)blockIdx.x * blockDim.x + threadIdx.x; }

// ---- SE(3) --------------------------------------------------------------------------------------------------------
template <bool F> __global__ void k_pose_to_matrix(const float *x, float *M, int n)
{
    const int64_t i = gid();
    if (i >= n) return;
    const float rot[3] = { x[6 * i], x[6 * i + 1], x[6 * i + 2] }, trans[3] = { x[6 * i + 3], x[6 * i + 4], x[6 * i + 5] };
    const Mat4 o = pose_to_matrix<F>(rot, trans);
    for (int k = 0; k < 16; k++) M[16 * i + k] = o.m[k];
}

template <bool F> __global__ void k_matrix_to_pose(const float *M, float *x, int n)
{
    const int64_t i = gid();
    if (i >= n) return;
    Mat4 a;
    for (int k = 0; k < 16; k++) a.m[k] = M[16 * i + k];
    float rot[3], trans[3];
    matrix_to_pose<F>(a, rot, trans);
    for (int k = 0; k < 3; k++) { x[6 * i + k] = rot[k]; x[6 * i + 3 + k] = trans[k]; }
}

template <bool F> __global__ void k_exp_rotation(const float *w, float *R, int n)
{
    const int64_t i = gid();
    if (i >= n) return;
    const float v[3] = { w[3 * i], w[3 * i + 1], w[3 * i + 2] };
    float r[9];
    exp_rotation<F>(v, r);
    for (int k = 0; k < 9; k++) R[9 * i + k] = r[k];
}

template <bool F> __global__ void k_ln_rotation(const float *R, float *w, int n)
{
    const int64_t i = gid();
    if (i >= n) return;
    float r[9], o[3];
    for (int k = 0; k < 9; k++) r[k] = R[9 * i + k];
    ln_rotation<F>(r, o);
    for (int k = 0; k < 3; k++) w[3 * i + k] = o[k];
}

// d = (dW, dT) as the solver's delta record holds them per frame, x = (rot, trans), T = Exp(x) from an earlier launch (as the solve kernels
// find it): out = Log(Exp(dW, dT) Exp(x)) by their update_frame, which takes the delta as the PCG leaves it ([trans, rot]) and T from LDS
template <bool F> __global__ void __launch_bounds__(kProbeBlock) k_update(const float *d, const float *x, const float *T, float *out, int n)
{
    __shared__ __attribute__((aligned(16))) float Tk[kProbeBlock][16];
    const int64_t i = gid();
    if (i >= n) return;
    for (int k = 0; k < 16; k++) Tk[threadIdx.x][k] = T[16 * i + k];
    const float dk[6] = { d[6 * i + 3], d[6 * i + 4], d[6 * i + 5], d[6 * i], d[6 * i + 1], d[6 * i + 2] };
    float rot[3] = { x[6 * i], x[6 * i + 1], x[6 * i + 2] }, trans[3] = { x[6 * i + 3], x[6 * i + 4], x[6 * i + 5] };
    update_frame<F>(true, dk, Tk[threadIdx.x], rot, trans);
    for (int k = 0; k < 3; k++) { out[6 * i + k] = rot[k]; out[6 * i + 3 + k] = trans[k]; }
}

// matrix c on lanes 16 c .. 16 c + 15: lane e writes entry e of its inverse
template <bool F> __global__ void __launch_bounds__(kProbeBlock) k_inverse16(const float *M, float *out, int n)
{
    __shared__ __attribute__((aligned(16))) float m[kProbeBlock];
    const int64_t i = gid(), last = 16 * (int64_t)n - 1;
    m[threadIdx.x] = M[i < last ? i : last];                  // (the groups behind the last matrix run along and store nothing)
    __syncthreads();
    const float v = inverse_on_sixteen_lanes<F>(m + (threadIdx.x & ~15u), threadIdx.x);
    if (i <= last) out[i] = v;
}

__global__ void k_mat_inverse(const float *M, float *out, int n)
{
    const int64_t i = gid();
    if (i >= n) return;
    Mat4 a;
    for (int k = 0; k < 16; k++) a.m[k] = M[16 * i + k];
    const Mat4 o = mat_inverse(a);
    for (int k = 0; k < 16; k++) out[16 * i + k] = o.m[k];
}

__global__ void k_huber(const float *e, const float *delta, float *out, int n)
{
    const int64_t i = gid();
    if (i < n) out[i] = huber_weight(e[i], delta[i]);
}

template <bool F> __global__ void k_div(const float *a, const float *b, float *out, int n)
{
    const int64_t i = gid();
    if (i < n) out[i] = se3_div<F>(a[i], b[i]);
}

template <bool F> __global__ void k_sqrt(const float *x, float *out, int n)
{
    const int64_t i = gid();
    if (i < n) out[i] = se3_sqrt<F>(x[i]);
}

__global__ void k_sincos(const float *x, float *out, int n)      // out[4 i ..]: sincosf's sine, cosine, then sinf, cosf
{
    const int64_t i = gid();
    if (i >= n) return;
    float s, c;
    sincosf(x[i], &s, &c);
    out[4 * i] = s; out[4 * i + 1] = c; out[4 * i + 2] = sinf(x[i]); out[4 * i + 3] = cosf(x[i]);
}

// ---- sweeps that count on the device ------------------------------------------------------------------------------
// Inputs: every float whose bit pattern lies in [lo, lo + n), or xs[0 .. n) when xs is given.  stat[0] counts the inputs that fail the
// check, stat[1] holds the largest error seen (bits of a non-negative float: their unsigned order is the float order), bad[] the first
// n_bad failing inputs.
enum { SWEEP_SINCOS = 0, SWEEP_SQRT_SCALE_IEEE = 1, SWEEP_SQRT_SCALE_FAST = 2, SWEEP_RCP_ULP = 3, SWEEP_SQRT_ULP = 4 };

__device__ __forceinline__ double ulp_of(double y)       // the spacing of the floats at |y| (normal range)
{
    const float f = fabsf((float)y);
    return (double)f == 0.0 ? 0.0 : ldexp(1.0, ilogbf(f) - 23);
}

__global__ void k_sweep(int which, uint32_t lo, int64_t n, const float *xs, unsigned *stat, float *bad, int n_bad)
{
    const int64_t i = gid();
    if (i >= n) return;
    const float x = xs ? xs[i] : __uint_as_float(lo + (uint32_t)i);
    bool fail = false;
    float err = 0.0f;
    if (which == SWEEP_SINCOS) {
        float s, c;
        sincosf(x, &s, &c);
        fail = __float_as_uint(s) != __float_as_uint(sinf(x)) || __float_as_uint(c) != __float_as_uint(cosf(x));
    } else if (which == SWEEP_SQRT_SCALE_IEEE || which == SWEEP_SQRT_SCALE_FAST) {
        const float a = which == SWEEP_SQRT_SCALE_FAST ? se3_sqrt<true>(x * 0.25f) : se3_sqrt<false>(x * 0.25f);
        const float b = which == SWEEP_SQRT_SCALE_FAST ? se3_sqrt<true>(x) : se3_sqrt<false>(x);
        fail = __float_as_uint(a) != __float_as_uint(0.5f * b);
    } else if (which == SWEEP_RCP_ULP || which == SWEEP_SQRT_ULP) {
        const double exact = which == SWEEP_RCP_ULP ? 1.0 / (double)x : sqrt((double)x);
        const float got = which == SWEEP_RCP_ULP ? se3_div<true>(1.0f, x) : se3_sqrt<true>(x);
        err = (float)(fabs((double)got - exact) / ulp_of(exact));
        fail = !(err <= 1.0f);
    }
    if (err > 0.0f) atomicMax(stat + 1, __float_as_uint(err));
    if (fail) {
        const unsigned slot = atomicAdd(stat, 1u);
        if ((int)slot < n_bad) bad[slot] = x;
    }
}

// ---- 3x3 SVD ------------------------------------------------------------------------------------------------------
__global__ void k_rsqrt(int refined, const float *x, float *out, int n)
{
    const int64_t i = gid();
    if (i < n) out[i] = refined ? svd3::rsqrt_refined(x[i]) : svd3::rsqrt_rn(x[i]);
}

__global__ void k_svd(const float *A, float *U, float *s, float *V, int n)
{
    const int64_t i = gid();
    if (i >= n) return;
    float a[9], u[9], sg[3], v[9];
    for (int k = 0; k < 9; k++) a[k] = A[9 * i + k];
    svd3::svd(a, u, sg, v);
    for (int k = 0; k < 9; k++) { U[9 * i + k] = u[k]; V[9 * i + k] = v[k]; }
    for (int k = 0; k < 3; k++) s[3 * i + k] = sg[k];
}

// case i: points [off[i], off[i + 1]) of src / dst (float4, xyz used) -> pose16[16 i ..] (last row 0 0 0 1), ok[i]
__global__ void k_procrustes(const float4 *src, const float4 *dst, const int *off, float *pose16, int *ok, int n)
{
    const int64_t i = gid();
    if (i >= n) return;
    float P[12];
    const int b = off[i];
    ok[i] = svd3::procrustes_reference(src + b, dst + b, off[i + 1] - b, P) ? 1 : 0;
    for (int k = 0; k < 12; k++) pose16[16 * i + k] = P[k];
    pose16[16 * i + 12] = 0.0f; pose16[16 * i + 13] = 0.0f; pose16[16 * i + 14] = 0.0f; pose16[16 * i + 15] = 1.0f;
}

// ---- wave64 reductions: one wave (or one workgroup of four) per case ----------------------------------------------
// x[64 c + lane] -> lane63[64 c + lane] = wave_sum_to_lane63 in every lane, all[64 c + lane] = wave_sum_all
__global__ void __launch_bounds__(64) k_wave_sum(const float *x, float *lane63, float *all)
{
    const int64_t o = 64 * (int64_t)blockIdx.x + threadIdx.x;
    lane63[o] = wave_sum_to_lane63(x[o]);
    all[o] = wave_sum_all(x[o]);
}

// acc[c][k][lane] (NV values per lane) -> q[c][k][lane], k < NV / 4
template <int NV> __global__ void __launch_bounds__(64) k_wave_fold(const float *acc, float *q)
{
    const int64_t base = (int64_t)blockIdx.x * NV * 64;
    float a[NV], r[NV / 4];
#pragma unroll
    for (int k = 0; k < NV; k++) a[k] = acc[base + 64 * k + threadIdx.x];
    wave_fold_sums<NV>(a, r);
    const int64_t ob = (int64_t)blockIdx.x * (NV / 4) * 64;
#pragma unroll
    for (int k = 0; k < NV / 4; k++) q[ob + 64 * k + threadIdx.x] = r[k];
}

// acc[c][k][tid] (NV values per thread, 4 waves) -> out[c][0 .. NV)
template <int NV> __global__ void __launch_bounds__(256) k_block_reduce(const float *acc, float *out, int mode)
{
    __shared__ float lds[4 * NV];
    const int64_t base = (int64_t)blockIdx.x * NV * 256;
    float a[NV];
#pragma unroll
    for (int k = 0; k < NV; k++) a[k] = acc[base + 256 * k + threadIdx.x];
    block_reduce_store<NV, 4>(a, lds, out + (int64_t)blockIdx.x * NV, mode);
}

}  // namespace

// ---- launchers ----------------------------------------------------------------------------------------------------
#define PROBE_F(kernel, ...) do { if (fast) hipLaunchKernelGGL(kernel<true>, dim3(n_blocks(n)), dim3(kProbeBlock), 0, 0, __VA_ARGS__); \
                                  else hipLaunchKernelGGL(kernel<false>, dim3(n_blocks(n)), dim3(kProbeBlock), 0, 0, __VA_ARGS__); } while (0)

PROBE_API int probe_pose_to_matrix(int fast, const float *x, float *M, int n) { if (n <= 0) return 0; PROBE_F(k_pose_to_matrix, x, M, n); return finish(); }
PROBE_API int probe_matrix_to_pose(int fast, const float *M, float *x, int n) { if (n <= 0) return 0; PROBE_F(k_matrix_to_pose, M, x, n); return finish(); }
PROBE_API int probe_exp_rotation(int fast, const float *w, float *R, int n) { if (n <= 0) return 0; PROBE_F(k_exp_rotation, w, R, n); return finish(); }
PROBE_API int probe_ln_rotation(int fast, const float *R, float *w, int n) { if (n <= 0) return 0; PROBE_F(k_ln_rotation, R, w, n); return finish(); }
PROBE_API int probe_update(int fast, const float *d, const float *x, float *out, int n)
{
    if (n <= 0) return 0;
    float *T = nullptr;                                      // Exp(x), by a launch of its own
    hipError_t e = hipMalloc(&T, (size_t)n * 16 * sizeof(float));
    if (e != hipSuccess) return (int)e;
    PROBE_F(k_pose_to_matrix, x, T, n);
    PROBE_F(k_update, d, x, T, out, n);
    const int rc = finish();
    hipFree(T);
    return rc;
}
PROBE_API int probe_div(int fast, const float *a, const float *b, float *out, int n) { if (n <= 0) return 0; PROBE_F(k_div, a, b, out, n); return finish(); }
PROBE_API int probe_sqrt(int fast, const float *x, float *out, int n) { if (n <= 0) return 0; PROBE_F(k_sqrt, x, out, n); return finish(); }

PROBE_API int probe_inverse16(int fast, const float *M, float *out, int n_mat)
{
    if (n_mat <= 0) return 0;
    const int64_t n = 16 * (int64_t)n_mat;
    PROBE_F(k_inverse16, M, out, n_mat);
    return finish();
}

PROBE_API int probe_mat_inverse(const float *M, float *out, int n)
{
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_mat_inverse, dim3(n_blocks(n)), dim3(kProbeBlock), 0, 0, M, out, n);
    return finish();
}

PROBE_API int probe_huber_weight(const float *e, const float *delta, float *out, int n)
{
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_huber, dim3(n_blocks(n)), dim3(kProbeBlock), 0, 0, e, delta, out, n);
    return finish();
}

PROBE_API int probe_sincos(const float *x, float *out, int n)
{
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_sincos, dim3(n_blocks(n)), dim3(kProbeBlock), 0, 0, x, out, n);
    return finish();
}

// stat: unsigned[2] (zeroed by the caller), bad: float[n_bad]
PROBE_API int probe_sweep(int which, uint32_t lo_bits, int64_t n, const float *xs, unsigned *stat, float *bad, int n_bad)
{
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_sweep, dim3(n_blocks(n)), dim3(kProbeBlock), 0, 0, which, lo_bits, n, xs, stat, bad, n_bad);
    return finish();
}

PROBE_API int probe_rsqrt(int refined, const float *x, float *out, int n)
{
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_rsqrt, dim3(n_blocks(n)), dim3(kProbeBlock), 0, 0, refined, x, out, n);
    return finish();
}

PROBE_API int probe_svd(const float *A, float *U, float *s, float *V, int n)
{
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_svd, dim3(n_blocks(n)), dim3(kProbeBlock), 0, 0, A, U, s, V, n);
    return finish();
}

PROBE_API int probe_procrustes(const float *src4, const float *dst4, const int *off, float *pose16, int *ok, int n)
{
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_procrustes, dim3(n_blocks(n)), dim3(kProbeBlock), 0, 0, (const float4 *)src4, (const float4 *)dst4, off, pose16, ok, n);
    return finish();
}

PROBE_API int probe_wave_sum(const float *x, float *lane63, float *all, int n_cases)
{
    if (n_cases <= 0) return 0;
    hipLaunchKernelGGL(k_wave_sum, dim3(n_cases), dim3(64), 0, 0, x, lane63, all);
    return finish();
}

PROBE_API int probe_wave_fold(int nv, const float *acc, float *q, int n_cases)
{
    if (n_cases <= 0) return 0;
    switch (nv) {
    case 4: hipLaunchKernelGGL(k_wave_fold<4>, dim3(n_cases), dim3(64), 0, 0, acc, q); break;
    case 8: hipLaunchKernelGGL(k_wave_fold<8>, dim3(n_cases), dim3(64), 0, 0, acc, q); break;
    case 28: hipLaunchKernelGGL(k_wave_fold<28>, dim3(n_cases), dim3(64), 0, 0, acc, q); break;
    case 44: hipLaunchKernelGGL(k_wave_fold<44>, dim3(n_cases), dim3(64), 0, 0, acc, q); break;
    default: return (int)hipErrorInvalidValue;
    }
    return finish();
}

PROBE_API int probe_block_reduce(int nv, int mode, const float *acc, float *out, int n_cases)
{
    if (n_cases <= 0 || (mode != 0 && mode != 2)) return n_cases <= 0 ? 0 : (int)hipErrorInvalidValue;
    switch (nv) {
    case 28: hipLaunchKernelGGL(k_block_reduce<28>, dim3(n_cases), dim3(256), 0, 0, acc, out, mode); break;
    case 44: hipLaunchKernelGGL(k_block_reduce<44>, dim3(n_cases), dim3(256), 0, 0, acc, out, mode); break;
    default: return (int)hipErrorInvalidValue;
    }
    return finish();
}
