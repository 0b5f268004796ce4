// btba_keyframes_point.hpp -- the rotation distance of the keyframe memory (btba_keyframes.hpp): Utils::rotationGeodesicDistance
// (Utils.cpp:42-47) as three __host__ __device__ functions that give the same bits under the host compiler, in numpy
// (tests/keyframes_ref.py restates them) and on the device.  No HIP header: plain g++ compiles it (tests/cpp/keyframes_point.cpp).
//
//   keyframes_tmp      the oracle's float arithmetic up to the clamp, statement for statement (oracle/btba_oracle_keyframes.c:30-40)
//   keyframes_acosf    acos of a float in [-1, 1].  The C library's acosf is not correctly rounded and differs between libraries, so the memory
//                      defines its own: fp64 from IEEE-exact operations only (+ - * / sqrt), fixed coefficients, fixed order, ONE rounding to float.
//                          a = |t|,  u = sqrt((1 - a) / (1 + a)) in [0, 1]         (1 - a and 1 + a are exact in fp64 for a float a)
//                          four half-angle steps  u <- u / (1 + sqrt(1 + u u))       (atan u = 2 atan of the new u;  u <= tan(pi / 64) after them)
//                          atan u = u P(u u), P the odd Taylor series' nine terms 1 / (2 k + 1), Horner from the last (remainder < 2^-80)
//                          acos a = 32 atan u;  acos t = pi - acos a for t < 0      (t = -1: u = 0, the result is (float)pi)
//   keyframes_degrees  rot_diff * 180 / M_PI as Bundler.cpp:210 types it: float product, double division, stored as float
//
// Contraction is off in every function; the host side relies on the baseline x86-64 / aarch64 rule that a * b + c is two roundings unless
// the compiler is told otherwise (no -ffast-math, no -ffp-contract=fast with FMA hardware enabled: the builds here set neither).
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define BTBA_KEYFRAMES_HD __host__ __device__
#else
#define BTBA_KEYFRAMES_HD
#endif

namespace btba {

// A, B: row-major 4 x 4 poses; only the rotation blocks are read.
BTBA_KEYFRAMES_HD inline float keyframes_tmp(const float *A, const float *B)
{
#pragma clang fp contract(off)
    float trace = 0.0f;
    for (int i = 0; i < 3; i++) {
        float dot = A[4 * i + 0] * B[4 * i + 0];
        dot += A[4 * i + 1] * B[4 * i + 1];
        dot += A[4 * i + 2] * B[4 * i + 2];
        trace = (i == 0) ? dot : trace + dot;
    }
    float tmp = (float)((double)(trace - 1.0f) / 2.0);
    tmp = fmaxf(fminf(1.0f, tmp), -1.0f);
    return tmp;
}

BTBA_KEYFRAMES_HD inline float keyframes_acosf(float t)
{
#pragma clang fp contract(off)
    const double a = (double)fabsf(t);
    double u = sqrt((1.0 - a) / (1.0 + a));
    for (int k = 0; k < 4; k++) u = u / (1.0 + sqrt(1.0 + u * u));
    const double z = u * u;
    double p = 1.0 / 17.0;
    p = 1.0 / 15.0 - z * p;
    p = 1.0 / 13.0 - z * p;
    p = 1.0 / 11.0 - z * p;
    p = 1.0 / 9.0 - z * p;
    p = 1.0 / 7.0 - z * p;
    p = 1.0 / 5.0 - z * p;
    p = 1.0 / 3.0 - z * p;
    p = 1.0 - z * p;
    const double r = 32.0 * (u * p);
    return (float)(t < 0.0f ? 3.141592653589793 - r : r);
}

BTBA_KEYFRAMES_HD inline float keyframes_degrees(float d)
{
#pragma clang fp contract(off)
    return (float)((double)(d * 180.0f) / 3.141592653589793);
}

BTBA_KEYFRAMES_HD inline float keyframes_distance(const float *A, const float *B) { return keyframes_acosf(keyframes_tmp(A, B)); }

}  // namespace btba
