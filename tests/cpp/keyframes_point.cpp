// keyframes_point.cpp -- the keyframe memory's distance functions (bundletrack_amd/csrc/btba_keyframes_point.hpp) under the host compiler, for a
// sanitizer build (tests/test_keyframes_layout.py): prints, for a fixed argument list, the bits of keyframes_acosf and keyframes_degrees, and for
// fixed pose pairs the bits of keyframes_tmp; the test compares them with the numpy restatement's (tests/keyframes_ref.py).
//   a <argument> <keyframes_acosf> <keyframes_degrees of it>
//   t <16 floats of A> <16 floats of B> <keyframes_tmp>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../bundletrack_amd/csrc/btba_keyframes_point.hpp"

static uint32_t bits(float f)
{
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

int main()
{
    using namespace btba;
    std::vector<float> args = { 1.0f, -1.0f, 0.0f, -0.0f };
    float up1 = 1.0f, dn1 = -1.0f, p0 = 0.0f, m0 = -0.0f, mid = 0.5f;
    for (int k = 0; k < 64; k++) {                                   // the 64 neighbours of 1, -1, 0 from either side, and of 0.5
        up1 = std::nextafterf(up1, 0.0f); dn1 = std::nextafterf(dn1, 0.0f); p0 = std::nextafterf(p0, 1.0f); m0 = std::nextafterf(m0, -1.0f);
        mid = std::nextafterf(mid, 1.0f);
        args.insert(args.end(), { up1, dn1, p0, m0, mid });
    }
    for (int k = 0; k <= 2048; k++) args.push_back(-1.0f + (float)k / 1024.0f);
    uint32_t lcg = 12345u;
    auto next = [&]() { lcg = lcg * 1664525u + 1013904223u; return (float)(lcg >> 8) / 8388608.0f - 1.0f; };      // [-1, 1)
    for (int k = 0; k < 4096; k++) args.push_back(next());
    for (float t : args) {
        const float d = keyframes_acosf(t);
        std::printf("a %08x %08x %08x\n", bits(t), bits(d), bits(keyframes_degrees(d)));
    }
    for (int k = 0; k < 512; k++) {
        float A[16], B[16];
        for (int e = 0; e < 16; e++) { A[e] = next(); B[e] = k % 4 == 0 ? A[e] : next() * (k % 4 == 1 ? 1e-20f : 1.0f); }
        std::printf("t");
        for (int e = 0; e < 16; e++) std::printf(" %08x", bits(A[e]));
        for (int e = 0; e < 16; e++) std::printf(" %08x", bits(B[e]));
        std::printf(" %08x\n", bits(keyframes_tmp(A, B)));
    }
    return 0;
}
