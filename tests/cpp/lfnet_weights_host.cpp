// lfnet_weights_host.cpp -- the LF-Net weights layer (bundletrack_amd/csrc/btba_lfnet_weights.hpp) on the CPU, for a sanitizer build:
// reads cases from stdin, runs lfnet_conv_ok, lfnet_bn_ok and lfnet_fold on each, writes the verdicts and the (scale, shift) bits.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I include tests/cpp/lfnet_weights_host.cpp -o tests/cpp/lfnet_weights_host
// A case: "K N eps" then six presence flags in the order weights, biases, gamma, beta, moving_mean, moving_variance, then the present
// arrays in that order (K * N values for weights, N for the others).  Every float is the hexadecimal form of its 32 bits.
// Per case one line: "conv_ok bn_ok" and, where bn_ok, N scale words and N shift words.  Every array is a heap block of exactly its
// stated size, so a read past an end is the sanitizer's to report.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>

#include "../../bundletrack_amd/csrc/btba_lfnet_weights.hpp"

static bool read_float(float *out)
{
    unsigned int bits = 0;
    if (std::scanf("%x", &bits) != 1) return false;
    const uint32_t b = bits;
    std::memcpy(out, &b, sizeof(b));
    return true;
}

static uint32_t bits_of(float v)
{
    uint32_t b;
    std::memcpy(&b, &v, sizeof(b));
    return b;
}

int main()
{
    long K, N;
    while (std::scanf("%ld %ld", &K, &N) == 2) {
        float eps;
        int present[6];
        if (K < 1 || N < 1 || !read_float(&eps)) return 2;
        for (int &p : present)
            if (std::scanf("%d", &p) != 1) return 2;
        std::unique_ptr<float[]> arrays[6];
        for (int a = 0; a < 6; a++) {
            if (!present[a]) continue;
            const size_t n = a == 0 ? (size_t)K * N : (size_t)N;
            arrays[a].reset(new float[n]);
            for (size_t i = 0; i < n; i++)
                if (!read_float(&arrays[a][i])) return 2;
        }
        btba_lfnet_desc_layer l{};
        l.weights = arrays[0].get(); l.biases = arrays[1].get(); l.gamma = arrays[2].get(); l.beta = arrays[3].get();
        l.moving_mean = arrays[4].get(); l.moving_variance = arrays[5].get();
        const bool conv_ok = btba_host::lfnet_conv_ok(l, (size_t)K, (size_t)N), bn_ok = btba_host::lfnet_bn_ok(l, (size_t)N, eps);
        std::printf("%d %d", (int)conv_ok, (int)bn_ok);
        if (bn_ok) {
            std::unique_ptr<float[]> scale(new float[N]), shift(new float[N]);
            btba_host::lfnet_fold(l, l.biases, (int)N, eps, scale.get(), shift.get());
            for (long n = 0; n < N; n++) std::printf(" %08x", bits_of(scale[n]));
            for (long n = 0; n < N; n++) std::printf(" %08x", bits_of(shift[n]));
        }
        std::printf("\n");
    }
    return 0;
}
