// vos_net_host.cpp -- the segmentation backbone's host-side plan and weight re-layout (bundletrack_amd/csrc/btba_vos_net_plan.hpp) on
// the CPU, for a sanitizer build: reads commands from stdin and writes what the plan says.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I include tests/cpp/vos_net_host.cpp -o tests/cpp/vos_net_host
// "P block l0 l1 l2 l3 eps H W": the plan of a configuration for H x W frames.  One line "ok n_layers arena_floats buffer_floats Hd Wd
//     macs" (ok 0: the configuration is refused, nothing else follows), then one line per convolution in the order it runs, the stem
//     first: "layer ks stride pad cin cout src dst res relu Hi Wi Ho Wo w scale shift".
// "L cout cin ks eps" then five presence flags (weight, bn_weight, bn_bias, running_mean, running_var) and the present arrays in that
//     order: one record through vos_net_layer_ok and vos_net_put.  One line: "ok" and, where ok, the K * cout words of the re-laid
//     weight, cout scale words and cout shift words.  Every float is the hexadecimal form of its 32 bits; every array is a heap block
//     of exactly its stated size, so a read past an end is the sanitizer's to report.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>

#include "../../bundletrack_amd/csrc/btba_vos_net_plan.hpp"

using namespace btba_host;

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

static void print_conv(const VosNetConv &c)
{
    std::printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %zu %zu %zu\n", c.layer, c.ks, c.stride, c.pad, c.cin, c.cout, c.src, c.dst, c.res,
                c.relu, c.Hi, c.Wi, c.Ho, c.Wo, c.w, c.scale, c.shift);
}

int main()
{
    char cmd[8];
    while (std::scanf("%7s", cmd) == 1) {
        if (cmd[0] == 'P') {
            btba_vos_net_config cfg{};
            int H, W;
            if (std::scanf("%d %d %d %d %d", &cfg.block, &cfg.layers[0], &cfg.layers[1], &cfg.layers[2], &cfg.layers[3]) != 5) return 2;
            if (!read_float(&cfg.bn_eps) || std::scanf("%d %d", &H, &W) != 2) return 2;
            const int count = vos_net_layer_count(&cfg);
            if (count < 0) { std::printf("0\n"); continue; }
            LfnetArena arena;
            VosNetPlan P = vos_net_plan(cfg, arena);
            vos_net_plan_sizes(P, H, W);
            if (P.n_layers != count || vos_net_out_size(H) != P.Hd || vos_net_out_size(W) != P.Wd) return 3;
            std::printf("1 %d %zu %zu %d %d %.17g\n", P.n_layers, arena.total, P.buffer_floats, P.Hd, P.Wd, P.macs);
            print_conv(P.stem);
            for (const VosNetConv &c : P.convs) print_conv(c);
        } else if (cmd[0] == 'L') {
            VosNetConv c;
            float eps;
            int present[5];
            if (std::scanf("%d %d %d", &c.cout, &c.cin, &c.ks) != 3 || c.cout < 1 || c.cin < 1 || c.ks < 1 || !read_float(&eps)) return 2;
            for (int &p : present)
                if (std::scanf("%d", &p) != 1) return 2;
            const size_t K = (size_t)c.ks * c.ks * c.cin, N = (size_t)c.cout;
            std::unique_ptr<float[]> arrays[5];
            for (int a = 0; a < 5; a++) {
                if (!present[a]) continue;
                const size_t n = a == 0 ? K * N : N;
                arrays[a].reset(new float[n]);
                for (size_t i = 0; i < n; i++)
                    if (!read_float(&arrays[a][i])) return 2;
            }
            const btba_vos_net_layer l{ arrays[0].get(), arrays[1].get(), arrays[2].get(), arrays[3].get(), arrays[4].get() };
            const bool ok = vos_net_layer_ok(l, c, eps);
            std::printf("%d", (int)ok);
            if (ok) {
                LfnetArena arena;
                c.w = arena.take(K * N); c.scale = arena.take(N); c.shift = arena.take(N);
                arena.fill();
                vos_net_put(arena, c, l, eps);
                for (size_t i = 0; i < K * N; i++) std::printf(" %08x", bits_of(arena.at(c.w)[i]));
                for (size_t n = 0; n < N; n++) std::printf(" %08x", bits_of(arena.at(c.scale)[n]));
                for (size_t n = 0; n < N; n++) std::printf(" %08x", bits_of(arena.at(c.shift)[n]));
            }
            std::printf("\n");
        } else {
            return 2;
        }
    }
    return 0;
}
