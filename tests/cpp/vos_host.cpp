// vos_host.cpp -- stand-alone program (tests/test_vos_ref.py): the C++ host layer's vosSampleFrames, which needs no GPU, printed for
// frame_idx 1 .. n_frames as one line per frame: "frame_idx n_dense idx0 idx1 ...".
//   vos_host <ref_num> <range> <n_frames>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../bundletrack_amd/cpp/btba_host.hpp"

int main(int argc, char **argv)
{
    if (argc != 4) { std::fprintf(stderr, "usage: vos_host <ref_num> <range> <n_frames>\n"); return 2; }
    btba_vos_params p = btba::vosParams();
    p.ref_num = std::atoi(argv[1]);
    p.range = std::atoi(argv[2]);
    const int n_frames = std::atoi(argv[3]);
    try {
        for (int f = 1; f <= n_frames; f++) {
            std::vector<int> idx;
            int n_dense = 0;
            btba::vosSampleFrames(p, f, idx, n_dense);
            std::printf("%d %d", f, n_dense);
            for (int i : idx) std::printf(" %d", i);
            std::printf("\n");
        }
    } catch (const btba::Error &e) {
        std::fprintf(stderr, "vos_host: %s\n", e.what());
        return 1;
    }
    return 0;
}
