// Stage B of the keypoint head (btba_lfnet_select, include/btba.h) restated for the host compiler by the device's route, from the
// rules alone: peaks of the thresholded map, scores as order-preserving keys (the non-peaks one count at the key of zero), the k-th
// largest key over all positions, then every peak above it and the peaks equal to it while their rank among the equal positions is
// below what is left of k.  Reads from stdin: int32 H, W, top_k, crop_radius, nms_ksize, float nms_thresh, then H * W floats.
// Writes to stdout: int32 n, then n int32 pairs (x, y) in raster order.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>

static uint32_t key_of(float v)
{
    if (v == 0.0f) return 0x80000000u;
    uint32_t b;
    std::memcpy(&b, &v, 4);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

int main()
{
    int32_t hdr[5];
    float thresh;
    if (std::fread(hdr, 4, 5, stdin) != 5 || std::fread(&thresh, 4, 1, stdin) != 1) return 2;
    const int H = hdr[0], W = hdr[1], top_k = hdr[2], crop = hdr[3], hk = hdr[4] / 2, HW = H * W;
    std::vector<float> heat((size_t)HW);
    if (std::fread(heat.data(), 4, (size_t)HW, stdin) != (size_t)HW) return 2;
    auto works = [&](int y, int x) {
        if (y < 0 || y >= H || x < 0 || x >= W) return 0.0f;
        const float v = heat[(size_t)y * W + x];
        return v < thresh ? 0.0f : v;
    };
    std::vector<int32_t> idx;
    std::vector<uint32_t> key;
    for (int i = 0; i < HW; i++) {
        const int y = i / W, x = i % W;
        const float c = works(y, x);
        bool peak = true;
        for (int dy = -hk; dy <= hk && peak; dy++)
            for (int dx = -hk; dx <= hk; dx++)
                if ((dy || dx) && !(c > works(y + dy, x + dx))) { peak = false; break; }
        if (!peak) continue;
        const bool in_crop = y >= crop && y < H - crop && x >= crop && x < W - crop;
        idx.push_back(i);
        key.push_back(in_crop ? key_of(heat[(size_t)i]) : 0x80000000u);
    }
    const uint32_t U0 = 0x80000000u;
    const size_t k = (size_t)std::min(top_k, HW);
    std::vector<uint32_t> all(key);
    all.resize((size_t)HW, U0);                                       // the non-peaks score zero
    std::nth_element(all.begin(), all.begin() + (k - 1), all.end(), std::greater<uint32_t>());
    const uint32_t T = all[k - 1];
    size_t above = 0;
    for (uint32_t u : all) above += u > T;
    const long need = (long)(k - above);
    std::vector<int32_t> out;
    long before = 0;                                                  // nonzero peaks (T = zero's key) or peaks equal to T seen so far
    for (size_t j = 0; j < idx.size(); j++) {
        const uint32_t u = key[j];
        const long rank = T == U0 ? (long)idx[j] - before : before;
        if (u > T || (u == T && rank < need)) { out.push_back(idx[j] % W); out.push_back(idx[j] / W); }
        before += T == U0 ? u != U0 : u == T;
    }
    const int32_t n = (int32_t)(out.size() / 2);
    std::fwrite(&n, 4, 1, stdout);
    return std::fwrite(out.data(), 4, out.size(), stdout) == out.size() ? 0 : 1;
}
