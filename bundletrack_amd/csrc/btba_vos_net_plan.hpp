// btba_vos_net_plan.hpp -- the VOS backbone (btba_vos_net_*, btba_vos_features; include/btba.h) as a list of convolutions: what
// btba_vos_net_model_create lays the weights out by and what btba_vos_features launches.  From a configuration: every convolution's
// shape, stride, buffers, epilogue and arena offsets, in the order they RUN; from (H, W): every convolution's image sizes and the
// scratch a frame needs.  Internal, and free of HIP: only btba.h, btba_lfnet_weights.hpp and the standard library.
//   ResNet, _make_layer, Bottleneck, BasicBlock   transductive-vos.pytorch/modeling/backbone/resnet.py:23-134
//   VOSNet                                        transductive-vos.pytorch/modeling/network.py:7-50
#pragma once
#include <cstdint>
#include <vector>

#include "btba_lfnet_weights.hpp"

namespace btba_host __attribute__((visibility("hidden"))) {

constexpr int kVosNetBasic = 0, kVosNetBottleneck = 1;
constexpr int kVosNetStemK = 7, kVosNetStemC = 64, kVosNetOutC = 256;
constexpr int kVosNetPlanes[4] = { 64, 128, 256, 256 }, kVosNetStride[4] = { 1, 2, 1, 1 };      // resnet.py:104-107
// the activation buffers of a pass, NHWC: X the residual stream, A and B a block's inner outputs, R the downsampled shortcut;
// kVosNetOut is the caller's NCHW features
constexpr int kVosNetX = 0, kVosNetA = 1, kVosNetB = 2, kVosNetR = 3, kVosNetOut = 4, kVosNetBuffers = 4;

struct VosNetConv {
    int layer = 0;                               // index into the caller's records (the forward order of include/btba.h)
    int ks = 1, stride = 1, pad = 0, cin = 0, cout = 0;
    int src = 0, dst = 0, res = -1;              // buffers; res -1: no residual
    int relu = 0;
    size_t w = 0, scale = 0, shift = 0;          // offsets in floats into the arena: [ks * ks * cin][cout], [cout], [cout]
    int Hi = 0, Wi = 0, Ho = 0, Wo = 0;          // vos_net_plan_sizes
};

struct VosNetPlan {
    VosNetConv stem;                             // 7 x 7, stride 2, pad 3, 3 -> 64 from the planar input into A; the max pool takes A to X
    std::vector<VosNetConv> convs;               // everything behind the pool, in the order it runs
    int n_layers = 0;
    int H = 0, W = 0, H1 = 0, W1 = 0, H2 = 0, W2 = 0, Hd = 0, Wd = 0;   // input, behind the stem, behind the pool, features
    size_t buffer_floats = 0;                    // one frame's share of each of the four buffers
    double macs = 0.0;                           // multiply-adds of one frame, stem included
};

inline bool vos_net_config_ok(const btba_vos_net_config *c)
{
    if (!c || (c->block != kVosNetBasic && c->block != kVosNetBottleneck)) return false;
    for (int s = 0; s < 4; s++)
        if (c->layers[s] < 1 || c->layers[s] > BTBA_VOS_NET_MAX_BLOCKS) return false;
    return std::isfinite(c->bn_eps) && c->bn_eps >= 0.0f;
}

inline int vos_net_conv_out(int in, int ks, int stride) { return (in + 2 * (ks / 2) - ks) / stride + 1; }

// ceil(size / 8): three halvings, each ceil (stem, pool, layer2)
inline int vos_net_out_size(int size) { return (size + 7) / 8; }

// The structure and the arena offsets of a checked configuration.  `arena` has had every region taken when this returns.
inline VosNetPlan vos_net_plan(const btba_vos_net_config &cfg, LfnetArena &arena)
{
    VosNetPlan P;
    int layer = 0;
    auto conv = [&](int ks, int stride, int cin, int cout, int src, int dst, int res, int relu) {
        VosNetConv c;
        c.layer = layer++;
        c.ks = ks; c.stride = stride; c.pad = ks / 2; c.cin = cin; c.cout = cout; c.src = src; c.dst = dst; c.res = res; c.relu = relu;
        c.w = arena.take((size_t)ks * ks * cin * cout); c.scale = arena.take((size_t)cout); c.shift = arena.take((size_t)cout);
        return c;
    };
    P.stem = conv(kVosNetStemK, 2, 3, kVosNetStemC, -1, kVosNetA, -1, 1);
    const bool bott = cfg.block == kVosNetBottleneck;
    const int expansion = bott ? 4 : 1;
    int inplanes = kVosNetStemC;
    for (int s = 0; s < 4; s++) {
        const int planes = kVosNetPlanes[s], out_c = planes * expansion;
        for (int b = 0; b < cfg.layers[s]; b++) {
            const int stride = b == 0 ? kVosNetStride[s] : 1;
            const bool down = b == 0 && (stride != 1 || inplanes != out_c);             // resnet.py:121
            const int res = down ? kVosNetR : kVosNetX;
            const bool last = !bott && s == 3 && b == cfg.layers[3] - 1;                // a basic net ends in its last block
            if (bott) {
                VosNetConv c1 = conv(1, 1, inplanes, planes, kVosNetX, kVosNetA, -1, 1);
                VosNetConv c2 = conv(3, stride, planes, planes, kVosNetA, kVosNetB, -1, 1);
                VosNetConv c3 = conv(1, 1, planes, out_c, kVosNetB, kVosNetX, res, 1);    // in place where the shortcut is X itself
                P.convs.push_back(c1); P.convs.push_back(c2);
                if (down) P.convs.push_back(conv(1, stride, inplanes, out_c, kVosNetX, kVosNetR, -1, 0));
                P.convs.push_back(c3);
            } else {
                VosNetConv c1 = conv(3, stride, inplanes, planes, kVosNetX, kVosNetA, -1, 1);
                VosNetConv c2 = conv(3, 1, planes, planes, kVosNetA, last ? kVosNetOut : kVosNetX, res, 1);
                P.convs.push_back(c1);
                if (down) P.convs.push_back(conv(1, stride, inplanes, out_c, kVosNetX, kVosNetR, -1, 0));
                P.convs.push_back(c2);
            }
            inplanes = out_c;
        }
    }
    if (bott) P.convs.push_back(conv(1, 1, inplanes, kVosNetOutC, kVosNetX, kVosNetOut, -1, 0));   // adjust_dim + bn256, no relu
    P.n_layers = layer;
    return P;
}

inline int vos_net_layer_count(const btba_vos_net_config *cfg)
{
    if (!vos_net_config_ok(cfg)) return -1;
    LfnetArena a;
    return vos_net_plan(*cfg, a).n_layers;
}

// Every convolution's image sizes for H x W frames, the scratch of one frame and its multiply-adds.
inline void vos_net_plan_sizes(VosNetPlan &P, int H, int W)
{
    P.H = H; P.W = W;
    P.H1 = vos_net_conv_out(H, 7, 2); P.W1 = vos_net_conv_out(W, 7, 2);
    P.H2 = vos_net_conv_out(P.H1, 3, 2); P.W2 = vos_net_conv_out(P.W1, 3, 2);           // the pool: 3 x 3, stride 2, pad 1
    P.stem.Hi = H; P.stem.Wi = W; P.stem.Ho = P.H1; P.stem.Wo = P.W1;
    P.buffer_floats = (size_t)P.H1 * P.W1 * kVosNetStemC;
    P.macs = (double)P.H1 * P.W1 * kVosNetStemC * (kVosNetStemK * kVosNetStemK * 3);
    int h[kVosNetBuffers + 1] = {}, w[kVosNetBuffers + 1] = {};
    h[kVosNetX] = P.H2; w[kVosNetX] = P.W2;
    for (VosNetConv &c : P.convs) {
        c.Hi = h[c.src]; c.Wi = w[c.src];
        c.Ho = vos_net_conv_out(c.Hi, c.ks, c.stride); c.Wo = vos_net_conv_out(c.Wi, c.ks, c.stride);
        h[c.dst] = c.Ho; w[c.dst] = c.Wo;
        const size_t out = (size_t)c.Ho * c.Wo * c.cout;
        if (c.dst != kVosNetOut && out > P.buffer_floats) P.buffer_floats = out;
        P.macs += (double)out * c.ks * c.ks * c.cin;
    }
    P.Hd = h[kVosNetOut]; P.Wd = w[kVosNetOut];
}

// PyTorch's [C_out][C_in][k][k] to the kernels' [K][N]: K = (ky, kx, c_in) in that order, N = C_out.
inline void vos_net_relayout(const float *w, int cout, int cin, int ks, float *out)
{
    for (int o = 0; o < cout; o++)
        for (int c = 0; c < cin; c++)
            for (int t = 0; t < ks * ks; t++)
                out[((size_t)t * cin + c) * cout + o] = w[((size_t)o * cin + c) * ks * ks + t];
}

// one record: all five arrays present, finite, running_var + eps > 0
inline bool vos_net_layer_ok(const btba_vos_net_layer &l, const VosNetConv &c, float eps)
{
    if (!l.weight || !l.bn_weight || !l.bn_bias || !l.running_mean || !l.running_var) return false;
    const btba_lfnet_desc_layer bn{ l.weight, nullptr, l.bn_weight, l.bn_bias, l.running_mean, l.running_var };
    return lfnet_all_finite(l.weight, (size_t)c.ks * c.ks * c.cin * c.cout) && lfnet_bn_ok(bn, (size_t)c.cout, eps);
}

// a record into the filled arena: the weight re-laid, the batch norm folded into (scale, shift) in fp64, rounded once
inline void vos_net_put(LfnetArena &arena, const VosNetConv &c, const btba_vos_net_layer &l, float eps)
{
    vos_net_relayout(l.weight, c.cout, c.cin, c.ks, arena.at(c.w));
    const btba_lfnet_desc_layer bn{ nullptr, nullptr, l.bn_weight, l.bn_bias, l.running_mean, l.running_var };
    lfnet_fold(bn, nullptr, c.cout, eps, arena.at(c.scale), arena.at(c.shift));
}

}  // namespace btba_host
