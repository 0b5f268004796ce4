// btba_api_vos_net.hip -- host side of libbtba.so: the VOS backbone, ResNet frames to features.
#include "btba_host_common.hpp"
#include "btba_vos_net_plan.hpp"
#include "btba_vos_net.hpp"

struct btba_vos_net_model : LfnetModelBase {
    btba_vos_net_config cfg{};
    VosNetPlan plan;
};

extern "C" {

void btba_vos_net_config_default(btba_vos_net_config *c)
{
    if (!c) return;
    std::memset(c, 0, sizeof(*c));
    c->block = BTBA_VOS_NET_BOTTLENECK;                                   // run_video.py's default: resnet50
    c->layers[0] = 3; c->layers[1] = 4; c->layers[2] = 6; c->layers[3] = 3;
    c->bn_eps = 1e-5f;                                                    // nn.BatchNorm2d's default
}

int btba_vos_net_layer_count(const btba_vos_net_config *cfg) { return vos_net_layer_count(cfg); }

int btba_vos_net_out_size(int H, int W, int32_t *Hd, int32_t *Wd)
{
    if (!Hd || !Wd || H < 1 || W < 1 || H > BTBA_VOS_NET_MAX_SIZE || W > BTBA_VOS_NET_MAX_SIZE) return BTBA_EINVAL;
    *Hd = vos_net_out_size(H); *Wd = vos_net_out_size(W);
    return BTBA_OK;
}

int btba_vos_net_model_create(btba_workspace *ws, const btba_vos_net_config *cfg, const btba_vos_net_layer *layers, int n_layers,
                              btba_vos_net_model **out)
{
    if (out) *out = nullptr;
    if (!ws || !layers || !out || !vos_net_config_ok(cfg)) return BTBA_EINVAL;
    std::unique_ptr<btba_vos_net_model> M(new (std::nothrow) btba_vos_net_model());
    if (!M) return BTBA_ENOMEM;
    M->ws = ws; M->device = ws->device; M->cfg = *cfg;
    LfnetArena A;
    M->plan = vos_net_plan(*cfg, A);
    if (n_layers != M->plan.n_layers) return BTBA_EINVAL;
    const float eps = cfg->bn_eps;
    if (!vos_net_layer_ok(layers[M->plan.stem.layer], M->plan.stem, eps)) return BTBA_EINVAL;
    for (const VosNetConv &c : M->plan.convs)
        if (!vos_net_layer_ok(layers[c.layer], c, eps)) return BTBA_EINVAL;
    // every argument has been checked; the first HIP call follows
    A.fill();
    vos_net_put(A, M->plan.stem, layers[M->plan.stem.layer], eps);
    for (const VosNetConv &c : M->plan.convs) vos_net_put(A, c, layers[c.layer], eps);
    DeviceGuard device_guard(ws);
    if (int rc = M->upload(A)) return rc;
    *out = M.release();
    return BTBA_OK;
}

void btba_vos_net_model_destroy(btba_vos_net_model *M) { destroy_on_device(M); }

int btba_vos_features(btba_workspace *ws, const btba_vos_net_model *M, int n_frames, int H, int W, const float *rgb_dev, float *features_out_dev)
{
    if (!ws || !M || n_frames < 0 || M->ws != ws) return BTBA_EINVAL;
    if (H < 1 || W < 1 || H > BTBA_VOS_NET_MAX_SIZE || W > BTBA_VOS_NET_MAX_SIZE) return BTBA_EINVAL;
    if (n_frames == 0) return BTBA_OK;
    if (!rgb_dev || !features_out_dev || misaligned(rgb_dev, 16) || misaligned(features_out_dev, 16)) return BTBA_EINVAL;
    DeviceGuard device_guard(ws);
    VosNetPlan P = M->plan;
    vos_net_plan_sizes(P, H, W);
    const int64_t frame_px = (int64_t)H * W;
    const int per_pass = (int)std::min<int64_t>(n_frames, std::max<int64_t>(1, BTBA_VOS_NET_PASS_PIXELS / frame_px));
    Scratch sc;
    Scratch::Region<float> regions[kVosNetBuffers] = { sc.add<float>((size_t)per_pass * P.buffer_floats), sc.add<float>((size_t)per_pass * P.buffer_floats),
                                                       sc.add<float>((size_t)per_pass * P.buffer_floats), sc.add<float>((size_t)per_pass * P.buffer_floats) };
    if (int rc = sc.bind(ws->vos_net)) return rc;
    const float *Wd = M->dev.as<float>();
    const size_t out_frame = (size_t)kVosNetOutC * P.Hd * P.Wd;
    for (int f0 = 0; f0 < n_frames; f0 += per_pass) {
        const int nf = std::min(per_pass, n_frames - f0);
        float *buf[kVosNetBuffers + 1] = { regions[0], regions[1], regions[2], regions[3], features_out_dev + (size_t)f0 * out_frame };
        {
            VosStem G{};
            G.rgb = rgb_dev + (size_t)f0 * 3 * frame_px; G.w = Wd + P.stem.w; G.scale = Wd + P.stem.scale; G.shift = Wd + P.stem.shift;
            G.out = buf[kVosNetA]; G.H = H; G.W = W; G.Ho = P.H1; G.Wo = P.W1; G.threads = (long long)nf * P.H1 * P.W1 * 16;
            k_vos_stem<<<(unsigned)((G.threads + 255) / 256), 256, 0, ws->stream>>>(G);
            HIP_TRY(hipGetLastError());
        }
        {
            VosPool G{};
            G.in = buf[kVosNetA]; G.out = buf[kVosNetX]; G.Hi = P.H1; G.Wi = P.W1; G.Ho = P.H2; G.Wo = P.W2;
            G.threads = (long long)nf * P.H2 * P.W2 * 16;
            k_vos_pool<<<(unsigned)((G.threads + 255) / 256), 256, 0, ws->stream>>>(G);
            HIP_TRY(hipGetLastError());
        }
        for (const VosNetConv &c : P.convs) {
            VosConv G{};
            G.in = buf[c.src]; G.w = Wd + c.w; G.scale = Wd + c.scale; G.shift = Wd + c.shift; G.res = c.res >= 0 ? buf[c.res] : nullptr;
            G.out = buf[c.dst]; G.M = nf * c.Ho * c.Wo; G.N = c.cout; G.K = c.ks * c.ks * c.cin; G.Hi = c.Hi; G.Wi = c.Wi; G.Cin = c.cin;
            G.Ho = c.Ho; G.Wo = c.Wo; G.ks = c.ks; G.stride = c.stride; G.pad = c.pad; G.relu = c.relu; G.nchw = c.dst == kVosNetOut;
            k_vos_conv<<<dim3((unsigned)((G.M + kVosBM - 1) / kVosBM), (unsigned)(G.N / kVosBN)), 256, 0, ws->stream>>>(G);
            HIP_TRY(hipGetLastError());
        }
    }
    return BTBA_OK;
}

}  // extern "C"
