// btba_api_lfnet_det.hip -- host side of libbtba.so: LF-Net's detector net.
#include "btba_host_common.hpp"
#include "btba_lfnet_det.hpp"

namespace {
// (int)((float)size * (float)(1.0 / s) + 0.5f) with the product rounded before the add, as TensorFlow's two ops round it
int det_map_size(double s, int size)
{
    volatile float prod = (float)size * (float)(1.0 / s);
    return (int)(prod + 0.5f);
}

bool det_config_ok(const btba_lfnet_det_config *c)
{
    if (!c || c->channels < 16 || c->channels > 64 || c->channels % 16 || (c->ksize != 3 && c->ksize != 5)) return false;
    if (c->blocks < 1 || c->blocks > BTBA_LFNET_DET_MAX_BLOCKS || c->num_scales < 1 || c->num_scales > BTBA_LFNET_MAX_SCALES) return false;
    for (int j = 0; j < c->num_scales; j++)
        if (!std::isfinite(c->scale_factors[j]) || !(c->scale_factors[j] > 0.0)) return false;
    if (c->activation < 0 || c->activation > 1 || !std::isfinite(c->leaky_alpha) || !std::isfinite(c->bn_eps) || c->bn_eps < 0.0f) return false;
    return true;
}

}  // namespace

struct btba_lfnet_det_model : LfnetModelBase {
    btba_lfnet_det_config cfg{};
    struct Pair { size_t scale = 0, shift = 0; };                    // offsets in floats into dev
    struct Block { Pair pre, mid, out; size_t w1 = 0, w2 = 0; };
    size_t init_w = 0, init_b = 0;
    Block blocks[BTBA_LFNET_DET_MAX_BLOCKS];
    Pair fin;
    size_t score_w[BTBA_LFNET_MAX_SCALES] = {}, ori_w = 0;
    float score_b[BTBA_LFNET_MAX_SCALES] = {}, ori_b[2] = {};
};

namespace {
template <int NT, int KS> int det_conv_launch(btba_workspace *ws, const DetConv &G, unsigned grid)
{
    const size_t lds = sizeof(float) * det_lds_floats(16 * NT, KS);
    k_det_conv<NT, KS><<<grid, 256, lds, ws->stream>>>(G);
    HIP_TRY(hipGetLastError());
    return BTBA_OK;
}

int det_conv_enqueue(btba_workspace *ws, int C, int ks, const DetConv &G, unsigned grid)
{
    switch ((C / 16) * 10 + ks) {
    case 13: return det_conv_launch<1, 3>(ws, G, grid);
    case 15: return det_conv_launch<1, 5>(ws, G, grid);
    case 23: return det_conv_launch<2, 3>(ws, G, grid);
    case 25: return det_conv_launch<2, 5>(ws, G, grid);
    case 33: return det_conv_launch<3, 3>(ws, G, grid);
    case 35: return det_conv_launch<3, 5>(ws, G, grid);
    case 43: return det_conv_launch<4, 3>(ws, G, grid);
    case 45: return det_conv_launch<4, 5>(ws, G, grid);
    }
    return BTBA_EINVAL;
}

// dynamic LDS above the default limit of 64 KB: the tiles of C >= 48 (108.8 KB at C = 64 with five taps)
int det_attrs(btba_workspace *ws)
{
    if (ws->lfnet_det_attr_set) return BTBA_OK;
    const void *fns[] = { reinterpret_cast<const void *>(&k_det_conv<3, 3>), reinterpret_cast<const void *>(&k_det_conv<3, 5>),
                          reinterpret_cast<const void *>(&k_det_conv<4, 3>), reinterpret_cast<const void *>(&k_det_conv<4, 5>),
                          reinterpret_cast<const void *>(&k_det_head<1>), reinterpret_cast<const void *>(&k_det_head<2>) };
    for (const void *fn : fns) HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
    ws->lfnet_det_attr_set = true;
    return BTBA_OK;
}
}  // namespace

extern "C" {

int btba_lfnet_det_scales(double min_scale, double max_scale, int num_scales, double *out)
{
    if (!out || num_scales < 1 || num_scales > BTBA_LFNET_MAX_SCALES || !std::isfinite(min_scale) || !std::isfinite(max_scale) ||
        !(min_scale > 0.0) || !(max_scale > 0.0))
        return BTBA_EINVAL;
    if (num_scales == 1) { out[0] = 1.0; return BTBA_OK; }           // mso_resnet_detector.py:106-107
    // numpy.linspace: arange(num) * step + start, the last value replaced by stop
    const double start = std::log(max_scale), stop = std::log(min_scale), step = (stop - start) / (double)(num_scales - 1);
    for (int i = 0; i < num_scales; i++) {
        volatile double prod = (double)i * step;
        out[i] = std::exp(i == num_scales - 1 ? stop : prod + start);
    }
    return BTBA_OK;
}

void btba_lfnet_det_config_default(btba_lfnet_det_config *c)
{
    if (!c) return;
    std::memset(c, 0, sizeof(*c));
    c->channels = 16; c->ksize = 5; c->blocks = 3; c->num_scales = 5;                 // train_lfnet.py:1113-1137
    (void)btba_lfnet_det_scales(1.0 / std::sqrt(2.0), std::sqrt(2.0), 5, c->scale_factors);
    c->activation = 1; c->leaky_alpha = 0.2f;
    c->bn_eps = 1e-5f;                                                                // tf_layer_utils.py:185
}

int btba_lfnet_det_model_create(btba_workspace *ws, const btba_lfnet_det_config *cfg, const btba_lfnet_det_weights *wts, btba_lfnet_det_model **out)
{
    if (out) *out = nullptr;
    if (!ws || !wts || !out || !det_config_ok(cfg)) return BTBA_EINVAL;
    const int C = cfg->channels, k = cfg->ksize, kk = k * k, S = cfg->num_scales;
    const size_t N = (size_t)C;
    const float eps = cfg->bn_eps;
    if (!lfnet_conv_ok(wts->init_conv, (size_t)kk, N) || !lfnet_bn_ok(wts->fin_bn, N, eps) || !lfnet_conv_ok(wts->ori_conv, (size_t)kk * C, 2))
        return BTBA_EINVAL;
    for (int i = 0; i < cfg->blocks; i++) {
        const btba_lfnet_det_block &b = wts->block[i];
        if (!lfnet_bn_ok(b.pre_bn, N, eps) || !lfnet_conv_ok(b.conv1, (size_t)kk * C, N) || !lfnet_bn_ok(b.conv1, N, eps) ||
            !lfnet_conv_ok(b.conv2, (size_t)kk * C, N))
            return BTBA_EINVAL;
    }
    for (int j = 0; j < S; j++)
        if (!lfnet_conv_ok(wts->score_conv[j], (size_t)kk * C, 1)) return BTBA_EINVAL;
    // every argument has been checked; the first HIP call follows
    std::unique_ptr<btba_lfnet_det_model> M(new (std::nothrow) btba_lfnet_det_model());
    if (!M) return BTBA_ENOMEM;
    M->ws = ws; M->device = ws->device; M->cfg = *cfg;
    LfnetArena A;
    auto take_pair = [&](btba_lfnet_det_model::Pair &p) { p.scale = A.take(N); p.shift = A.take(N); };
    M->init_w = A.take((size_t)kk * C); M->init_b = A.take(N);
    for (int i = 0; i < cfg->blocks; i++) {
        btba_lfnet_det_model::Block &B = M->blocks[i];
        take_pair(B.pre); B.w1 = A.take((size_t)kk * C * C); take_pair(B.mid); B.w2 = A.take((size_t)kk * C * C); take_pair(B.out);
    }
    take_pair(M->fin);
    for (int j = 0; j < S; j++) M->score_w[j] = A.take((size_t)kk * C);
    M->ori_w = A.take((size_t)kk * C * 2);
    A.fill();
    auto fold = [&](const btba_lfnet_desc_layer &bn, const float *bias, const btba_lfnet_det_model::Pair &p) {
        lfnet_fold(bn, bias, C, eps, A.at(p.scale), A.at(p.shift));
    };
    A.put(M->init_w, wts->init_conv.weights, (size_t)kk * C);                                    // [k][k][1][C] IS [k * k][C]
    if (wts->init_conv.biases) A.put(M->init_b, wts->init_conv.biases, N);
    const btba_lfnet_desc_layer no_bn{};
    for (int i = 0; i < cfg->blocks; i++) {
        const btba_lfnet_det_block &b = wts->block[i];
        const btba_lfnet_det_model::Block &B = M->blocks[i];
        fold(b.pre_bn, nullptr, B.pre);
        A.put(B.w1, b.conv1.weights, (size_t)kk * C * C);                                        // [k][k][C][C] IS [K][N] in (ky, kx, c_in) order
        fold(b.conv1, b.conv1.biases, B.mid);
        A.put(B.w2, b.conv2.weights, (size_t)kk * C * C);
        fold(no_bn, b.conv2.biases, B.out);
    }
    fold(wts->fin_bn, nullptr, M->fin);
    for (int j = 0; j < S; j++) {
        A.put(M->score_w[j], wts->score_conv[j].weights, (size_t)kk * C);
        M->score_b[j] = wts->score_conv[j].biases ? wts->score_conv[j].biases[0] : 0.0f;
    }
    A.put(M->ori_w, wts->ori_conv.weights, (size_t)kk * C * 2);
    for (int o = 0; o < 2; o++) M->ori_b[o] = wts->ori_conv.biases ? wts->ori_conv.biases[o] : 0.0f;
    DeviceGuard device_guard(ws);
    if (int rc = M->upload(A)) return rc;
    *out = M.release();
    return BTBA_OK;
}

void btba_lfnet_det_model_destroy(btba_lfnet_det_model *M) { destroy_on_device(M); }

int btba_lfnet_det_map_size(double scale_factor, int size)
{
    if (!std::isfinite(scale_factor) || !(scale_factor > 0.0) || size < 1 || size > BTBA_LFNET_MAX_SIZE) return -1;
    return det_map_size(scale_factor, size);
}

int btba_lfnet_det_map_sizes(const btba_lfnet_det_model *M, int H, int W, int32_t *map_h, int32_t *map_w)
{
    if (!M || !map_h || !map_w || H < 1 || W < 1 || H > BTBA_LFNET_MAX_SIZE || W > BTBA_LFNET_MAX_SIZE) return BTBA_EINVAL;
    for (int j = 0; j < M->cfg.num_scales; j++) {
        map_h[j] = det_map_size(M->cfg.scale_factors[j], H);
        map_w[j] = det_map_size(M->cfg.scale_factors[j], W);
        if (map_h[j] < 1 || map_w[j] < 1 || map_h[j] > BTBA_LFNET_MAX_SIZE || map_w[j] > BTBA_LFNET_MAX_SIZE) return BTBA_EINVAL;
    }
    return BTBA_OK;
}

int btba_lfnet_det_pad_size(const btba_lfnet_det_model *M)
{
    return M ? (2 * M->cfg.blocks + 2) * (M->cfg.ksize / 2) : -1;     // num_conv * (conv_ksize // 2), mso_resnet_detector.py:171
}

int btba_lfnet_scores(btba_workspace *ws, const btba_lfnet_det_model *M, int n_frames, int H, int W, const float *photo_dev,
                      float *const *score_dev, float *ori_dev)
{
    if (!ws || !M || n_frames < 0 || M->ws != ws) return BTBA_EINVAL;
    int32_t mh[BTBA_LFNET_MAX_SCALES], mw[BTBA_LFNET_MAX_SCALES];
    if (int rc = btba_lfnet_det_map_sizes(M, H, W, mh, mw)) return rc;
    if (n_frames == 0) return BTBA_OK;
    if (!photo_dev || !score_dev || !ori_dev || misaligned(photo_dev, 4) || misaligned(ori_dev, 4)) return BTBA_EINVAL;
    const btba_lfnet_det_config &c = M->cfg;
    const int C = c.channels, ks = c.ksize, S = c.num_scales;
    for (int j = 0; j < S; j++)
        if (!score_dev[j] || misaligned(score_dev[j], 4)) return BTBA_EINVAL;
    DeviceGuard device_guard(ws);
    const int64_t frame_px = (int64_t)H * W;
    const int per_pass = (int)std::min<int64_t>(n_frames, std::max<int64_t>(1, BTBA_LFNET_DET_PASS_PIXELS / frame_px));
    Scratch sc;
    Scratch::Region<float> rx = sc.add<float>((size_t)per_pass * frame_px * C), rt = sc.add<float>((size_t)per_pass * frame_px * C);
    if (int rc = sc.bind(ws->lfnet_det)) return rc;
    if (int rc = det_attrs(ws)) return rc;
    float *x = rx, *t = rt;
    const float *Wd = M->dev.as<float>();
    const int tiles_x = (W + kDetTile - 1) / kDetTile, tiles_y = (H + kDetTile - 1) / kDetTile;
    const size_t head_lds = sizeof(float) * det_lds_floats(C, ks);
    for (int f0 = 0; f0 < n_frames; f0 += per_pass) {
        const int nf = std::min(per_pass, n_frames - f0);
        {
            DetInit G{};
            G.photo = photo_dev + (size_t)f0 * frame_px; G.w = Wd + M->init_w; G.bias = Wd + M->init_b; G.out = x;
            G.H = H; G.W = W; G.C = C; G.ks = ks; G.threads = (long long)nf * frame_px * (C / 4);
            k_det_init<<<(unsigned)((G.threads + 255) / 256), 256, 0, ws->stream>>>(G);
            HIP_TRY(hipGetLastError());
        }
        const unsigned grid = (unsigned)nf * tiles_y * tiles_x;
        for (int i = 0; i < c.blocks; i++) {
            const btba_lfnet_det_model::Block &B = M->blocks[i];
            DetConv G{};
            G.H = H; G.W = W; G.tiles_x = tiles_x; G.tiles_y = tiles_y; G.act = c.activation; G.alpha = c.leaky_alpha;
            G.in = x; G.w = Wd + B.w1; G.in_scale = Wd + B.pre.scale; G.in_shift = Wd + B.pre.shift; G.scale = Wd + B.mid.scale;
            G.shift = Wd + B.mid.shift; G.shortcut = nullptr; G.out = t; G.out_act = c.activation;
            if (int rc = det_conv_enqueue(ws, C, ks, G, grid)) return rc;
            G.in = t; G.w = Wd + B.w2; G.in_scale = G.in_shift = nullptr; G.scale = Wd + B.out.scale; G.shift = Wd + B.out.shift;
            G.shortcut = x; G.out = x; G.out_act = kLfnetActNone;          // in place: a lane reads and writes its own elements only
            if (int rc = det_conv_enqueue(ws, C, ks, G, grid)) return rc;
        }
        DetHead G{};
        G.x = x; G.fscale = Wd + M->fin.scale; G.fshift = Wd + M->fin.shift; G.H = H; G.W = W; G.C = C; G.ks = ks; G.act = c.activation;
        G.alpha = c.leaky_alpha;
        for (int j = 0; j < S; j++) {
            G.w = Wd + M->score_w[j]; G.out = score_dev[j] + (size_t)f0 * mh[j] * mw[j]; G.bias0 = M->score_b[j]; G.bias1 = 0.0f;
            G.h = mh[j]; G.w_out = mw[j]; G.tiles_x = (mw[j] + kDetTile - 1) / kDetTile; G.tiles_y = (mh[j] + kDetTile - 1) / kDetTile;
            k_det_head<1><<<(unsigned)nf * G.tiles_y * G.tiles_x, 256, head_lds, ws->stream>>>(G);
            HIP_TRY(hipGetLastError());
        }
        G.w = Wd + M->ori_w; G.out = ori_dev + (size_t)f0 * frame_px * 2; G.bias0 = M->ori_b[0]; G.bias1 = M->ori_b[1];
        G.h = H; G.w_out = W; G.tiles_x = tiles_x; G.tiles_y = tiles_y;
        k_det_head<2><<<grid, 256, head_lds, ws->stream>>>(G);
        HIP_TRY(hipGetLastError());
    }
    return BTBA_OK;
}

}  // extern "C"
