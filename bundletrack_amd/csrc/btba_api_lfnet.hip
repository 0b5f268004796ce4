// btba_api_lfnet.hip -- host side of libbtba.so: LF-Net's key-point head and descriptor net.
#include "btba_host_common.hpp"
#include "btba_lfnet.hpp"
#include "btba_lfnet_desc.hpp"

extern "C" {

void btba_lfnet_params_default(btba_lfnet_params *p)
{
    if (!p) return;
    p->sm_ksize = 15; p->com_strength = 3.0f; p->score_com_strength = 100.0f; p->scale_com_strength = 100.0f;      // train_lfnet.py:1047-1189
    p->nms_thresh = 0.0f; p->nms_ksize = 5;
    p->top_k = 500;                                                   // run_server.py
    p->pad_size = 16;                                                 // mso_resnet_detector.py:171: five-tap convolutions, three blocks
    p->crop_radius = 16; p->soft_kpts = 1; p->kp_loc_size = 9; p->do_softmax_kp_refine = 1; p->kp_com_strength = 1.0f; p->patch_size = 32;
}

namespace {
bool lfnet_params_ok(const btba_lfnet_params *p, int n_frames, int H, int W)
{
    if (!p || n_frames < 1 || H < 1 || W < 1 || H > BTBA_LFNET_MAX_SIZE || W > BTBA_LFNET_MAX_SIZE) return false;
    if (p->sm_ksize < 1 || p->sm_ksize > BTBA_LFNET_MAX_KSIZE || p->sm_ksize % 2 == 0) return false;
    if (p->nms_ksize < 1 || p->nms_ksize > BTBA_LFNET_MAX_KSIZE || p->nms_ksize % 2 == 0) return false;
    if (p->top_k < 1 || p->top_k > BTBA_LFNET_MAX_TOP_K) return false;
    const int m = std::min(H, W);
    if (p->pad_size < 0 || p->crop_radius < 0 || 2 * (int64_t)p->pad_size >= m || 2 * (int64_t)p->crop_radius >= m) return false;
    if (p->patch_size < 2 || p->patch_size > 64 || p->kp_loc_size < 2 || p->kp_loc_size > 64) return false;
    return true;
}

// One layout for all three stages, so that a call of any of them leaves the others' regions where they were.
struct LfnetScratch {
    Scratch sc;
    Scratch::Region<float2> stats;
    Scratch::Region<uint8_t> peak;
    Scratch::Region<int32_t> list_idx;
    Scratch::Region<uint32_t> list_key;
    LfnetScratch(int n_frames, int H, int W)
        : stats(sc.add<float2>((size_t)n_frames * kLfnetMaxScales)), peak(sc.add<uint8_t>((size_t)n_frames * H * W)),
          list_idx(sc.add<int32_t>((size_t)n_frames * H * W)), list_key(sc.add<uint32_t>((size_t)n_frames * H * W)) {}
};

int lfnet_heatmaps_enqueue(btba_workspace *ws, const btba_lfnet_params *prm, LfnetScratch &L, int n_frames, int H, int W, int S,
                           const float *const *score_dev, const int32_t *map_h, const int32_t *map_w, const float *scale_factors,
                           float *heat_dev, float *scales_dev)
{
    LfnetMaps M{};
    for (int s = 0; s < S; s++) { M.p[s] = score_dev[s]; M.h[s] = map_h[s]; M.w[s] = map_w[s]; M.sf[s] = scale_factors[s]; }
    const int h = prm->sm_ksize / 2;
    int T = 16;
    if (sizeof(float) * lfnet_heat_lds_floats(S, T, h) > 80 * 1024) T = 8;
    const size_t lds = sizeof(float) * lfnet_heat_lds_floats(S, T, h);          // at most 122 KB (S = 16, k = 31)
    if (!ws->lfnet_attr_set) {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_lfnet_heat), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        ws->lfnet_attr_set = true;
    }
    k_lfnet_moments<<<dim3(S, n_frames), 256, 0, ws->stream>>>(M, L.stats);
    HIP_TRY(hipGetLastError());
    k_lfnet_heat<<<dim3((W + T - 1) / T, (H + T - 1) / T, n_frames), 256, lds, ws->stream>>>(
        M, L.stats, S, H, W, T, h, prm->com_strength, prm->score_com_strength, prm->scale_com_strength, prm->pad_size, heat_dev, scales_dev);
    HIP_TRY(hipGetLastError());
    return BTBA_OK;
}

int lfnet_select_enqueue(btba_workspace *ws, const btba_lfnet_params *prm, LfnetScratch &L, int n_frames, int H, int W, const float *heat_dev,
                         int32_t *kpts_xy_dev, int32_t *n_kpts_dev)
{
    k_lfnet_peaks<<<dim3((H * W + 255) / 256, n_frames), 256, 0, ws->stream>>>(heat_dev, H, W, prm->nms_thresh, prm->nms_ksize / 2, L.peak);
    HIP_TRY(hipGetLastError());
    k_lfnet_select<<<n_frames, kLfnetSelectThreads, 0, ws->stream>>>(heat_dev, L.peak, H, W, prm->crop_radius, prm->top_k, L.list_idx, L.list_key,
                                                                     kpts_xy_dev, n_kpts_dev);
    HIP_TRY(hipGetLastError());
    return BTBA_OK;
}

int lfnet_crops_enqueue(btba_workspace *ws, const btba_lfnet_params *prm, int n_frames, int H, int W, const float *photo_dev, const float *ori_dev,
                        const float *heat_dev, const float *scales_dev, const int32_t *kpts_xy_dev, const int32_t *n_kpts_dev,
                        float *kpts_out_dev, float *kpts_scale_out_dev, float *kpts_ori_out_dev, float *patches_out_dev)
{
    k_lfnet_crops<<<dim3(prm->top_k, n_frames), 64, 0, ws->stream>>>(photo_dev, ori_dev, heat_dev, scales_dev, kpts_xy_dev, n_kpts_dev, H, W,
                                                                     prm->top_k, prm->soft_kpts, prm->kp_loc_size, prm->do_softmax_kp_refine,
                                                                     prm->kp_com_strength, prm->patch_size, kpts_out_dev, kpts_scale_out_dev,
                                                                     kpts_ori_out_dev, patches_out_dev);
    HIP_TRY(hipGetLastError());
    return BTBA_OK;
}

bool lfnet_maps_ok(int S, const float *const *score_dev, const int32_t *map_h, const int32_t *map_w, const float *scale_factors)
{
    if (S < 1 || S > BTBA_LFNET_MAX_SCALES || !score_dev || !map_h || !map_w || !scale_factors) return false;
    for (int s = 0; s < S; s++)
        if (!score_dev[s] || misaligned(score_dev[s], 4) || map_h[s] < 1 || map_w[s] < 1 || map_h[s] > 4 * BTBA_LFNET_MAX_SIZE ||
            map_w[s] > 4 * BTBA_LFNET_MAX_SIZE || (int64_t)map_h[s] * map_w[s] > INT32_MAX)
            return false;
    return true;
}
}  // namespace

int btba_lfnet_heatmaps(btba_workspace *ws, const btba_lfnet_params *prm, int n_frames, int H, int W, int S, const float *const *score_dev,
                        const int32_t *map_h, const int32_t *map_w, const float *scale_factors, float *max_heatmaps_dev, float *max_scales_dev)
{
    if (!ws || !lfnet_params_ok(prm, n_frames, H, W) || !lfnet_maps_ok(S, score_dev, map_h, map_w, scale_factors) || !max_heatmaps_dev ||
        !max_scales_dev || misaligned(max_heatmaps_dev, 4) || misaligned(max_scales_dev, 4))
        return BTBA_EINVAL;
    DeviceGuard device_guard(ws);
    LfnetScratch L(n_frames, H, W);
    if (int rc = L.sc.bind(ws->lfnet)) return rc;
    return lfnet_heatmaps_enqueue(ws, prm, L, n_frames, H, W, S, score_dev, map_h, map_w, scale_factors, max_heatmaps_dev, max_scales_dev);
}

int btba_lfnet_select(btba_workspace *ws, const btba_lfnet_params *prm, int n_frames, int H, int W, const float *heat_dev,
                      int32_t *kpts_xy_dev, int32_t *n_kpts_dev)
{
    if (!ws || !lfnet_params_ok(prm, n_frames, H, W) || !heat_dev || !kpts_xy_dev || !n_kpts_dev || misaligned(heat_dev, 4) ||
        misaligned(kpts_xy_dev, 4) || misaligned(n_kpts_dev, 4))
        return BTBA_EINVAL;
    DeviceGuard device_guard(ws);
    LfnetScratch L(n_frames, H, W);
    if (int rc = L.sc.bind(ws->lfnet)) return rc;
    return lfnet_select_enqueue(ws, prm, L, n_frames, H, W, heat_dev, kpts_xy_dev, n_kpts_dev);
}

int btba_lfnet_crops(btba_workspace *ws, const btba_lfnet_params *prm, int n_frames, int H, int W, const float *photo_dev, const float *ori_dev,
                     const float *heat_dev, const float *scales_dev, const int32_t *kpts_xy_dev, const int32_t *n_kpts_dev,
                     float *kpts_out_dev, float *kpts_scale_out_dev, float *kpts_ori_out_dev, float *patches_out_dev)
{
    if (!ws || !lfnet_params_ok(prm, n_frames, H, W) || !photo_dev || !ori_dev || !heat_dev || !scales_dev || !kpts_xy_dev || !n_kpts_dev ||
        !kpts_out_dev || !kpts_scale_out_dev || !kpts_ori_out_dev || !patches_out_dev)
        return BTBA_EINVAL;
    for (const void *q : { (const void *)photo_dev, (const void *)ori_dev, (const void *)heat_dev, (const void *)scales_dev, (const void *)kpts_xy_dev,
                           (const void *)n_kpts_dev, (const void *)kpts_out_dev, (const void *)kpts_scale_out_dev, (const void *)kpts_ori_out_dev,
                           (const void *)patches_out_dev })
        if (misaligned(q, 4)) return BTBA_EINVAL;
    DeviceGuard device_guard(ws);
    return lfnet_crops_enqueue(ws, prm, n_frames, H, W, photo_dev, ori_dev, heat_dev, scales_dev, kpts_xy_dev, n_kpts_dev, kpts_out_dev,
                               kpts_scale_out_dev, kpts_ori_out_dev, patches_out_dev);
}

int btba_lfnet_keypoints(btba_workspace *ws, const btba_lfnet_params *prm, int n_frames, int H, int W, int S, const float *const *score_dev,
                         const int32_t *map_h, const int32_t *map_w, const float *scale_factors, const float *photo_dev, const float *ori_dev,
                         float *max_heatmaps_dev, float *max_scales_dev, int32_t *kpts_xy_dev, int32_t *n_kpts_dev, float *kpts_out_dev,
                         float *kpts_scale_out_dev, float *kpts_ori_out_dev, float *patches_out_dev, int32_t *n_kpts_host)
{
    // every argument is checked before the first HIP call
    if (!ws || !lfnet_params_ok(prm, n_frames, H, W) || !lfnet_maps_ok(S, score_dev, map_h, map_w, scale_factors) || !photo_dev || !ori_dev ||
        !max_heatmaps_dev || !max_scales_dev || !kpts_xy_dev || !n_kpts_dev || !kpts_out_dev || !kpts_scale_out_dev || !kpts_ori_out_dev ||
        !patches_out_dev)
        return BTBA_EINVAL;
    for (const void *q : { (const void *)photo_dev, (const void *)ori_dev, (const void *)max_heatmaps_dev, (const void *)max_scales_dev,
                           (const void *)kpts_xy_dev, (const void *)n_kpts_dev, (const void *)kpts_out_dev, (const void *)kpts_scale_out_dev,
                           (const void *)kpts_ori_out_dev, (const void *)patches_out_dev })
        if (misaligned(q, 4)) return BTBA_EINVAL;
    DeviceGuard device_guard(ws);
    LfnetScratch L(n_frames, H, W);
    if (int rc = L.sc.bind(ws->lfnet)) return rc;
    if (int rc = lfnet_heatmaps_enqueue(ws, prm, L, n_frames, H, W, S, score_dev, map_h, map_w, scale_factors, max_heatmaps_dev, max_scales_dev)) return rc;
    if (int rc = lfnet_select_enqueue(ws, prm, L, n_frames, H, W, max_heatmaps_dev, kpts_xy_dev, n_kpts_dev)) return rc;
    if (int rc = lfnet_crops_enqueue(ws, prm, n_frames, H, W, photo_dev, ori_dev, max_heatmaps_dev, max_scales_dev, kpts_xy_dev, n_kpts_dev,
                                     kpts_out_dev, kpts_scale_out_dev, kpts_ori_out_dev, patches_out_dev))
        return rc;
    if (n_kpts_host) {
        HIP_TRY(hipMemcpyAsync(n_kpts_host, n_kpts_dev, sizeof(int32_t) * (size_t)n_frames, hipMemcpyDeviceToHost, ws->stream));
        HIP_TRY(hipStreamSynchronize(ws->stream));                   // the call's one host wait
    }
    return BTBA_OK;
}

void btba_lfnet_desc_config_default(btba_lfnet_desc_config *c)
{
    if (!c) return;
    c->patch_size = 32; c->depth = 3; c->channels = 64; c->fc_dim = 512; c->out_dim = 256;      // simple_desc.py:10-14, run_server.py's checkpoint
    c->activation = 0; c->leaky_alpha = 0.2f; c->norm = 0;
    c->bn_eps = 1e-5f;                                                // tf_layer_utils.py:185
}

struct btba_lfnet_desc_model : LfnetModelBase {
    btba_lfnet_desc_config cfg{};
    struct Layer { size_t w = 0, scale = 0, shift = 0; int K = 0, N = 0; };      // offsets in floats into dev
    Layer layers[BTBA_LFNET_DESC_MAX_DEPTH + 2];
    int n_layers = 0;
    size_t widest = 0;                     // floats per patch of the widest layer output
};

namespace {
bool desc_config_ok(const btba_lfnet_desc_config *c)
{
    if (!c || c->depth < 1 || c->depth > BTBA_LFNET_DESC_MAX_DEPTH || c->patch_size < 8 || c->patch_size > 64 || c->patch_size % (1 << c->depth)) return false;
    if (c->channels < 16 || c->channels > 128 || c->channels % 16 || c->fc_dim < 16 || c->fc_dim > 1024 || c->fc_dim % 16) return false;
    if (c->out_dim < 16 || c->out_dim > 512 || c->out_dim % 16 || c->activation < 0 || c->activation > 1 || c->norm < 0 || c->norm > 1) return false;
    if (!std::isfinite(c->leaky_alpha) || !std::isfinite(c->bn_eps) || c->bn_eps < 0.0f) return false;
    const int s = c->patch_size >> c->depth;
    return (int64_t)s * s * (c->channels << (c->depth - 1)) <= 16384;
}
}  // namespace

int btba_lfnet_desc_model_create(btba_workspace *ws, const btba_lfnet_desc_config *cfg, const btba_lfnet_desc_weights *wts, btba_lfnet_desc_model **out)
{
    if (out) *out = nullptr;
    if (!ws || !wts || !out || !desc_config_ok(cfg)) return BTBA_EINVAL;
    const int depth = cfg->depth, n_layers = depth + 2;
    const btba_lfnet_desc_layer *src[BTBA_LFNET_DESC_MAX_DEPTH + 2];
    int Ks[BTBA_LFNET_DESC_MAX_DEPTH + 2], Ns[BTBA_LFNET_DESC_MAX_DEPTH + 2];
    size_t widest = 0;
    for (int i = 0; i < depth; i++) {
        src[i] = &wts->conv[i];
        Ks[i] = 9 * (i ? cfg->channels << (i - 1) : 1);
        Ns[i] = cfg->channels << i;
        const size_t s = (size_t)(cfg->patch_size >> (i + 1));
        widest = std::max(widest, s * s * Ns[i]);
    }
    const int flat = (cfg->patch_size >> depth) * (cfg->patch_size >> depth) * Ns[depth - 1];
    src[depth] = &wts->fc1; Ks[depth] = flat; Ns[depth] = cfg->fc_dim;
    src[depth + 1] = &wts->fc2; Ks[depth + 1] = cfg->fc_dim; Ns[depth + 1] = cfg->out_dim;
    widest = std::max(widest, (size_t)std::max(cfg->fc_dim, cfg->out_dim));
    for (int i = 0; i < n_layers; i++)
        if (!lfnet_conv_ok(*src[i], (size_t)Ks[i], (size_t)Ns[i]) || !lfnet_bn_ok(*src[i], (size_t)Ns[i], cfg->bn_eps)) return BTBA_EINVAL;
    // every argument has been checked; the first HIP call follows
    std::unique_ptr<btba_lfnet_desc_model> M(new (std::nothrow) btba_lfnet_desc_model());
    if (!M) return BTBA_ENOMEM;
    M->ws = ws; M->device = ws->device; M->cfg = *cfg; M->n_layers = n_layers; M->widest = widest;
    LfnetArena A;
    for (int i = 0; i < n_layers; i++) {
        btba_lfnet_desc_model::Layer &L = M->layers[i];
        L.K = Ks[i]; L.N = Ns[i];
        L.w = A.take((size_t)L.K * L.N); L.scale = A.take(L.N); L.shift = A.take(L.N);
    }
    A.fill();
    for (int i = 0; i < n_layers; i++) {
        const btba_lfnet_desc_model::Layer &L = M->layers[i];
        A.put(L.w, src[i]->weights, (size_t)L.K * L.N);              // [3][3][C_in][C_out] IS [K][N] in (ky, kx, c_in) order
        lfnet_fold(*src[i], src[i]->biases, L.N, cfg->bn_eps, A.at(L.scale), A.at(L.shift));
    }
    DeviceGuard device_guard(ws);
    if (int rc = M->upload(A)) return rc;
    *out = M.release();
    return BTBA_OK;
}

void btba_lfnet_desc_model_destroy(btba_lfnet_desc_model *M) { destroy_on_device(M); }

int btba_lfnet_descriptors(btba_workspace *ws, const btba_lfnet_desc_model *M, int n_frames, int slots, const float *patches_dev,
                           const int32_t *n_kpts_dev, float *desc_dev)
{
    // the counts first: a model is not read before they are known to be sane
    if (!ws || !M || n_frames < 0 || slots < 0 || slots > BTBA_LFNET_MAX_TOP_K || (int64_t)n_frames * slots > (1 << 24)) return BTBA_EINVAL;
    const int total = n_frames * slots;
    if (total == 0) return BTBA_OK;
    if (!patches_dev || !desc_dev || misaligned(patches_dev, 4) || misaligned(desc_dev, 4) || misaligned(n_kpts_dev, 4) || M->ws != ws) return BTBA_EINVAL;
    DeviceGuard device_guard(ws);
    const btba_lfnet_desc_config &c = M->cfg;
    const int chunk = std::min(total, kDescChunk), P = c.patch_size, depth = c.depth, D = c.out_dim;
    Scratch sc;
    Scratch::Region<float> b0 = sc.add<float>((size_t)chunk * M->widest), b1 = sc.add<float>((size_t)chunk * M->widest);
    if (int rc = sc.bind(ws->lfnet_desc)) return rc;
    float *buf[2] = { b0, b1 };
    const float *W = M->dev.as<float>();
    for (int p0 = 0; p0 < total; p0 += chunk) {
        const int np = std::min(chunk, total - p0);
        {
            const btba_lfnet_desc_model::Layer &L = M->layers[0];
            DescConv1 G{};
            G.patches = patches_dev + (size_t)p0 * P * P; G.w = W + L.w; G.scale = W + L.scale; G.shift = W + L.shift; G.out = buf[0];
            G.n_kpts = n_kpts_dev; G.n_patches = np; G.P = P; G.Ho = P / 2; G.pad = 0; G.C = L.N; G.act = c.activation; G.slots = slots;
            G.patch0 = p0; G.alpha = c.leaky_alpha;
            const int64_t threads = (int64_t)np * G.Ho * G.Ho * (L.N / 4);
            k_desc_conv1<<<(unsigned)((threads + 255) / 256), 256, 0, ws->stream>>>(G);
            HIP_TRY(hipGetLastError());
        }
        for (int i = 1; i < M->n_layers; i++) {
            const btba_lfnet_desc_model::Layer &L = M->layers[i];
            const bool conv = i < depth;
            DescGemm G{};
            G.in = buf[(i - 1) & 1]; G.out = buf[i & 1]; G.w = W + L.w; G.scale = W + L.scale; G.shift = W + L.shift; G.n_kpts = n_kpts_dev;
            G.N = L.N; G.K = L.K; G.slots = slots; G.patch0 = p0; G.alpha = c.leaky_alpha;
            if (conv) {               // an even input size: TensorFlow's SAME pads nothing before and one row and column after
                G.Hi = G.Wi = P >> i; G.Ho = G.Wo = P >> (i + 1); G.Cin = L.K / 9; G.ks = 3; G.pad = 0; G.act = c.activation;
            } else {
                G.Hi = G.Wi = G.Ho = G.Wo = 1; G.Cin = L.K; G.ks = 1; G.pad = 0; G.act = i == depth ? c.activation : kLfnetActNone;
            }
            G.M = np * G.Ho * G.Wo;
            k_desc_gemm<<<dim3((G.M + kDescBM - 1) / kDescBM, (G.N + kDescBN - 1) / kDescBN), 256, 0, ws->stream>>>(G);
            HIP_TRY(hipGetLastError());
        }
        k_desc_finish<<<(np + 3) / 4, 256, 0, ws->stream>>>(buf[(M->n_layers - 1) & 1], desc_dev + (size_t)p0 * D, n_kpts_dev, np, D, c.norm == 0,
                                                             slots, p0);
        HIP_TRY(hipGetLastError());
    }
    return BTBA_OK;
}

}  // extern "C"
