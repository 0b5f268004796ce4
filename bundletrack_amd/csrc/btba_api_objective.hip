// btba_api_objective.hip -- the objective report: the cost the Gauss-Newton loop descends, at the caller's poses (btba_objective_batch_zn_aux).
// Kernels: btba_objective.hpp; their layout: btba_objective_layout.hpp.  The kernels call the sweeps' device functions, and the header that holds
// those (btba_kernels.hpp) defines kernels and so belongs to one unit: the launches are objective_enqueue in btba_api.hip, behind the checks made here.
#include "btba_host_common.hpp"
#include "btba_objective_layout.hpp"

static_assert(sizeof(btba_objective_pair) == 40 && sizeof(btba_objective_total) == 64, "the record sizes include/btba.h states");
static_assert(sizeof(btba_objective_pair) == kObjectiveRecordBytes, "the scratch layout counts in these records");
static_assert(kObjectiveChunkEntries % 64 == 0, "a chunk starts on a group of the 24-byte layout when its segment does");

extern "C" {

int btba_objective_batch_zn_aux(btba_workspace *ws, const btba_params *params, int n_instances, int n_frames, int H, int W, const float *K,
                                const float *zn_dev, const btba_zn_aux *aux, const btba_entryj *corr_dev, int64_t corr_stride,
                                const uint32_t *pair_offsets_dev, uint32_t max_corr_per_pair, const int32_t *dense_pairs, int n_dense_pairs,
                                const float *poses_dev, btba_objective_total *total_dev, btba_objective_pair *sparse_dev, btba_objective_pair *dense_dev)
{
    // (argument checks first: none of them touches the device)
    if (!ws || !params || !poses_dev || !total_dev || n_instances < 1 || n_frames < 2 || n_frames > BTBA_MAX_FRAMES) return BTBA_EINVAL;
    if (params->weights_sparse_per_iter || params->weights_dense_per_iter) return BTBA_EINVAL;      // the objective of WHICH iterate?  the scalar weights say
    if (misaligned(total_dev, 8) || misaligned(sparse_dev, 8) || misaligned(dense_dev, 8) || misaligned(poses_dev, 16)) return BTBA_EINVAL;
    // what btba_solve_batch_zn_aux asks of the cache
    if (!K || !zn_dev || H < 2 || W < 2 || !(params->image_downscale >= 1.0f)) return BTBA_EINVAL;
    const int Wd = (int)(W / params->image_downscale), Hd = (int)(H / params->image_downscale);
    if (Wd < 2 || Hd < 2) return BTBA_EINVAL;
    if (dense_pairs && n_dense_pairs < 0) return BTBA_EINVAL;
    const bool c24 = aux && aux->corr24;
    const void *corr = c24 ? static_cast<const void *>(aux->corr24) : static_cast<const void *>(corr_dev);
    if (corr && corr_stride < 0) return BTBA_EINVAL;
    DeviceGuard device_guard(ws);
    ObjectiveCall c{};
    c.prm = params; c.B = n_instances; c.N = n_frames; c.H = H; c.W = W; c.Hd = Hd; c.Wd = Wd;
    c.K = K; c.zn = zn_dev; c.poses = poses_dev;
    c.corr = corr; c.corr24 = c24; c.corr_stride = corr_stride;
    c.pair_offsets = pair_offsets_dev; c.max_corr_per_pair = max_corr_per_pair;
    c.dense_pairs = dense_pairs; c.n_dense_pairs = n_dense_pairs;
    c.total = total_dev; c.sparse = sparse_dev; c.dense = dense_dev;
    return objective_enqueue(ws, c);      // (no timed region, no event: the workspace's stats stay those of the last solve)
}

}  // extern "C"
