// btba_mappoints.hpp -- map-point (feature track) memory and the per-pair stages of the tracker's findCorres
// (btba_mappoints_*, btba_corres_chain, include/btba.h)
//   SiftManager::findCorres                 src/FeatureManager.cpp:173-240
//   SiftManager::updateFramePairMapPoints   :448-487
//   SiftManager::findCorresByMapPoints      :489-521
//   SiftManager::forgetFrame                :142-170
// Layout: a frame slot holds its keypoints (copied at registration), the canonical index of every keypoint (lowest index with
// the same (u, v)), the walk order of its canonical keys ((u, v) ascending, Frame::_map_points' std::map order) and map_F as one
// int32 map-point id per keypoint index (meaningful at canonical indices, -1 = none).  A map point is one row of img: one int32
// canonical keypoint index per slot (-1 = none).  Ids come from a free stack (map points whose row became empty on forget)
// before the high-water mark grows.  Every per-pair kernel is one workgroup; a chain runs them pair after pair on one stream.
#pragma once
#include <hip/hip_runtime.h>
#include <climits>

#include "btba_match.hpp"

namespace btba {

struct MpSlot {                        // device view of a frame slot
    const float2 *kpts;                // [n] keypoints (x, y)
    const int *canon;                  // [n] canonical index of every keypoint
    const int *order;                  // [n] canonical keys in (u, v) order, -1 past the last key
    int *map;                          // [n] map_F: map-point id per keypoint index, -1 = none
    int n, pad0, pad1, pad2;
};
enum { kMpNext = 0, kMpTop = 1, kMpErr = 2 };   // allocator words: high-water mark, free-stack height, overflow flag

struct CorresFrame { const float *depth; float pose[12]; int slot, pad; };
struct CorresPair { int a, b, neighbor, base; };    // frame indices (A newer), |idA - idB| == 1, first entry of the pair's working region
struct CorresDims { int W, H, slot_cap, mp_cap; Mat4 Kinv; };

__device__ __forceinline__ bool uv_less(float2 p, float2 q) { return p.x < q.x || (p.x == q.x && p.y < q.y); }

// ---- registration -------------------------------------------------------------------------------------------------------
// grid ceil(n / 256) x 256: canon[i] = lowest j with (u_j, v_j) == (u_i, v_i) (fp32 ==, so -0 == +0); bad = 1 on a non-finite keypoint
__global__ void __launch_bounds__(256) k_mp_canon(const float2 *__restrict__ kp, int n, int *__restrict__ canon, int *__restrict__ bad)
{
    __shared__ float2 tile[256];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const float2 me = i < n ? kp[i] : make_float2(0.f, 0.f);
    int c = i;
    for (int t0 = 0; t0 < n; t0 += 256) {
        if (t0 + (int)threadIdx.x < n) tile[threadIdx.x] = kp[t0 + threadIdx.x];
        __syncthreads();
        const int m = min(256, n - t0);
        for (int j = 0; j < m; j++) {
            const float2 q = tile[j];
            if (q.x == me.x && q.y == me.y) c = min(c, t0 + j);
        }
        __syncthreads();
    }
    if (i < n) {
        canon[i] = c;
        if (!(isfinite(me.x) && isfinite(me.y))) *bad = 1;
    }
}

// grid ceil(n / 256) x 256: order[rank of canonical key i among canonical keys] = i; map[i] = -1
__global__ void __launch_bounds__(256) k_mp_order(const float2 *__restrict__ kp, int n, const int *__restrict__ canon, int *__restrict__ order, int *__restrict__ map)
{
    __shared__ float2 tile[256];
    __shared__ int tcanon[256];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const float2 me = i < n ? kp[i] : make_float2(0.f, 0.f);
    int rank = 0;
    for (int t0 = 0; t0 < n; t0 += 256) {
        if (t0 + (int)threadIdx.x < n) { tile[threadIdx.x] = kp[t0 + threadIdx.x]; tcanon[threadIdx.x] = canon[t0 + threadIdx.x]; }
        __syncthreads();
        const int m = min(256, n - t0);
        for (int j = 0; j < m; j++) rank += (tcanon[j] == t0 + j && uv_less(tile[j], me)) ? 1 : 0;
        __syncthreads();
    }
    if (i < n) {
        map[i] = -1;
        if (canon[i] == i) order[rank] = i;
    }
}

// one workgroup of 256: erase img[F] of every map point (ids below the high-water mark); map points whose row becomes empty go
// onto the free stack in ascending id order
__global__ void __launch_bounds__(256) k_mp_forget(int slot, int slot_cap, int *__restrict__ img, int *__restrict__ hdr, int *__restrict__ stack)
{
    __shared__ int wsum[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int next = hdr[kMpNext];
    int top = hdr[kMpTop];
    for (int m0 = 0; m0 < next; m0 += 256) {
        const int m = m0 + threadIdx.x;
        bool freed = false;
        if (m < next && img[(size_t)m * slot_cap + slot] >= 0) {
            img[(size_t)m * slot_cap + slot] = -1;
            freed = true;
            for (int s = 0; s < slot_cap && freed; s++) freed = img[(size_t)m * slot_cap + s] < 0;
        }
        const unsigned long long bal = __ballot(freed);
        if (lane == 0) wsum[wave] = __popcll(bal);
        __syncthreads();
        int off = top + __popcll(bal & ((1ull << lane) - 1ull));
        for (int w = 0; w < wave; w++) off += wsum[w];
        if (freed) stack[off] = m;
        top += wsum[0] + wsum[1] + wsum[2] + wsum[3];
        __syncthreads();
    }
    if (threadIdx.x == 0) hdr[kMpTop] = top;
}

// ---- the chain's per-pair stages ------------------------------------------------------------------------------------------
// camera-space point at the rounded keypoint (the matcher's xyz convention, no gate; a tracked keypoint passed the matcher's
// pixel test when it entered the memory, an out-of-image one gives zeros)
__device__ __forceinline__ float3 corres_point(const CorresDims &C, const float *depth, float2 kp)
{
    const float u = roundf(kp.x), v = roundf(kp.y);
    if (!(u >= 0.0f && u < (float)C.W && v >= 0.0f && v < (float)C.H)) return make_float3(0.f, 0.f, 0.f);
    const int x = (int)u, y = (int)v;
    return backproject(C.Kinv.m, x, y, depth[(size_t)y * C.W + x]);
}

// ordered compaction helper: position of this lane's flag among the flags of the workgroup's 256 lanes; total in *total
__device__ __forceinline__ int wg_prefix(bool flag, int *wsum, int &total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long bal = __ballot(flag);
    if (lane == 0) wsum[wave] = __popcll(bal);
    __syncthreads();
    int off = __popcll(bal & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; w++) off += wsum[w];
    total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();
    return off;
}

// one workgroup of 256, pair p.  Steps 1-3 of findCorres: the NN matches into the working list, the FAIL gate of the NN stage,
// propagation along the map points (non-neighbours), the RANSAC point count.  meta[2p] = active (A not FAIL), meta[2p+1] = list length.
__global__ void __launch_bounds__(256) k_corres_prop(CorresDims C, int p, const CorresFrame *__restrict__ F, const CorresPair *__restrict__ P,
                                                     const MpSlot *__restrict__ S, const int *__restrict__ img,
                                                     const btba_match *__restrict__ nn, const float4 *__restrict__ nn_pa, const float4 *__restrict__ nn_pb,
                                                     const int *__restrict__ nn_cnt, const int *__restrict__ nn_off, int *__restrict__ status,
                                                     btba_match *__restrict__ list, float4 *__restrict__ la, float4 *__restrict__ lb,
                                                     int *__restrict__ meta, int *__restrict__ roff, unsigned long long *__restrict__ best, int *__restrict__ stage)
{
    __shared__ unsigned bitA[kMatchMaxKpts / 32], bitB[kMatchMaxKpts / 32];
    __shared__ int firstB[kMatchMaxKpts];
    __shared__ int wsum[4];
    __shared__ int s_active;
    const int tid = threadIdx.x;
    const CorresPair pr = P[p];
    const CorresFrame &fa = F[pr.a], &fb = F[pr.b];
    const MpSlot sa = S[fa.slot], sb = S[fb.slot];
    const int n0 = nn_cnt[p], o0 = nn_off[p];
    if (tid == 0) {
        int st = status[pr.a];
        if (st == 0 && sa.n > 0 && sb.n > 0 && pr.neighbor && n0 < 5) { st = 1; status[pr.a] = 1; }
        s_active = st == 0;
    }
    for (int w = tid; w < kMatchMaxKpts / 32; w += 256) { bitA[w] = 0u; bitB[w] = 0u; }
    for (int k = tid; k < sb.n; k += 256) firstB[k] = INT_MAX;
    __syncthreads();
    const bool active = s_active != 0;
    for (int i = tid; i < n0; i += 256) {
        const btba_match m = nn[o0 + i];
        list[pr.base + i] = m;
        la[pr.base + i] = nn_pa[o0 + i];
        lb[pr.base + i] = nn_pb[o0 + i];
        const int ka = sa.canon[m.idx_a], kb = sb.canon[m.idx_b];
        atomicOr(&bitA[ka >> 5], 1u << (ka & 31));
        atomicOr(&bitB[kb >> 5], 1u << (kb & 31));
    }
    __syncthreads();
    int n1 = n0;
    if (active && !pr.neighbor) {
        // first pass: the lowest walk rank per B key among the candidates no NN match excludes
        for (int r = tid; r < sa.n; r += 256) {
            const int k = sa.order[r];
            if (k < 0) continue;
            const int mp = sa.map[k];
            if (mp < 0) continue;
            const int kb = img[(size_t)mp * C.slot_cap + fb.slot];
            if (kb < 0 || ((bitA[k >> 5] >> (k & 31)) & 1u) || ((bitB[kb >> 5] >> (kb & 31)) & 1u)) continue;
            atomicMin(&firstB[kb], r);
        }
        __syncthreads();
        // second pass: the survivors in walk order, appended behind the NN matches
        for (int r0 = 0; r0 < sa.n; r0 += 256) {
            const int r = r0 + tid;
            int k = -1, kb = -1;
            if (r < sa.n) {
                k = sa.order[r];
                const int mp = k >= 0 ? sa.map[k] : -1;
                kb = mp >= 0 ? img[(size_t)mp * C.slot_cap + fb.slot] : -1;
            }
            const bool keep = kb >= 0 && firstB[kb] == r;
            int total;
            const int pos = n1 + wg_prefix(keep, wsum, total);
            if (keep) {
                const float3 pa = corres_point(C, fa.depth, sa.kpts[k]), pb = corres_point(C, fb.depth, sb.kpts[kb]);
                btba_match m;
                m.idx_a = k; m.idx_b = kb; m.dist = -1.0f; m.dir = 2;
                m.ptA_cam[0] = pa.x; m.ptA_cam[1] = pa.y; m.ptA_cam[2] = pa.z;
                m.ptB_cam[0] = pb.x; m.ptB_cam[1] = pb.y; m.ptB_cam[2] = pb.z;
                list[pr.base + pos] = m;
                const float3 PA = match_model_point(fa.pose, pa), PB = match_model_point(fb.pose, pb);
                la[pr.base + pos] = make_float4(PA.x, PA.y, PA.z, 1.0f);
                lb[pr.base + pos] = make_float4(PB.x, PB.y, PB.z, 1.0f);
            }
            n1 += total;
        }
    }
    if (tid == 0) {
        meta[2 * p] = active ? 1 : 0;
        meta[2 * p + 1] = n1;
        roff[2 * p] = 0;
        roff[2 * p + 1] = (active && n1 > 5) ? n1 : 0;      // <= 5 matches: cleared without RANSAC (:574-578)
        best[p] = 0ull;
        stage[4 * p] = n0;
        stage[4 * p + 1] = n1;
    }
}

// one workgroup of 256, pair p.  Steps 4-7: the RANSAC inliers (in ascending order), the map-point update, the final gate, the
// pair's records at out[out_off[p]].  The update goes in chunks of 256 matches: a match whose A key and B key occur in no earlier
// lane of its chunk decides from the chunk's starting state (nothing before it in the chunk touches its keys), all such lanes
// at once; the others follow one by one in order.  img[A] of a shared map point is written afterwards by the highest match
// index that targets it (integer atomicMax on a per-map-point stamp), which is the sequential rule's last writer.
__global__ void __launch_bounds__(256) k_corres_update(CorresDims C, int p, const CorresFrame *__restrict__ F, const CorresPair *__restrict__ P,
                                                       const MpSlot *__restrict__ S, int *__restrict__ img, int *__restrict__ stamp,
                                                       int *__restrict__ hdr, int *__restrict__ stack, int *__restrict__ status,
                                                       const btba_match *__restrict__ list, const int *__restrict__ meta, const int *__restrict__ ids,
                                                       const int *__restrict__ nin, int *__restrict__ upd_mp, int *__restrict__ upd_a,
                                                       btba_match *__restrict__ out, int *__restrict__ out_off, int *__restrict__ n_out, int *__restrict__ stage)
{
    __shared__ int mapA[kMatchMaxKpts], mapB[kMatchMaxKpts];
    __shared__ int firstA[kMatchMaxKpts], firstB[kMatchMaxKpts];
    __shared__ int cka[256], ckb[256], cconf[256];
    __shared__ int wsum[4];
    __shared__ int s_next, s_top, s_err;
    const int tid = threadIdx.x;
    const CorresPair pr = P[p];
    const int slotA = F[pr.a].slot, slotB = F[pr.b].slot;
    const MpSlot sa = S[slotA], sb = S[slotB];
    const int active = meta[2 * p], n1 = meta[2 * p + 1], base = pr.base, o = out_off[p];
    if (!active) {                                  // A is FAIL: the matches stay as the NN stage left them (:185-188)
        for (int i = tid; i < n1; i += 256) out[o + i] = list[base + i];
        if (tid == 0) { out_off[p + 1] = o + n1; n_out[p] = n1; stage[4 * p + 2] = n1; stage[4 * p + 3] = n1; }
        return;
    }
    int n2 = n1 > 5 ? nin[p] : 0;
    if (n2 < 5) n2 = 0;                             // :728-731
    for (int k = tid; k < sa.n; k += 256) { mapA[k] = sa.map[k]; firstA[k] = INT_MAX; }
    for (int k = tid; k < sb.n; k += 256) { mapB[k] = sb.map[k]; firstB[k] = INT_MAX; }
    if (tid == 0) { s_next = hdr[kMpNext]; s_top = hdr[kMpTop]; s_err = 0; }
    __syncthreads();
    for (int c0 = 0; c0 < n2; c0 += 256) {
        const int j = c0 + tid;
        const bool valid = j < n2;
        int ka = 0, kb = 0;
        if (valid) {
            const btba_match m = list[base + ids[base + j]];
            ka = sa.canon[m.idx_a]; kb = sb.canon[m.idx_b];
            atomicMin(&firstA[ka], tid);
            atomicMin(&firstB[kb], tid);
        }
        __syncthreads();
        const bool conf = valid && (firstA[ka] != tid || firstB[kb] != tid);
        const bool par = valid && !conf;
        const bool hasA = par && mapA[ka] >= 0, hasB = par && mapB[kb] >= 0;
        const bool skip = hasA && hasB;
        const bool create = par && !hasB;
        const int next0 = s_next, top0 = s_top;
        int n_create;
        const int r = wg_prefix(create, wsum, n_create);
        if (par) {
            int mp = -1;
            if (!skip) {
                if (create) {
                    mp = r < top0 ? stack[top0 - 1 - r] : next0 + (r - top0);
                    if (mp >= C.mp_cap) { s_err = 1; mp = -1; }
                    else { mapB[kb] = mp; img[(size_t)mp * C.slot_cap + slotB] = kb; }
                } else {
                    mp = mapB[kb];
                }
                if (mp >= 0) mapA[ka] = mp;
            }
            upd_mp[base + j] = mp;
            upd_a[base + j] = ka;
        }
        cka[tid] = ka; ckb[tid] = kb; cconf[tid] = conf ? 1 : 0;
        __syncthreads();
        if (tid == 0) {
            int next = next0 + max(n_create - top0, 0), top = max(top0 - n_create, 0);
            for (int l = 0; l < 256; l++) {
                if (!cconf[l]) continue;
                const int a = cka[l], b = ckb[l];
                int mp = -1;
                if (!(mapA[a] >= 0 && mapB[b] >= 0)) {
                    if (mapB[b] < 0) {
                        mp = top > 0 ? stack[--top] : next++;
                        if (mp >= C.mp_cap) { s_err = 1; mp = -1; next--; }
                        else { mapB[b] = mp; img[(size_t)mp * C.slot_cap + slotB] = b; }
                    } else {
                        mp = mapB[b];
                    }
                    if (mp >= 0) mapA[a] = mp;
                }
                upd_mp[base + c0 + l] = mp;
                upd_a[base + c0 + l] = a;
            }
            s_next = next; s_top = top;
        }
        __syncthreads();
        if (valid) { firstA[ka] = INT_MAX; firstB[kb] = INT_MAX; }
        __syncthreads();
    }
    // img[A] of every touched map point = the A key of the highest match index that targets it
    __threadfence();
    __syncthreads();
    for (int j = tid; j < n2; j += 256) { const int mp = upd_mp[base + j]; if (mp >= 0) atomicMax(&stamp[mp], j); }
    __threadfence();
    __syncthreads();
    for (int j = tid; j < n2; j += 256) {
        const int mp = upd_mp[base + j];
        if (mp >= 0 && __hip_atomic_load(&stamp[mp], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == j) img[(size_t)mp * C.slot_cap + slotA] = upd_a[base + j];
    }
    __threadfence();
    __syncthreads();
    for (int j = tid; j < n2; j += 256) { const int mp = upd_mp[base + j]; if (mp >= 0) atomicExch(&stamp[mp], -1); }
    for (int k = tid; k < sa.n; k += 256) sa.map[k] = mapA[k];
    for (int k = tid; k < sb.n; k += 256) sb.map[k] = mapB[k];
    // final gate (:232-240): after RANSAC the list holds 0 or >= 5 matches
    const int n3 = n2 < 5 ? 0 : n2;
    for (int i = tid; i < n3; i += 256) out[o + i] = list[base + ids[base + i]];
    if (tid == 0) {
        if (n3 == 0 && pr.neighbor) status[pr.a] = 1;
        hdr[kMpNext] = s_next; hdr[kMpTop] = s_top;
        if (s_err) hdr[kMpErr] = 1;
        out_off[p + 1] = o + n3; n_out[p] = n3;
        stage[4 * p + 2] = n2; stage[4 * p + 3] = n3;
    }
}

}  // namespace btba
