// btba_lfnet_net.hpp -- what the kernels of both LF-Net nets (btba_lfnet_desc.hpp, btba_lfnet_det.hpp) share: the activation of
// tf_batch_norm_act (lf-net-release/common/tf_layer_utils.py:167-199) behind the batch norm that the host folded into (scale, shift).
#pragma once
#include <hip/hip_runtime.h>

namespace btba {

constexpr int kLfnetActRelu = 0, kLfnetActLeaky = 1, kLfnetActNone = 2;

__device__ inline float lfnet_act(float v, int act, float alpha)
{
    if (act == kLfnetActRelu) return fmaxf(v, 0.0f);
    if (act == kLfnetActLeaky) return v >= 0.0f ? v : alpha * v;
    return v;
}

// act(v * scale[c .. c + 3] + shift[c .. c + 3]) on four consecutive channels
__device__ inline float4 lfnet_bn_act4(float4 v, const float *__restrict__ scale, const float *__restrict__ shift, int c, int act, float alpha)
{
    const float4 sc = *reinterpret_cast<const float4 *>(scale + c), sh = *reinterpret_cast<const float4 *>(shift + c);
    v.x = lfnet_act(fmaf(v.x, sc.x, sh.x), act, alpha); v.y = lfnet_act(fmaf(v.y, sc.y, sh.y), act, alpha);
    v.z = lfnet_act(fmaf(v.z, sc.z, sh.z), act, alpha); v.w = lfnet_act(fmaf(v.w, sc.w, sh.w), act, alpha);
    return v;
}

}  // namespace btba
