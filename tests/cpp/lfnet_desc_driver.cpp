// lfnet_desc_driver.cpp -- ctypes entry into the C++ host layer's descriptor net (tests/test_gpu_lfnet_desc.py): a btba::LfnetDescriptor
// made from the caller's host arrays, run on caller-owned device buffers either through describe() or as the LfnetDetector::DescFn
// that asDescNet() hands out.
#include <hip/hip_runtime_api.h>

#include "../../bundletrack_amd/cpp/btba_host.hpp"

// via_desc_net: 0 = describe(n_frames, slots, ...), 1 = the DescFn on frame 0's `slots` patches (n_kpts_dev is not used).
// Returns 0, a btba status, or -1 when the DescFn reports a wrong pointer or dimension.
extern "C" __attribute__((visibility("default"))) int lfnet_desc_driver(void *ws, const btba_lfnet_desc_config *config,
                                                                         const btba_lfnet_desc_weights *weights, int n_frames, int slots,
                                                                         const float *patches_dev, const int32_t *n_kpts_dev, float *desc_dev,
                                                                         int via_desc_net)
{
    try {
        const btba::LfnetDescriptor net(static_cast<btba_workspace *>(ws), *config, *weights);
        if (via_desc_net) {
            const btba::LfnetDetector::DescFn fn = net.asDescNet(desc_dev);
            int dim = 0;
            const float *got = fn(patches_dev, slots, dim);
            if (got != desc_dev || dim != config->out_dim) return -1;
        } else {
            net.describe(n_frames, slots, patches_dev, n_kpts_dev, desc_dev);
        }
        // the model is destroyed on return: its destructor waits for the device
        return 0;
    } catch (const btba::Error &e) {
        return e.status;
    }
}
