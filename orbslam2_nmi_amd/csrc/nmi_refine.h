// nmi_refine.h -- internal: refined peaks of a rating table (include/nmi_hip.h, "Refined peaks"; nmi_refine.hip).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "nmi_refine_rule.h"

namespace nmi {

// One call: the table and its shape (axis order of nmi_host.h; cells = the product of num, below 2^32 - 1), K in 1..kRefineMaxK,
// the K keys -- a device array, or, when keys is null, host_keys, which travel in the launch's arguments -- and where the K records
// go: a device array, a mapped host array, or both.  post (optional, mapped host memory, K words): word k receives seq once record
// k is written, for a host that polls.
struct RefineArgs {
    const float *ratings = nullptr;
    int32_t num[6] = {1, 1, 1, 1, 1, 1};
    uint32_t cells = 0;
    int32_t K = 0;
    const unsigned long long *keys = nullptr;
    nmi_refined_peak *out = nullptr, *out_host = nullptr;
    unsigned long long *post = nullptr;
    unsigned long long seq = 0;
    unsigned long long host_keys[kRefineMaxK] = {};
};

hipError_t launch_refine(const RefineArgs &a, hipStream_t stream);

}  // namespace nmi
