/* sfr_host_shim.cpp — what csrc/cooling_host.hip and csrc/sfr_host.hip need to link into a shared library of their own
 * (sfr_cases.build_nudged: the host engine with SHQ_COOL_NUDGE), and the header's struct sizes as that compiler sees them. */
#include <stdint.h>
#include "shenqi_hip.h"

void shq_set_error(const char *, ...) {}

extern "C" void shq_sfr_struct_sizes(int64_t out[5])
{
    out[0] = (int64_t) sizeof(shq_sfr_params);
    out[1] = (int64_t) sizeof(shq_sfr_arrays);
    out[2] = (int64_t) sizeof(shq_sfr_eval_step);
    out[3] = (int64_t) sizeof(shq_sfr_fields);
    out[4] = (int64_t) sizeof(shq_sfr_result);
}
