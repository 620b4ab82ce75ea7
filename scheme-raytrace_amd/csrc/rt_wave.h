// rt_wave.h — wave64 helpers the device translation units share (rt_kernels.hip, rt_frame.hip).
// Device code only: the host translation units do not include it.
#pragma once
#include <hip/hip_runtime.h>

namespace rtamd {

// the number of set bits of m below this lane's
__device__ __forceinline__ uint32_t lanes_below(unsigned long long m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

}  // namespace rtamd
