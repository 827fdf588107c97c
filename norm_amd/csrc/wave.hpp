// wave.hpp -- wave-level helpers of the hand-written kernels (device code only).
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

namespace nfec {

// a value every lane of the wave holds alike, into scalar registers
__device__ __forceinline__ uint32_t uniform(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint64_t uniform64(uint64_t v)
{
    return ((uint64_t)uniform((uint32_t)(v >> 32)) << 32) | uniform((uint32_t)v);
}

__device__ __forceinline__ uint32_t lane_up(uint32_t v, uint32_t d) { return __shfl_up(v, d, 64); }
__device__ __forceinline__ uint64_t lane_up(uint64_t v, uint32_t d) { return __shfl_up((unsigned long long)v, d, 64); }

// inclusive prefix sum of v over the wave's 64 lanes (lane 63 holds the total)
template <typename T>
__device__ __forceinline__ T wave_scan(T v, uint32_t lane)
{
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const T up = lane_up(v, d);
        if (lane >= d) v += up;
    }
    return v;
}

}  // namespace nfec
