// message_wave.hpp -- what the one-wave-per-message kernels share (rx_place_kernel, rx_ingest_kernel,
// tx_emit_kernel; device code only): a few thousand workgroups of four waves, each wave taking
// messages wave, wave + nwaves, ... one at a time and adding its counts to `stats` once, at its end.
#pragma once

#include "nfec_internal.hpp"
#include "wave.hpp"

namespace nfec {

// the messages a call takes: min(count, *count_dev) where the caller left a count on the device
__device__ __forceinline__ uint64_t message_count(uint32_t count, const uint64_t* __restrict__ count_dev)
{
    return count_dev ? min((uint64_t)count, uniform64(*count_dev)) : (uint64_t)count;
}

// One entry of a segment list.  Every lane reads the same words (one request each); a wave requests
// the next entry before it copies this one, so the latency hides behind the copy.
struct Descriptor {
    uint32_t b = 0, s = 0, len = 0;
    uint64_t off = 0;
    template <typename Args>
    __device__ __forceinline__ void request(const Args& a, uint64_t i)
    {
        b = a.block_index[i], s = a.symbol_id[i], len = a.length[i], off = a.offsets[i];
    }
    // the entry in scalar registers
    __device__ __forceinline__ Descriptor taken() const
    {
        Descriptor d;
        d.b = uniform(b), d.s = uniform(s), d.len = uniform(len), d.off = uniform64(off);
        return d;
    }
};

// the numData (>= 1) of block b when the batch has a slot s of block b, else 0 (b and s wave-uniform)
__device__ __forceinline__ uint32_t slot_num_data(const BatchView& v, uint32_t b, uint32_t s)
{
    if (b >= v.nblocks) return 0;
    const uint32_t nd = v.num_data ? uniform(v.num_data[b]) : v.k;
    return nd >= 1 && nd <= v.k && s < nd + v.m ? nd : 0;
}

__device__ __forceinline__ uint8_t* slot_address(const BatchView& v, uint32_t b, uint32_t s)
{
    return v.base + (uint64_t)b * v.block_stride + (uint64_t)s * v.seg_stride;
}

// lane 0 sets the slot's bit of the block's mask; whether it was set before goes to the whole wave
__device__ __forceinline__ bool claim_slot(uint32_t* __restrict__ mask, uint32_t mask_stride, uint32_t b, uint32_t s,
                                           uint32_t lane)
{
    uint32_t was = 0;
    if (lane == 0) {
        const uint32_t bit = 1u << (s & 31u);
        was = atomicOr(mask + (uint64_t)b * mask_stride + (s >> 5), bit) & bit;
    }
    return __builtin_amdgcn_readlane(was, 0) != 0;
}

// the wave's counters into stats[0 .. 2]: one atomic per wave and counter that is not zero,
// instead of one per message on a single address
__device__ __forceinline__ void flush_stats(uint32_t* __restrict__ stats, uint32_t lane, uint32_t n0, uint32_t n1,
                                            uint32_t n2 = 0)
{
    if (!stats || lane != 0) return;
    if (n0) atomicAdd(stats + 0, n0);
    if (n1) atomicAdd(stats + 1, n1);
    if (n2) atomicAdd(stats + 2, n2);
}

}  // namespace nfec
