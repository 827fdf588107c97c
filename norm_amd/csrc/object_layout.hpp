// object_layout.hpp -- the segment rule of a NORM data object (nfec.h, "object segmentation on the
// device"), shared by the host entries (object.cpp) and the kernels (kernels_obj.hip): what the
// CPU tests check of the 64-bit offsets is what the kernels compute.
#pragma once

#include <stdint.h>

#include "nfec.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NFEC_HD __host__ __device__
#else
#define NFEC_HD
#endif

namespace nfec {

// NormObject::GetBlockSize: the large blocks come first
NFEC_HD inline uint32_t object_block_size(const nfec_object_layout& L, uint32_t block)
{
    return block < L.large_block_count ? L.large_block_size : L.small_block_size;
}

// ReadSegment's / WriteSegment's length rule (reference src/common/normObject.cpp:2682-2694,
// :2637-2648): segment_size, except final_segment_size for the last segment of the final block.
NFEC_HD inline uint32_t object_segment_length(const nfec_object_layout& L, uint32_t block, uint32_t segment)
{
    return block == L.final_block_id && segment + 1u == object_block_size(L, block) ? L.final_segment_size
                                                                                    : L.segment_size;
}

// NormDataObject::ReadSegment / WriteSegment (:2696-2709, :2649-2662): the byte offset and the length
// of segment `segment` of block `block`.  The caller has checked block < num_blocks and segment <
// object_block_size(block); the offset is then below object_size, so nothing here leaves 64 bits.
// The segments of one block lie one behind the other: segment s + j starts j * segment_size bytes
// past segment s.  The kernels take a run's first offset from here and step through the run by that.
NFEC_HD inline void object_segment_at(const nfec_object_layout& L, uint32_t block, uint32_t segment, uint64_t* offset,
                                      uint32_t* length)
{
    const uint64_t seg = L.segment_size;
    const uint64_t large_len = (uint64_t)L.large_block_size * seg, small_len = (uint64_t)L.small_block_size * seg;
    uint64_t off;
    if (block < L.large_block_count) off = large_len * block + seg * segment;
    else off = large_len * L.large_block_count + small_len * (block - L.large_block_count) + seg * segment;
    *offset = off;
    *length = object_segment_length(L, block, segment);
}

// The kernels split a lane's first flat index f < 256 into f / d and f % d (d: 16-byte pieces per
// segment, at most 2^13) by one multiply: with magic = ceil(2^32 / d) the error magic * d - 2^32
// is below d, so f * error < 2^21 < 2^32 and (f * magic) >> 32 == f / d exactly.  d == 1 has no
// 32-bit magic: 0 stands for it.
inline uint32_t div_magic32(uint32_t d) { return d <= 1u ? 0u : (uint32_t)(((1ull << 32) + d - 1u) / d); }
NFEC_HD inline uint32_t div_by_magic32(uint32_t f, uint32_t magic)
{
    return magic ? (uint32_t)(((uint64_t)f * magic) >> 32) : f;
}

}  // namespace nfec
