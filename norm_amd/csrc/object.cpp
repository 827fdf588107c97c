// object.cpp -- the FEC block partition of a NORM data object, on the host (no GPU, no codec).
//
// NormObject::Open's arithmetic for non-stream objects (reference src/common/normObject.cpp:134-137,
// :203-231; NORM spec 5.1.1, the large / small blocks of RFC 5052), and the segment rule of
// NormDataObject::ReadSegment / WriteSegment (:2673-2718, :2628-2670), which object_layout.hpp
// shares with the kernels of kernels_obj.hip.
#include "nfec_internal.hpp"
#include "object_layout.hpp"

using namespace nfec;

namespace {

// NormObjectSize's divide: it rounds up (and must not overflow near 2^64)
inline uint64_t div_up(uint64_t a, uint64_t b) { return a / b + (a % b != 0); }

}  // namespace

extern "C" int nfec_object_layout_for(uint64_t object_size, uint32_t segment_size, uint32_t num_data,
                                      nfec_object_layout* out)
{
    if (!out) return fail(NFEC_EINVAL, "object_layout_for: null out");
    if (object_size == 0) return fail(NFEC_EINVAL, "object_layout_for: object_size of 0");
    if (segment_size == 0 || segment_size > 65535) return fail(NFEC_EINVAL, "object_layout_for: segment_size outside [1, 65535]");
    if (num_data == 0 || num_data > 65535) return fail(NFEC_EINVAL, "object_layout_for: num_data outside [1, 65535]");
    const uint64_t num_segments = div_up(object_size, segment_size);
    const uint64_t num_blocks = div_up(num_segments, num_data);
    if (num_blocks > 0xffffffffull) return fail(NFEC_ERANGE, "object_layout_for: more than 2^32 - 1 blocks");
    nfec_object_layout L{};
    L.object_size = object_size;
    L.segment_size = segment_size;
    L.num_data = num_data;
    L.num_segments = num_segments;
    L.num_blocks = (uint32_t)num_blocks;
    L.large_block_size = (uint32_t)div_up(num_segments, num_blocks);
    if (num_segments == num_blocks * L.large_block_size) {
        L.small_block_size = L.large_block_size;
        L.small_block_count = L.num_blocks;
        L.large_block_count = 0;
    } else {
        L.small_block_size = L.large_block_size - 1u;
        L.large_block_count = (uint32_t)(num_segments - num_blocks * L.small_block_size);
        L.small_block_count = L.num_blocks - L.large_block_count;
    }
    L.final_block_id = L.large_block_count + L.small_block_count - 1u;
    L.final_segment_size = (uint32_t)(object_size - (num_segments - 1u) * segment_size);
    *out = L;
    return NFEC_OK;
}

extern "C" int nfec_object_segment(const nfec_object_layout* layout, uint32_t block, uint32_t segment, uint64_t* offset,
                                   uint32_t* length)
{
    if (!layout) return fail(NFEC_EINVAL, "object_segment: null layout");
    if (block >= layout->num_blocks) return fail(NFEC_ERANGE, "object_segment: block outside the object");
    if (segment >= object_block_size(*layout, block)) return fail(NFEC_ERANGE, "object_segment: segment outside its block");
    uint64_t off;
    uint32_t len;
    object_segment_at(*layout, block, segment, &off, &len);
    if (offset) *offset = off;
    if (length) *length = len;
    return NFEC_OK;
}

extern "C" int nfec_object_block_sizes(const nfec_object_layout* layout, uint32_t first_block, uint32_t nblocks,
                                       uint16_t* num_data_out)
{
    if (!layout) return fail(NFEC_EINVAL, "object_block_sizes: null layout");
    if ((uint64_t)first_block + nblocks > layout->num_blocks)
        return fail(NFEC_ERANGE, "object_block_sizes: first_block + nblocks > num_blocks");
    if (nblocks && !num_data_out) return fail(NFEC_EINVAL, "object_block_sizes: null num_data_out");
    for (uint32_t i = 0; i < nblocks; ++i) num_data_out[i] = (uint16_t)object_block_size(*layout, first_block + i);
    return NFEC_OK;
}
