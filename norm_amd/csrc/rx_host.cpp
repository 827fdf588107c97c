// rx_host.cpp -- erasure lists from NORM's per-block reception masks, on the host (no GPU).
//
// The list NormObject::HandleObjectMessage builds before it calls Decode (reference
// src/common/normObject.cpp:1560-1606): the missing source slots ascending, then the missing
// parity slots; nothing for a block whose source is complete.  rx_erasures_kernel
// (kernels_rx.hip) applies the same rule to masks in device memory.
#include "nfec_internal.hpp"

using namespace nfec;

namespace {

inline bool received_bit(const uint32_t* mask, uint32_t slot) { return (mask[slot >> 5] >> (slot & 31u)) & 1u; }

}  // namespace

extern "C" int nfec_rx_erasures_host(uint32_t k, uint32_t m, const uint32_t* received, uint32_t mask_stride,
                                     const uint16_t* num_data, uint32_t nblocks, uint16_t* erasure_locs,
                                     uint32_t erasure_stride, uint16_t* erasure_counts)
{
    if (k == 0 || m == 0 || (uint64_t)k + m > 65536) return fail(NFEC_EINVAL, "rx_erasures_host: bad k or m");
    if ((uint64_t)mask_stride * 32u < (uint64_t)k + m)
        return fail(NFEC_EINVAL, "rx_erasures_host: mask_stride smaller than (k + m + 31) / 32");
    if (nblocks == 0) return NFEC_OK;
    if (!received) return fail(NFEC_EINVAL, "rx_erasures_host: null received mask");
    if (!erasure_locs && erasure_stride) return fail(NFEC_EINVAL, "rx_erasures_host: null erasure_locs");
    if (!erasure_counts) return fail(NFEC_EINVAL, "rx_erasures_host: null erasure_counts");
    for (uint32_t b = 0; b < nblocks; ++b) {
        const uint32_t nd = num_data ? num_data[b] : k;
        uint32_t count = 0;
        if (nd >= 1 && nd <= k) {
            const uint32_t* mask = received + (size_t)b * mask_stride;
            uint16_t* locs = erasure_locs + (size_t)b * erasure_stride;
            for (uint32_t s = 0; s < nd; ++s)
                if (!received_bit(mask, s)) {
                    if (count < erasure_stride) locs[count] = (uint16_t)s;
                    ++count;
                }
            if (count)
                for (uint32_t s = nd; s < nd + m; ++s)
                    if (!received_bit(mask, s)) {
                        if (count < erasure_stride) locs[count] = (uint16_t)s;
                        ++count;
                    }
        }
        erasure_counts[b] = (uint16_t)(count < 65535u ? count : 65535u);
    }
    return NFEC_OK;
}
