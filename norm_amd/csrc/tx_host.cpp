// tx_host.cpp -- the transmission list from NORM's per-block pending masks, on the host (no GPU).
//
// The walk NormObject::NextSenderMsg makes once a block's parity exists (reference
// src/common/normObject.cpp:1877, :1989): blocks ascending, within a block the pending slots
// ascending; a source segment at its own length, a parity segment at the block's seg_size_max, the
// longest of its source segments whether pending or not (:2035, :2050, :2071).  The kernels of
// nfec_tx_list (kernels_tx.hip) apply the same rule to masks in device memory.
#include "nfec_internal.hpp"

using namespace nfec;

extern "C" int nfec_tx_list_host(uint32_t k, uint32_t m, uint32_t vector_size, const uint32_t* pending,
                                 uint32_t mask_stride, const uint16_t* num_data, uint32_t nblocks,
                                 const uint16_t* seg_length, uint32_t length_stride, uint32_t gap, uint64_t* offsets,
                                 uint32_t* block_index, uint16_t* symbol_id, uint16_t* length, uint32_t capacity,
                                 uint64_t* block_start)
{
    if (k == 0 || m == 0 || (uint64_t)k + m > 65536) return fail(NFEC_EINVAL, "tx_list_host: bad k or m");
    if (vector_size == 0 || vector_size > 65535) return fail(NFEC_EINVAL, "tx_list_host: bad vector_size");
    if ((uint64_t)mask_stride * 32u < (uint64_t)k + m)
        return fail(NFEC_EINVAL, "tx_list_host: mask_stride smaller than (k + m + 31) / 32");
    if (seg_length && length_stride < k) return fail(NFEC_EINVAL, "tx_list_host: length_stride < k");
    if (!block_start) return fail(NFEC_EINVAL, "tx_list_host: null block_start");
    if (capacity && (!offsets || !block_index || !symbol_id || !length))
        return fail(NFEC_EINVAL, "tx_list_host: null output array");
    if (nblocks && !pending) return fail(NFEC_EINVAL, "tx_list_host: null pending mask");
    uint64_t count = 0, bytes = 0;
    for (uint32_t b = 0; b < nblocks; ++b) {
        block_start[2 * (size_t)b] = count;
        block_start[2 * (size_t)b + 1] = bytes;
        const uint32_t nd = num_data ? num_data[b] : k;
        if (nd < 1 || nd > k) continue;
        const uint32_t* mask = pending + (size_t)b * mask_stride;
        const uint16_t* lens = seg_length ? seg_length + (size_t)b * length_stride : nullptr;
        uint32_t smax = vector_size;
        if (lens) {
            smax = 0;
            for (uint32_t s = 0; s < nd; ++s) smax = lens[s] > smax ? lens[s] : smax;
        }
        for (uint32_t s = 0; s < nd + m; ++s) {
            if (!((mask[s >> 5] >> (s & 31u)) & 1u)) continue;
            const uint32_t len = s >= nd ? smax : lens ? lens[s] : vector_size;
            if (count < capacity) {
                offsets[count] = bytes + gap;
                block_index[count] = b;
                symbol_id[count] = (uint16_t)s;
                length[count] = (uint16_t)len;
            }
            ++count;
            bytes += (uint64_t)gap + len;
        }
    }
    block_start[2 * (size_t)nblocks] = count;
    block_start[2 * (size_t)nblocks + 1] = bytes;
    return NFEC_OK;
}
