// rx_host.cpp -- erasure lists from NORM's per-block reception masks, on the host (no GPU).
//
// The list NormObject::HandleObjectMessage builds before it calls Decode (reference
// src/common/normObject.cpp:1560-1606): the missing source slots ascending, then the missing
// parity slots; nothing for a block whose source is complete.  rx_erasures_kernel
// (kernels_rx.hip) applies the same rule to masks in device memory.
// Also the host form of the intake's parse (nfec_rx_parse_host): (block, slot) of each message from
// the FEC payload ID in front of its payload, by the code rx_ingest_kernel runs (rx_parse.hpp).
#include "nfec_internal.hpp"
#include "rx_parse.hpp"

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

// The parse half of the intake on host arrays: rx_parse.hpp's rule, message by message.  The ID's
// bytes are gathered into the two words rx_id_decode takes (byte j in bits [8j, 8j + 8)), whatever
// the host's byte order.
extern "C" int nfec_rx_parse_host(uint8_t fec_id, uint8_t fec_m, uint32_t first_block_id, const void* wire,
                                  uint64_t wire_bytes, const uint64_t* offsets, const uint16_t* length, uint32_t count,
                                  uint32_t* block_index_out, uint16_t* symbol_id_out, uint16_t* block_len_out)
{
    const uint32_t kind = payload_id_kind(fec_id, fec_m);
    if (kind == PAYLOAD_ID_NONE) return fail(NFEC_EINVAL, "rx_parse_host: bad fec_id / fec_m");
    if (count == 0) return 0;
    if (count > 0x7fffffffu) return fail(NFEC_ERANGE, "rx_parse_host: count above 2^31 - 1");
    if (!wire) return fail(NFEC_EINVAL, "rx_parse_host: null wire");
    if (!offsets) return fail(NFEC_EINVAL, "rx_parse_host: null offsets");
    if (!length) return fail(NFEC_EINVAL, "rx_parse_host: null length");
    const uint8_t* bytes = static_cast<const uint8_t*>(wire);
    const uint32_t idlen = payload_id_length(kind);
    int readable = 0;
    for (uint32_t i = 0; i < count; ++i) {
        RxId id{0xffffffffu, 0xffffu, 0xffffu};
        if (rx_readable(offsets[i], length[i], idlen, wire_bytes)) {
            const uint8_t* p = bytes + (offsets[i] - idlen);
            uint32_t w[2] = {0u, 0u};
            for (uint32_t j = 0; j < idlen; ++j) w[j >> 2] |= (uint32_t)p[j] << (8u * (j & 3u));
            id = rx_id_decode(kind, w[0], w[1], first_block_id);
            ++readable;
        }
        if (block_index_out) block_index_out[i] = id.block;
        if (symbol_id_out) symbol_id_out[i] = (uint16_t)id.symbol;
        if (block_len_out) block_len_out[i] = (uint16_t)id.block_len;
    }
    return readable;
}
