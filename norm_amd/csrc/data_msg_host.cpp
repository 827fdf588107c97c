// data_msg_host.cpp -- the host twins of the NORM_DATA message calls (nfec.h, "NORM_DATA messages
// on the device"): no GPU, no codec.  The header words and the parse are data_msg.hpp's, the code
// tx_emit_data_kernel and rx_ingest_data_kernel run; this file moves bytes in and out of them and
// holds the argument checks the device entries share.
#include "data_msg.hpp"
#include "nfec_internal.hpp"

using namespace nfec;

namespace nfec {

// the call's constants out of the caller's struct; NFEC_EINVAL for what nfec_tx_emit_data refuses
int data_header_fixed_from(const nfec_data_header* h, DataHeaderFixed& f)
{
    if (!h) return fail(NFEC_EINVAL, "data header: null header");
    const uint32_t kind = payload_id_kind(h->fec_id, h->fec_m);
    if (kind == PAYLOAD_ID_NONE) return fail(NFEC_EINVAL, "data header: bad fec_id / fec_m");
    if (h->ext_bytes != 0 && h->ext_bytes != data_fti_length(h->fec_id))
        return fail(NFEC_EINVAL, "data header: ext_bytes is neither 0 nor the FTI's length");
    if (h->backoff > 15 || h->gsize > 15) return fail(NFEC_EINVAL, "data header: backoff or gsize above 15");
    data_header_fixed(f, h->source_id, h->instance_id, h->grtt, h->backoff, h->gsize, h->flags, h->fec_id, h->object_id);
    for (uint32_t j = 0; j < 4; ++j) {
        f.ext[j] = 0;
        for (uint32_t t = 0; t < 4; ++t)
            if (4 * j + t < h->ext_bytes) f.ext[j] |= (uint32_t)h->ext[4 * j + t] << (8u * t);
    }
    f.ext_bytes = h->ext_bytes;
    f.first_sequence = h->first_sequence;
    f.id_kind = kind;
    f.hdr_bytes = kDataBase + payload_id_length(kind) + h->ext_bytes;
    return NFEC_OK;
}

int data_filter_from(const nfec_data_filter* in, DataFilter& f)
{
    if (!in) return fail(NFEC_EINVAL, "data filter: null filter");
    f.id_kind = payload_id_kind(in->fec_id, in->fec_m);
    if (f.id_kind == PAYLOAD_ID_NONE) return fail(NFEC_EINVAL, "data filter: bad fec_id / fec_m");
    f.source_id = in->source_id;
    f.instance_id = in->instance_id;
    f.fec_id = in->fec_id;
    f.object_id = in->object_id;
    return NFEC_OK;
}

}  // namespace nfec

extern "C" int nfec_data_header_bytes(uint8_t fec_id, uint8_t ext_bytes)
{
    const uint32_t idlen = data_id_length(fec_id);
    if (!idlen) return fail(NFEC_EINVAL, "data_header_bytes: unknown fec_id");
    if (ext_bytes != 0 && ext_bytes != data_fti_length(fec_id))
        return fail(NFEC_EINVAL, "data_header_bytes: ext_bytes is neither 0 nor the FTI's length");
    return (int)(kDataBase + idlen + ext_bytes);
}

extern "C" int nfec_data_header_write_host(const nfec_data_header* header, uint32_t i, uint32_t block_id, uint16_t symbol,
                                           uint16_t block_len, void* out, size_t cap)
{
    DataHeaderFixed f;
    const int rc = data_header_fixed_from(header, f);
    if (rc) return rc;
    if (!out) return fail(NFEC_EINVAL, "data_header_write_host: null out");
    if (cap < f.hdr_bytes) return fail(NFEC_EINVAL, "data_header_write_host: cap below the header's length");
    uint32_t w[kDataHeaderWords];
    data_header_words(f, i, payload_id(f.id_kind, block_id, symbol, block_len), w);
    uint8_t* b = static_cast<uint8_t*>(out);
    for (uint32_t j = 0; j < f.hdr_bytes; ++j) b[j] = (uint8_t)(w[j >> 2] >> (8u * (j & 3u)));
    return (int)f.hdr_bytes;
}

// The datagram's first bytes are gathered into the words data_parse takes (byte t of word j in bits
// [8t, 8t + 8)), whatever the host's byte order; bytes past the datagram's length stay zero and
// are not read from the wire.
extern "C" int nfec_rx_parse_data_host(const nfec_data_filter* filter, uint32_t first_block_id, const void* wire,
                                       uint64_t wire_bytes, const uint64_t* offsets, const uint16_t* length,
                                       uint32_t count, uint8_t* class_out, uint16_t* sequence_out,
                                       uint32_t* block_index_out, uint16_t* symbol_id_out, uint16_t* block_len_out,
                                       uint64_t* payload_offset_out, uint16_t* payload_length_out,
                                       uint64_t* fti_index_out)
{
    DataFilter f;
    const int rc = data_filter_from(filter, f);
    if (rc) return rc;
    if (fti_index_out) *fti_index_out = ~(uint64_t)0;
    if (count == 0) return 0;
    if (count > 0x7fffffffu) return fail(NFEC_ERANGE, "rx_parse_data_host: count above 2^31 - 1");
    if (!wire) return fail(NFEC_EINVAL, "rx_parse_data_host: null wire");
    if (!offsets) return fail(NFEC_EINVAL, "rx_parse_data_host: null offsets");
    if (!length) return fail(NFEC_EINVAL, "rx_parse_data_host: null length");
    const uint8_t* bytes = static_cast<const uint8_t*>(wire);
    int parsed = 0;
    bool fti_seen = false;
    for (uint32_t i = 0; i < count; ++i) {
        const uint64_t off = offsets[i];
        const uint32_t len = length[i];
        uint32_t cls = DGRAM_UNREADABLE, plen = 0;
        uint64_t poff = 0;
        RxId id{0xffffffffu, 0xffffu, 0xffffu};
        if (data_readable(off, len, wire_bytes)) {
            uint32_t h[kParseWords] = {0, 0, 0, 0, 0, 0, 0};
            const uint32_t n = len < kParseBytes ? len : kParseBytes;
            for (uint32_t j = 0; j < n; ++j) h[j >> 2] |= (uint32_t)bytes[off + j] << (8u * (j & 3u));
            const DataParse p = data_parse(h, len, f, first_block_id);
            cls = p.cls;
            if (sequence_out) sequence_out[i] = (uint16_t)p.sequence;
            if (cls == DGRAM_PARSED) {
                id = p.id;
                poff = off + p.hdr_bytes, plen = len - p.hdr_bytes;
                ++parsed;
                if (p.fti && !fti_seen) {
                    fti_seen = true;
                    if (fti_index_out) *fti_index_out = i;
                }
            }
        }
        if (class_out) class_out[i] = (uint8_t)cls;
        if (block_index_out) block_index_out[i] = id.block;
        if (symbol_id_out) symbol_id_out[i] = (uint16_t)id.symbol;
        if (block_len_out) block_len_out[i] = (uint16_t)id.block_len;
        if (payload_offset_out) payload_offset_out[i] = poff;
        if (payload_length_out) payload_length_out[i] = (uint16_t)plen;
    }
    return parsed;
}

extern "C" int nfec_rx_data_chunks_host(uint64_t off, uint16_t length, uint64_t* chunk_out)
{
    const uint32_t n = data_chunk_count(off, length);
    for (uint32_t c = 0; c < n && chunk_out; ++c) chunk_out[c] = data_chunk_offset(off) + 16u * c;
    return (int)n;
}
