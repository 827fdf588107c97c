// rx_parse.hpp -- the FEC payload ID in front of a payload on the wire (nfec.h, "sender assembly
// on the device" and "receiver assembly on the device"): its layouts, how nfec_tx_emit writes one and
// what nfec_rx_ingest reads out of one, and which messages of a wire buffer can be read.  Shared by
// the host entry (nfec_rx_parse_host, rx_host.cpp), the ABI entries and the kernels (tx_emit_kernel,
// rx_ingest_kernel): what the CPU tests check of the decode is what the kernel runs.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NFEC_ID_HD __host__ __device__
#else
#define NFEC_ID_HD
#endif

namespace nfec {

// The payload ID's layout (NormPayloadId, reference include/normMessage.h:396-567)
enum { PAYLOAD_ID_NONE = 0, PAYLOAD_ID_BLOCK24 = 1, PAYLOAD_ID_BLOCK16 = 2, PAYLOAD_ID_BLOCK32_LEN = 3 };

// the layout of a fec_id / fec_m pair; PAYLOAD_ID_NONE for a pair nfec_payload_id_write and
// nfec_payload_id_read refuse and for fec_id 0 (a message without an ID names no slot)
NFEC_ID_HD inline uint32_t payload_id_kind(uint8_t fec_id, uint8_t fec_m)
{
    switch (fec_id) {
    case 5: return PAYLOAD_ID_BLOCK24;
    case 2: return fec_m == 8 ? PAYLOAD_ID_BLOCK24 : fec_m == 16 ? PAYLOAD_ID_BLOCK16 : PAYLOAD_ID_NONE;
    case 129: return PAYLOAD_ID_BLOCK32_LEN;
    default: return PAYLOAD_ID_NONE;
    }
}

// nfec_payload_id_length of the layout
NFEC_ID_HD inline uint32_t payload_id_length(uint32_t kind)
{
    return kind == PAYLOAD_ID_NONE ? 0u : kind == PAYLOAD_ID_BLOCK32_LEN ? 8u : 4u;
}

NFEC_ID_HD inline uint32_t bswap16(uint32_t v) { return ((v & 0xffu) << 8) | ((v >> 8) & 0xffu); }

// the ID as nfec_payload_id_write lays it out (wire.cpp), byte j in bits [8j, 8j + 8)
NFEC_ID_HD inline uint64_t payload_id(uint32_t kind, uint32_t block_id, uint32_t s, uint32_t nd)
{
    switch (kind) {
    case PAYLOAD_ID_BLOCK24: return __builtin_bswap32((block_id << 8) | (s & 0xffu));
    case PAYLOAD_ID_BLOCK16: return bswap16(block_id & 0xffffu) | (bswap16(s) << 16);
    case PAYLOAD_ID_BLOCK32_LEN:
        return (uint64_t)__builtin_bswap32(block_id) | ((uint64_t)(bswap16(nd) | (bswap16(s) << 16)) << 32);
    default: return 0;
    }
}

// A message can be read (or written) when its ID and its payload lie inside the wire buffer:
// off >= idlen and off + len <= payload_bytes (no sum that could wrap).
NFEC_ID_HD inline bool rx_readable(uint64_t off, uint32_t len, uint32_t idlen, uint64_t payload_bytes)
{
    return off >= idlen && off <= payload_bytes && len <= payload_bytes - off;
}

struct RxId {
    uint32_t block;      // block of the batch: (block_id - first_block_id) mod 2^bits
    uint32_t symbol;     // slot
    uint32_t block_len;  // fec_id 129: the block's numData; 0 where the ID carries none
};

// w0 / w1: the ID's bytes 0-3 / 4-7 as memory holds them, byte j of a word in its bits [8j, 8j + 8)
// (w1 is read only for PAYLOAD_ID_BLOCK32_LEN).  Decodes as nfec_payload_id_read does (big-endian
// fields), then inverts nfec_tx_emit's first_block_id + b inside the block field's width, so a
// window that wraps the field lands where it was sent from.
NFEC_ID_HD inline RxId rx_id_decode(uint32_t kind, uint32_t w0, uint32_t w1, uint32_t first_block_id)
{
    const uint32_t v = __builtin_bswap32(w0);
    RxId id;
    switch (kind) {
    case PAYLOAD_ID_BLOCK24:
        id.block = ((v >> 8) - first_block_id) & 0x00ffffffu;
        id.symbol = v & 0xffu;
        id.block_len = 0;
        break;
    case PAYLOAD_ID_BLOCK16:
        id.block = ((v >> 16) - first_block_id) & 0xffffu;
        id.symbol = v & 0xffffu;
        id.block_len = 0;
        break;
    default: {  // PAYLOAD_ID_BLOCK32_LEN
        const uint32_t x = __builtin_bswap32(w1);
        id.block = v - first_block_id;
        id.block_len = x >> 16;
        id.symbol = x & 0xffffu;
        break;
    }
    }
    return id;
}

}  // namespace nfec
