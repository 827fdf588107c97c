// data_msg.hpp -- the NORM_DATA message on the wire (nfec.h, "NORM_DATA messages on the device"): the
// header nfec_tx_emit_data writes in front of a payload, what nfec_rx_ingest_data reads out of a
// datagram, and which aligned chunks of the wire buffer it loads to do so.  Shared by the host twins
// (data_msg_host.cpp), the ABI entries and the kernels (kernels_datamsg.hip), as rx_parse.hpp is: what
// the CPU tests check of the header and of the parse is what the kernels run.
//
// Layout (reference include/normMessage.h; all fields big-endian):
//   NormMsg        :688-696    byte 0 version << 4 | type, byte 1 hdr_len in 32-bit words, 2-3 sequence,
//                              4-7 source_id
//   NormObjectMsg  :769-779    8-9 instance_id, 10 grtt, 11 backoff << 4 | gsize, 12 flags, 13 fec_id,
//                              14-15 object transport id
//   NormDataMsg    :1183-1186  16 ... the FEC payload ID, then the header extensions up to 4 * hdr_len
//                              (AttachExtension, :612-616), then the payload (:636-637, :1127-1130)
#pragma once

#include <stdint.h>

#include "rx_parse.hpp"

namespace nfec {

// one class per datagram (NFEC_DGRAM_* of nfec.h), the first whose condition holds
enum {
    DGRAM_UNREADABLE = 0,
    DGRAM_OTHER_TYPE = 1,
    DGRAM_MALFORMED = 2,
    DGRAM_OTHER_SENDER = 3,
    DGRAM_OTHER_CODE = 4,
    DGRAM_OTHER_OBJECT = 5,
    DGRAM_REJECTED = 6,
    DGRAM_DUPLICATE = 7,
    DGRAM_PLACED = 8,
    DGRAM_CLASSES = 9,
    DGRAM_PARSED = 9  // the host twin's: past the filter, nfec_rx_place's rule decides the rest
};

constexpr uint32_t kDataBase = 16;        // NormObjectMsg::OBJ_MSG_OFFSET: where the payload ID starts
constexpr uint32_t kDataVersionType = 0x12;  // version 1 (:26), type DATA = 2 (:578)
constexpr uint32_t kDataMaxHeader = 40;   // 16 + the 8-byte ID + a 16-byte FTI
constexpr uint32_t kDataHeaderWords = kDataMaxHeader / 4;
constexpr uint32_t kExtFti = 64;          // NormHeaderExtension::FTI (:330)

// NormPayloadId::GetLength of the fec_id byte a message carries (0: unknown)
NFEC_ID_HD inline uint32_t data_id_length(uint32_t fec_id_byte)
{
    return fec_id_byte == 2u || fec_id_byte == 5u ? 4u : fec_id_byte == 129u ? 8u : 0u;
}

// the FTI extension's length for a fec_id (nfec_fti_write's)
NFEC_ID_HD inline uint32_t data_fti_length(uint32_t fec_id) { return fec_id == 5u ? 12u : 16u; }

// ---- the header a sender writes ----

// What the messages of one call share, as words of the wire (byte j of a word in its bits [8j, 8j +
// 8)): bytes 4-15 and the extension.  nfec_api.cpp and the host twin make it from an nfec_data_header.
struct DataHeaderFixed {
    uint32_t w1 = 0, w2 = 0, w3 = 0;  // bytes 4-7, 8-11, 12-15
    uint32_t ext[4] = {0, 0, 0, 0};
    uint32_t ext_bytes = 0;           // 0, 12 or 16
    uint32_t first_sequence = 0;
    uint32_t id_kind = 0;             // PAYLOAD_ID_* (never NONE)
    uint32_t hdr_bytes = 0;           // 16 + idlen + ext_bytes
};

NFEC_ID_HD inline void data_header_fixed(DataHeaderFixed& f, uint32_t source_id, uint32_t instance_id, uint32_t grtt,
                                         uint32_t backoff, uint32_t gsize, uint32_t flags, uint32_t fec_id,
                                         uint32_t object_id)
{
    f.w1 = __builtin_bswap32(source_id);
    f.w2 = bswap16(instance_id & 0xffffu) | ((grtt & 0xffu) << 16) | ((((backoff & 15u) << 4) | (gsize & 15u)) << 24);
    f.w3 = (flags & 0xffu) | ((fec_id & 0xffu) << 8) | (bswap16(object_id & 0xffffu) << 16);
}

// The header of message i of a call: hdr_bytes / 4 words, the rest of w[] zero.  id: payload_id()'s
// value for the message's block, slot and block length.
NFEC_ID_HD inline void data_header_words(const DataHeaderFixed& f, uint32_t i, uint64_t id, uint32_t (&w)[kDataHeaderWords])
{
    const uint32_t seq = (f.first_sequence + i) & 0xffffu;
    w[0] = kDataVersionType | ((f.hdr_bytes >> 2) << 8) | (bswap16(seq) << 16);
    w[1] = f.w1, w[2] = f.w2, w[3] = f.w3;
    w[4] = (uint32_t)id;
    const bool id8 = f.id_kind == PAYLOAD_ID_BLOCK32_LEN;
    const uint32_t e0 = f.ext_bytes ? f.ext[0] : 0u, e1 = f.ext_bytes ? f.ext[1] : 0u, e2 = f.ext_bytes ? f.ext[2] : 0u,
                   e3 = f.ext_bytes > 12u ? f.ext[3] : 0u;
    w[5] = id8 ? (uint32_t)(id >> 32) : e0;
    w[6] = id8 ? e0 : e1;
    w[7] = id8 ? e1 : e2;
    w[8] = id8 ? e2 : e3;
    w[9] = id8 ? e3 : 0u;
}

// ---- what a receiver loads of a datagram before it knows more than (off, length) ----
//
// The parse reads the first kParseBytes bytes of a datagram at the most: the base header, the
// longest payload ID and the first word of the first extension.  They are loaded as the aligned
// 16-byte chunks that hold bytes [off, off + min(length, kParseBytes)): at most three, each of
// which holds a byte of the datagram, so no load leaves a page the datagram touches.  This is the
// only place the chunk addresses are computed: with `at` the datagram's address (the wire buffer may
// lie at any byte alignment) the kernel loads chunk c at data_chunk_offset(at) + 16 c for c <
// data_chunk_count(at, length), and nfec_rx_data_chunks_host enumerates the same.
constexpr uint32_t kParseBytes = 28;
constexpr uint32_t kParseWords = kParseBytes / 4;
constexpr uint32_t kMinDatagram = 8;  // NormMsg's own header: below it no byte is loaded

NFEC_ID_HD inline uint64_t data_chunk_offset(uint64_t at) { return at & ~(uint64_t)15u; }
NFEC_ID_HD inline uint32_t data_chunk_count(uint64_t at, uint32_t length)
{
    const uint32_t n = length < kParseBytes ? length : kParseBytes;
    return length >= kMinDatagram ? ((uint32_t)(at & 15u) + n + 15u) >> 4 : 0u;
}

// off + length <= payload_bytes (no sum that could wrap) and length >= 8
NFEC_ID_HD inline bool data_readable(uint64_t off, uint32_t length, uint64_t payload_bytes)
{
    return length >= kMinDatagram && off <= payload_bytes && length <= payload_bytes - off;
}

// ---- the parse ----

struct DataFilter {
    uint32_t source_id = 0;
    uint32_t instance_id = 0;
    uint32_t fec_id = 0;
    uint32_t object_id = 0;
    uint32_t id_kind = 0;  // of the filter's fec_id / fec_m (never NONE)
};

struct DataParse {
    uint32_t cls;        // DGRAM_OTHER_TYPE ... DGRAM_OTHER_OBJECT, or DGRAM_PARSED
    uint32_t sequence;   // bytes 2-3
    uint32_t hdr_bytes;  // 4 * hdr_len: where the payload starts (DGRAM_PARSED only)
    RxId id;             // DGRAM_PARSED only; all ones elsewhere
    bool fti;            // DGRAM_PARSED, and the first extension has type 64 and fits inside the header
};

// h[j]: bytes [4j, 4j + 4) of a readable datagram as memory holds them, byte t in bits [8t, 8t + 8).
// A word is read only where the datagram has all the bytes the rule needs of it, so words past the
// datagram's length may hold anything.  The order of the tests is the order of the classes;
// DGRAM_MALFORMED is NormMsg::InitFromBuffer's rule for a DATA message (reference
// src/common/normMessage.cpp:17-92): an unknown fec_id byte, a header shorter than 16 + idlen or
// longer than the datagram.
NFEC_ID_HD inline DataParse data_parse(const uint32_t (&h)[kParseWords], uint32_t length, const DataFilter& f,
                                       uint32_t first_block_id)
{
    DataParse r;
    r.cls = DGRAM_PARSED;
    r.sequence = bswap16(h[0] >> 16);
    r.hdr_bytes = 0;
    r.id = RxId{0xffffffffu, 0xffffu, 0xffffu};
    r.fti = false;
    if ((h[0] & 0x0fu) != 2u) {
        r.cls = DGRAM_OTHER_TYPE;
        return r;
    }
    const uint32_t hdr = ((h[0] >> 8) & 0xffu) * 4u;
    const uint32_t fec_id = length >= kDataBase ? (h[3] >> 8) & 0xffu : 0u;
    const uint32_t idlen = data_id_length(fec_id);
    if (length < kDataBase || idlen == 0 || length < kDataBase + idlen || hdr < kDataBase + idlen || hdr > length) {
        r.cls = DGRAM_MALFORMED;
        return r;
    }
    if (__builtin_bswap32(h[1]) != f.source_id || bswap16(h[2] & 0xffffu) != f.instance_id) {
        r.cls = DGRAM_OTHER_SENDER;
        return r;
    }
    if (fec_id != f.fec_id) {
        r.cls = DGRAM_OTHER_CODE;
        return r;
    }
    if (bswap16(h[3] >> 16) != f.object_id) {
        r.cls = DGRAM_OTHER_OBJECT;
        return r;
    }
    r.hdr_bytes = hdr;
    r.id = rx_id_decode(f.id_kind, h[4], h[5], first_block_id);
    // The first extension, when the header has room for one word of it (which then lies inside the
    // datagram: hdr <= length).  Only the first is examined; a length byte of 0 is not followed.
    if (hdr >= kDataBase + idlen + 4u) {
        const uint32_t e = idlen == 8u ? h[6] : h[5];
        const uint32_t words = (e >> 8) & 0xffu;
        r.fti = (e & 0xffu) == kExtFti && words != 0 && kDataBase + idlen + 4u * words <= hdr;
    }
    return r;
}

}  // namespace nfec
