// stream_layout.hpp -- the segment rule of a NORM stream object (nfec.h, "stream objects on the
// device"), shared by the host entry (stream.cpp), the kernels (kernels_stream.hip) and a host
// driver (tests/native/stream_copy_asan.cpp): what the CPU tests check of the framing is what the
// kernels compute.
//
// The rule restates NormStreamObject::Write's loop (reference src/common/normObject.cpp:4166-4210)
// in closed form.  The call's byte run is the carry (the open trailing segment of the calls before)
// followed by the writes; an *element* is one contiguous piece of it: element 0 the carry, element
// i + 1 write i.  Per element the rule needs six scans -- four over the elements before it, two
// over the elements after it -- and everything else is arithmetic on one element:
//
//   B   its first byte's position (sum of the lengths before it)
//   G   the last cut at or before B: the end of the last FLUSH write before it, else 0
//   LN  1 + the last write of nonzero length before it, LE  1 + the last EOM write before it
//   NF  the first cut at or after its end: the end of the first FLUSH write from it on, else none
//   NM  the first message-start position in the elements after it, else none
//
// The host entry runs them as loops, the kernels as tiled scans.
#pragma once

#include <stdint.h>

#include "nfec.h"
#include "object_layout.hpp"  // NFEC_HD

namespace nfec {

constexpr uint64_t kStreamNone = ~0ull;  // "no such position"
constexpr uint32_t kStreamHeader = 8;    // NormDataMsg::GetStreamPayloadHeaderLength (normMessage.h:1145-1196)

// Write's test `msg_start && (0 != len)` (:4175) for a write of `len` bytes, from the two "last
// write" scans over the writes before it: the flag is raised behind every EOM write (:4214-4217,
// zero-length writes too) and taken by the next nonzero write, so it stands when an EOM write lies
// at or behind the last nonzero write -- or, before the call's first nonzero write, when the
// carried state had it raised or any EOM write came since.
NFEC_HD inline bool stream_flag_raised(uint64_t LN, uint64_t LE, bool pending0)
{
    return LN == 0 ? (pending0 || LE != 0) : LE >= LN;
}
NFEC_HD inline bool stream_is_message_start(uint32_t len, uint64_t LN, uint64_t LE, bool pending0)
{
    return len != 0 && stream_flag_raised(LN, LE, pending0);
}

// the first segment start at or after B in the group that begins at the cut G <= B
NFEC_HD inline uint64_t stream_first_start(uint64_t B, uint64_t G, uint32_t S)
{
    const uint64_t d = B - G;
    return G + (d + S - 1u) / S * S;
}

// Where the new carry begins: behind the full segments of the open group [G_last, end).
NFEC_HD inline uint64_t stream_consumed(uint64_t G_last, uint64_t end, uint32_t S)
{
    return G_last + (end - G_last) / S * S;
}

// The closed segments that start inside an element [B, E): starts x0, x0 + S, ... below E when a
// cut follows (NF), else below the new carry.
NFEC_HD inline uint64_t stream_closed_count(uint64_t x0, uint64_t E, uint64_t NF, uint64_t consumed, uint32_t S)
{
    const uint64_t lim = NF != kStreamNone || E < consumed ? E : consumed;
    return lim > x0 ? (lim - x0 + S - 1u) / S : 0u;
}

// Segment t of an element: [x, e) with its header's msg_start.  m_first: the first message-start
// position at or after x0 (the element's own when it has one there, else NM); later segments of
// the element start behind its own message start, so theirs is NM.
NFEC_HD inline void stream_segment_at(uint64_t x0, uint64_t t, uint32_t S, uint64_t NF, uint64_t m_first, uint64_t NM,
                                      uint64_t* start, uint16_t* len, uint16_t* msg_start)
{
    const uint64_t x = x0 + t * S;
    const uint64_t e = NF != kStreamNone && NF < x + S ? NF : x + S;
    const uint64_t p = t == 0 ? m_first : NM;
    *start = x;
    *len = (uint16_t)(e - x);
    *msg_start = p != kStreamNone && p < e ? (uint16_t)(p - x + 1u) : (uint16_t)0;
}

// The carry's message start behind `consumed`, from the first message-start position at or after it.
NFEC_HD inline uint32_t stream_carry_msg_start(uint64_t p, uint64_t consumed)
{
    return p == kStreamNone ? 0u : (uint32_t)(p - consumed + 1u);
}

// ---- the payload header (normMessage.h:1145-1196): length, msg_start, offset, big-endian ----
// As the two dwords of the slot's first 8 bytes on a little-endian machine.

NFEC_HD inline uint32_t stream_swap16(uint32_t v) { return ((v & 0xffu) << 8) | ((v >> 8) & 0xffu); }
NFEC_HD inline uint32_t stream_swap32(uint32_t v)
{
    return (v << 24) | ((v & 0xff00u) << 8) | ((v >> 8) & 0xff00u) | (v >> 24);
}
NFEC_HD inline void stream_header_encode(uint32_t len, uint32_t msg_start, uint32_t offset, uint32_t* w0, uint32_t* w1)
{
    *w0 = stream_swap16(len) | (stream_swap16(msg_start) << 16);
    *w1 = stream_swap32(offset);
}
NFEC_HD inline void stream_header_decode(uint32_t w0, uint32_t w1, uint32_t* len, uint32_t* msg_start, uint32_t* offset)
{
    *len = stream_swap16(w0 & 0xffffu);
    *msg_start = stream_swap16(w0 >> 16);
    *offset = stream_swap32(w1);
}

// ---- what the copy entries accept ----

// pack: a table entry may be copied (its block is checked apart)
NFEC_HD inline bool stream_entry_ok(uint64_t seg_start, uint32_t len, uint32_t S, uint64_t stream_bytes)
{
    return len != 0 && len <= S && len <= stream_bytes && seg_start <= stream_bytes - len;
}

// unpack: what a header asks for.  The header is network data: only DELIVER copies, and then
// len <= S and [d, d + len) lies inside the window.
enum StreamVerdict : uint32_t { STREAM_DELIVER = 0, STREAM_CONTROL = 2, STREAM_INVALID = 3 };  // (the stats index)
NFEC_HD inline uint32_t stream_header_verdict(uint32_t len, uint32_t offset, uint32_t base_offset, uint32_t S,
                                              uint64_t window_bytes, uint32_t* d)
{
    *d = offset - base_offset;  // mod 2^32
    if (len == 0) return STREAM_CONTROL;
    if (len > S || (uint64_t)*d + len > window_bytes) return STREAM_INVALID;
    return STREAM_DELIVER;
}

}  // namespace nfec
