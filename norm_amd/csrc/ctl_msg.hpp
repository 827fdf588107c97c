// ctl_msg.hpp -- the NORM_NACK and NORM_CMD(REPAIR_ADV) messages on the wire (nfec.h, "NORM_NACK and
// NORM_CMD(REPAIR_ADV) messages on the device"): the two headers, the rule that cuts repair-request
// content into messages of at most segment_size bytes, and what the intake reads out of a control
// datagram.  Shared by the host twins (ctl_msg_host.cpp), the ABI entries and the kernels
// (kernels_ctlmsg.hip), as data_msg.hpp is: what the CPU tests check of the headers, of the cut and
// of the parse is what the kernels run.
//
// Layout (reference include/normMessage.h; all fields big-endian):
//   NormNackMsg       :1906-1989   0 version << 4 | type (0x14), 1 hdr_len, 2-3 sequence, 4-7 source_id,
//                                  8-11 sender_id, 12-13 instance_id, 14-15 reserved, 16-19 / 20-23
//                                  grtt_response sec / usec, extensions up to 4 * hdr_len, the content
//   NormCmdRepairAdvMsg :1200-1249, :1688-1737   0 0x13, 1 hdr_len, 2-3 sequence, 4-7 source_id, 8-9
//                                  instance_id, 10 grtt, 11 backoff << 4 | gsize, 12 flavor (5), 13 flags,
//                                  14-15 reserved, extensions, the content
// The cut is NormSenderNode::FragmentNack (src/common/normNode.cpp:2676-2772) with the two departures
// nfec.h states.
#pragma once

#include <stdint.h>

#include "nack_layout.hpp"

namespace nfec {

constexpr uint32_t kNackBase = 24;         // NormNackMsg's header without extensions
constexpr uint32_t kAdvBase = 16;          // NormCmdRepairAdvMsg's
constexpr uint32_t kCtlExtBytes = 12;      // NormCCFeedbackExtension: three words
constexpr uint32_t kCtlMaxHeader = kNackBase + kCtlExtBytes;
constexpr uint32_t kCtlHeaderWords = kCtlMaxHeader / 4;
constexpr uint32_t kNackVersionType = 0x14;  // version 1, type NACK = 4
constexpr uint32_t kCmdVersionType = 0x13;   // version 1, type CMD = 3
constexpr uint32_t kCmdRepairAdv = 5;        // NormCmdMsg::REPAIR_ADV
constexpr uint32_t kAdvFlagLimit = 1;        // NORM_REPAIR_ADV_FLAG_LIMIT

// ---- the headers a sender of either message writes ----

// A header as words of the wire (byte j of a word in its bits [8j, 8j + 8)); word 0 holds the
// sequence and, for an advertisement, word 3 the flags: ctl_header_word0 / adv_flags_word make them
// per message.
struct CtlHeaderFixed {
    uint32_t w[kCtlHeaderWords] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t hdr_bytes = 0;       // base + ext_bytes
    uint32_t first_sequence = 0;
    uint32_t sequence_step = 0;
};

NFEC_ID_HD inline uint32_t ctl_header_word0(uint32_t version_type, uint32_t hdr_bytes, uint32_t sequence)
{
    return version_type | ((hdr_bytes >> 2) << 8) | (bswap16(sequence & 0xffffu) << 16);
}
NFEC_ID_HD inline uint32_t nack_sequence(const CtlHeaderFixed& f, uint64_t i)
{
    return (f.first_sequence + (uint32_t)i * f.sequence_step) & 0xffffu;
}
NFEC_ID_HD inline uint32_t adv_flags_word(uint32_t limit) { return kCmdRepairAdv | ((limit ? kAdvFlagLimit : 0u) << 8); }

// ext: the extension's words, read where ext_bytes is 12
NFEC_ID_HD inline void nack_header_fixed(CtlHeaderFixed& f, uint32_t source_id, uint32_t sender_id, uint32_t instance_id,
                                         uint32_t sec, uint32_t usec, const uint32_t* ext, uint32_t ext_bytes)
{
    f.hdr_bytes = kNackBase + ext_bytes;
    f.w[0] = ctl_header_word0(kNackVersionType, f.hdr_bytes, 0);
    f.w[1] = __builtin_bswap32(source_id);
    f.w[2] = __builtin_bswap32(sender_id);
    f.w[3] = bswap16(instance_id & 0xffffu);
    f.w[4] = __builtin_bswap32(sec);
    f.w[5] = __builtin_bswap32(usec);
    for (uint32_t j = 0; j < 3; ++j) f.w[6 + j] = ext_bytes ? ext[j] : 0u;
}
NFEC_ID_HD inline void adv_header_fixed(CtlHeaderFixed& f, uint32_t source_id, uint32_t instance_id, uint32_t sequence,
                                        uint32_t grtt, uint32_t backoff, uint32_t gsize, const uint32_t* ext,
                                        uint32_t ext_bytes)
{
    f.hdr_bytes = kAdvBase + ext_bytes;
    f.first_sequence = sequence & 0xffffu;
    f.w[0] = ctl_header_word0(kCmdVersionType, f.hdr_bytes, sequence);
    f.w[1] = __builtin_bswap32(source_id);
    f.w[2] = bswap16(instance_id & 0xffffu) | ((grtt & 0xffu) << 16) | ((((backoff & 15u) << 4) | (gsize & 15u)) << 24);
    f.w[3] = adv_flags_word(0);
    for (uint32_t j = 0; j < 3; ++j) f.w[4 + j] = ext_bytes ? ext[j] : 0u;
    f.w[7] = f.w[8] = 0;
}

// ---- the cut ----
//
// The content is a run of requests, each a 4-byte header and its items.  The cut never looks into
// an item; of a request it needs the header word alone.

constexpr uint32_t kCutEnd = 0xffffffffu;      // no next message
constexpr uint32_t kCutNoState = 0xfffffffeu;  // (tables: a position that is no state)

struct CutParams {
    uint32_t S = 0;  // segment_size: the most content bytes of a message
    uint32_t L = 0;  // item length
};

// NFEC_OK, or what nfec_nack_fragment refuses of (segment_size, header bytes)
NFEC_ID_HD inline bool cut_params_ok(uint32_t S, uint32_t L, uint32_t H)
{
    return (S & 3u) == 0 && S >= 4u + 2u * L && (uint64_t)S + H <= 65535u;
}

struct CutRequest {
    uint32_t len = 0;    // item bytes
    uint32_t unit = 0;   // U: 2 L for RANGES, L for any other form
    uint32_t units = 0;  // len / U
};
// The request whose header word is `word` (byte j in bits [8j, 8j + 8)), with `left` content bytes
// behind the header.  false where the walk stops: a length past the content, item bytes that are no
// multiple of L, an odd item count in RANGES.
NFEC_ID_HD inline bool cut_request(uint32_t word, uint64_t left, uint32_t L, CutRequest& q)
{
    q.len = bswap16(word >> 16);
    q.unit = (word & 0xffu) == REPAIR_RANGES ? 2u * L : L;
    q.units = q.len / q.unit;
    return q.len <= left && q.len % L == 0 && q.len % q.unit == 0;
}
// a request's header with the length field replaced (the copy arm B writes)
NFEC_ID_HD inline uint32_t cut_header_word(uint32_t word, uint32_t len) { return (word & 0xffffu) | (bswap16(len) << 16); }

// After a message closes, the walk's state is (request r, unit u): the next message begins with a
// copy of r's header and r's units from u on; (r, 0) is also the fresh state, since a split that
// starts at unit 0 produces the bytes of the whole copy.  A state is named by the content offset of
// its first unit, pos = off_r + 4 + u U_r (off_r + 4 for a request without items): no two states
// share one.  The requests are indexed by their offsets in dwords, req[0 .. R), ascending, and they
// tile the content's first `end` bytes.
struct CutIndex {
    const uint32_t* req = nullptr;  // [R]: a request's offset / 4
    uint32_t R = 0;
    uint64_t end = 0;               // where the walk stopped: the offset behind request R - 1
    NFEC_ID_HD uint64_t off(uint32_t r) const { return r < R ? (uint64_t)req[r] * 4u : end; }
};

// the request that holds the state at pos (pos >= 4): the last r with off(r) + 4 <= pos
NFEC_ID_HD inline uint32_t cut_owner(const CutIndex& x, uint64_t pos)
{
    uint32_t lo = 0, hi = x.R ? x.R - 1u : 0u;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1u) / 2u;
        if (x.off(mid) + 4u <= pos) lo = mid;
        else hi = mid - 1u;
    }
    return lo;
}

// One message: the content bytes [src, src + length) with the first dword replaced by `head` and,
// where tail_at is not 0, the dword at src + tail_at replaced by `tail`.
struct CutMessage {
    uint64_t src = 0;
    uint32_t length = 0;
    uint32_t head = 0;
    uint32_t tail_at = 0, tail = 0;
    uint64_t next = 0;      // the next state's pos; ~0: the content is used up
    uint64_t used = 0;      // the content offset up to which this and the earlier messages took it
    uint32_t split = 0;     // arm B was entered in this message
};
constexpr uint64_t kCutDone = ~(uint64_t)0;

// The message that begins in the state at pos, which request r holds.  load(off): the content's
// dword at byte offset off (off + 4 <= the content's length; every offset this function passes is a
// request's, out of the index).  From (r, u): min(n_r - u, (S - 4) / U_r) units of r; when that
// finishes r, whole requests while they fit (a search over the request offsets, which are the prefix
// sums of the request lengths); then t = (S - P - 4) / U_j >= 1 units of the first request j that
// does not fit, next state (j, t), or, when not even one unit fits, next state (j, 0).
template <class Load>
NFEC_ID_HD inline CutMessage cut_message(const CutParams& c, const CutIndex& x, uint32_t r, uint64_t pos, Load load)
{
    CutMessage m;
    const uint64_t off_r = x.off(r);
    const uint32_t hw = load(off_r);
    CutRequest q;
    cut_request(hw, ~(uint64_t)0, c.L, q);
    const uint32_t u = (uint32_t)((pos - off_r - 4u) / q.unit);
    const uint32_t fit = (c.S - 4u) / q.unit;
    const uint32_t rest = q.units > u ? q.units - u : 0u;
    const uint32_t a = rest < fit ? rest : fit;
    m.src = pos - 4u;
    m.head = cut_header_word(hw, a * q.unit);
    uint32_t P = 4u + a * q.unit;
    if (a < rest) {  // r goes on in the next message
        m.length = P;
        m.next = m.used = pos + (uint64_t)a * q.unit;
        m.split = u == 0;
        return m;
    }
    // whole requests: the last j in [r + 1, R] with off(j) - off(r + 1) <= S - P
    const uint64_t base = x.off(r + 1u);
    const uint32_t budget = c.S - P;
    uint32_t lo = r + 1u, hi = x.R;
    if (hi - lo > c.S / 4u) hi = lo + c.S / 4u;  // (a request is 4 bytes at least)
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1u) / 2u;
        if (x.off(mid) - base <= budget) lo = mid;
        else hi = mid - 1u;
    }
    const uint32_t j = lo;
    P += (uint32_t)(x.off(j) - base);
    m.length = P;
    m.used = x.off(j);
    if (j >= x.R) {
        m.next = kCutDone;
        return m;
    }
    const uint64_t off_j = x.off(j);
    const uint32_t hj = load(off_j);
    CutRequest qj;
    cut_request(hj, ~(uint64_t)0, c.L, qj);
    if (qj.units >= 1 && P + 4u + qj.unit <= c.S) {  // arm B
        uint32_t t = (c.S - P - 4u) / qj.unit;
        if (t > qj.units) t = qj.units;  // (only with an index that does not belong to the content)
        m.tail_at = P, m.tail = cut_header_word(hj, t * qj.unit);
        m.length = P + 4u + t * qj.unit;
        m.next = m.used = off_j + 4u + (uint64_t)t * qj.unit;
        m.split = 1;
    } else {  // arm C
        m.next = off_j + 4u;
    }
    return m;
}

// The first message of the cut of content[0, bytes) by a walk over its request headers, for a caller
// that wants no more than that message (an advertisement): cut_message's bytes for the state (0, 0)
// without an index.  length 0: the content holds no request.
template <class Load>
NFEC_ID_HD inline CutMessage cut_first_message(const CutParams& c, uint64_t bytes, Load load)
{
    CutMessage m;
    uint32_t P = 0;
    uint64_t off = 0;
    m.next = kCutDone;
    for (;;) {
        CutRequest q;
        if (bytes - off < 4u) break;
        const uint32_t w = load(off);
        if (!cut_request(w, bytes - off - 4u, c.L, q)) break;
        if (off == 0) m.head = w;
        if (P + 4u + q.len <= c.S) {  // arm A
            P += 4u + q.len, off += 4u + q.len;
            continue;
        }
        if (q.units >= 1 && P + 4u + q.unit <= c.S) {  // arm B
            const uint32_t t = (c.S - P - 4u) / q.unit;
            const uint32_t word = cut_header_word(w, t * q.unit);
            if (P == 0) m.head = word;
            else m.tail_at = P, m.tail = word;
            P += 4u + t * q.unit, off += 4u + (uint64_t)t * q.unit;
            m.split = 1;
            m.next = off;
        } else {  // arm C
            m.next = off + 4u;
        }
        break;
    }
    m.length = P, m.used = off;
    return m;
}

// ---- what the intake reads of a control datagram ----
//
// The first kCtlParseBytes bytes at the most: the NACK's base header.  They are loaded as the
// aligned 16-byte chunks that hold bytes [off, off + min(length, kCtlParseBytes)): at most three,
// each of which holds a byte of the datagram.
constexpr uint32_t kCtlParseBytes = 24;
constexpr uint32_t kCtlParseWords = kCtlParseBytes / 4;
constexpr uint32_t kCtlMinDatagram = 8;  // NormMsg's own header: below it no byte is loaded

NFEC_ID_HD inline uint64_t ctl_chunk_offset(uint64_t at) { return at & ~(uint64_t)15u; }
NFEC_ID_HD inline uint32_t ctl_chunk_count(uint64_t at, uint32_t length)
{
    const uint32_t n = length < kCtlParseBytes ? length : kCtlParseBytes;
    return length >= kCtlMinDatagram ? ((uint32_t)(at & 15u) + n + 15u) >> 4 : 0u;
}
NFEC_ID_HD inline bool ctl_readable(uint64_t off, uint32_t length, uint64_t payload_bytes)
{
    return length >= kCtlMinDatagram && off <= payload_bytes && length <= payload_bytes - off;
}

// one class per datagram (NFEC_CTL_* of nfec.h), the first whose condition holds
enum {
    CTL_UNREADABLE = 0,
    CTL_OTHER_TYPE = 1,
    CTL_MALFORMED = 2,
    CTL_OTHER_FLAVOR = 3,
    CTL_OWN = 4,
    CTL_OTHER_SENDER = 5,
    CTL_OTHER_INSTANCE = 6,
    CTL_NACK = 7,
    CTL_REPAIR_ADV = 8,
    CTL_CLASSES = 9,
    CTL_EXTENDED = 0x80
};
enum { CTL_ANY_INSTANCE = 1u, CTL_TAKE_NACK = 2u, CTL_TAKE_ADV = 4u };

struct CtlFilter {
    uint32_t sender_id = 0;
    uint32_t instance_id = 0;
    uint32_t local_id = 0;
    uint32_t flags = 0;
};

struct CtlParse {
    uint32_t cls;         // CTL_* (without CTL_EXTENDED)
    uint32_t extended;    // classes NACK and REPAIR_ADV: 4 * hdr_len exceeds the base header
    uint32_t hdr_bytes;   // 4 * hdr_len where the datagram gets a content entry, else 0
    uint32_t source_id;   // bytes 4-7
    uint32_t sec, usec;   // a NACK's grtt_response, else 0
};

// h[j]: bytes [4j, 4j + 4) of a readable datagram as memory holds them.  A word is read only where
// the datagram has all the bytes the rule needs of it, so words past its length may hold anything.
// CTL_MALFORMED is NormMsg::InitFromBuffer's rule (reference src/common/normMessage.cpp:17-92): 24
// bytes of base header for a NACK; 16 for a CMD, the base of REPAIR_ADV and the least of any flavor.
NFEC_ID_HD inline CtlParse ctl_parse(const uint32_t (&h)[kCtlParseWords], uint32_t length, const CtlFilter& f)
{
    CtlParse r;
    r.cls = CTL_OTHER_TYPE, r.extended = 0, r.hdr_bytes = 0, r.sec = r.usec = 0;
    r.source_id = __builtin_bswap32(h[1]);
    const uint32_t type = h[0] & 0x0fu;
    if (type != 4u && type != 3u) return r;
    const bool nack = type == 4u;
    const uint32_t base = nack ? kNackBase : kAdvBase;
    const uint32_t hdr = ((h[0] >> 8) & 0xffu) * 4u;
    if (length < base || hdr < base || hdr > length) {
        r.cls = CTL_MALFORMED;
        return r;
    }
    if (!nack && (h[3] & 0xffu) != kCmdRepairAdv) {
        r.cls = CTL_OTHER_FLAVOR;
        return r;
    }
    if (f.local_id != 0 && r.source_id == f.local_id) {
        r.cls = CTL_OWN;
        return r;
    }
    if ((nack ? __builtin_bswap32(h[2]) : r.source_id) != f.sender_id) {
        r.cls = CTL_OTHER_SENDER;
        return r;
    }
    const uint32_t instance = nack ? bswap16(h[3] & 0xffffu) : bswap16(h[2] & 0xffffu);
    if (!(f.flags & CTL_ANY_INSTANCE) && instance != f.instance_id) {
        r.cls = CTL_OTHER_INSTANCE;
        return r;
    }
    r.cls = nack ? CTL_NACK : CTL_REPAIR_ADV;
    r.extended = hdr > base;
    if (f.flags & (nack ? CTL_TAKE_NACK : CTL_TAKE_ADV)) r.hdr_bytes = hdr;
    if (nack) r.sec = __builtin_bswap32(h[4]), r.usec = __builtin_bswap32(h[5]);
    return r;
}

}  // namespace nfec
