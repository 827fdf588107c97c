// nack_layout.hpp -- the repair-request content of a NORM_NACK from reception masks (nfec.h,
// "repair requests on the device"): which blocks ask, what a block asks for, how its runs become
// ITEMS / RANGES units, where a request opens, and the bytes of a request header and of an item.
// Shared by the host entries (nack_host.cpp) and the kernels (kernels_nack.hip): what the CPU tests
// check of the rule is what the kernels run.
//
// Reference: NormObject::AppendRepairRequest (src/common/normObject.cpp:1179-1381, flush form,
// NACK_NORMAL), NormBlock::AppendRepairRequest (src/common/normSegment.cpp:524-630),
// NormRepairRequest::AppendRepairItem / AppendRepairRange / Pack (src/common/normMessage.cpp:163-276)
// and its Form / Flag values (include/normMessage.h:1551-1579).
#pragma once

#include "rx_parse.hpp"

namespace nfec {

// a block's class (block_start's second column)
enum { NACK_SILENT = 0, NACK_NEEDING = 1, NACK_ABSENT = 2 };
// NormRepairRequest::Form and ::Flag (normMessage.h:1551-1563)
enum { REPAIR_ITEMS = 1, REPAIR_RANGES = 2, REPAIR_ERASURES = 3 };
enum { REPAIR_SEGMENT = 0x01, REPAIR_BLOCK = 0x02, REPAIR_INFO = 0x04 };

// RepairItemLength (normMessage.h:1574): fec_id, reserved, object id, then the FEC payload ID
NFEC_ID_HD inline uint32_t nack_item_length(uint32_t id_kind) { return 4u + payload_id_length(id_kind); }
// the most units a request may hold: a unit is at most two items and the length field has 16 bits
NFEC_ID_HD inline uint32_t nack_max_units_limit(uint32_t id_kind) { return 65535u / (2u * nack_item_length(id_kind)); }

// The class of a block with nd source slots, e pending source slots, p received parity slots and
// `any` != 0 when some bit of [0, nd + m) is set.  A block without a received segment has no
// NormBlock in the reference (normObject.cpp:1207); one with e <= p is complete or decodable and is
// no longer pending there.
NFEC_ID_HD inline uint32_t nack_class(uint32_t nd, uint32_t k, uint32_t e, uint32_t p, uint32_t any)
{
    if (nd < 1 || nd > k) return NACK_SILENT;
    if (!any) return NACK_ABSENT;
    return e > p ? NACK_NEEDING : NACK_SILENT;
}

// The request set of a needing block is its pending slots inside [lo, hi) (normSegment.cpp:536-554):
// with e > m everything behind the m-th pending slot (mth, 0-based slot of the m-th pending one),
// otherwise the pending parity slots of [nd, nd + e).
struct NackCut {
    uint32_t lo, hi;
};
NFEC_ID_HD inline NackCut nack_cut(uint32_t nd, uint32_t m, uint32_t e, uint32_t mth)
{
    NackCut c;
    if (e > m) {
        c.lo = mth + 1u, c.hi = nd + m;
    } else {
        c.lo = nd, c.hi = nd + e;
    }
    return c;
}

// the bits of mask word w whose slots lie in [lo, hi)
NFEC_ID_HD inline uint32_t nack_range_bits(uint32_t w, uint32_t lo, uint32_t hi)
{
    const uint64_t first = (uint64_t)w << 5;
    if (hi <= first || lo >= first + 32u) return 0u;
    uint32_t bits = 0xffffffffu;
    if (lo > first) bits &= 0xffffffffu << (lo - first);
    if (hi < first + 32u) bits &= (1u << (hi - first)) - 1u;
    return bits;
}
// word w of the request set, from word w of the reception mask
NFEC_ID_HD inline uint32_t nack_request_word(uint32_t received, uint32_t w, NackCut c)
{
    return ~received & nack_range_bits(w, c.lo, c.hi);
}

// A maximal run of `len` consecutive slots (or absent blocks) is one unit (normSegment.cpp:572-584,
// normObject.cpp:1217-1228): its form and how many items it holds.
NFEC_ID_HD inline uint32_t nack_unit_form(uint64_t len) { return len >= 3 ? REPAIR_RANGES : REPAIR_ITEMS; }
NFEC_ID_HD inline uint32_t nack_unit_items(uint64_t len) { return len >= 2 ? 2u : 1u; }

// The scans' operator.  Every running state of the walk is a segmented sum: v adds up until an
// element with f set starts over from its own v.  The chain over blocks runs three of them:
//   - the absent-run length so far (an absent block is {1, 0}, any other block {0, 1}),
//   - the last form in the chain (a unit is {form, 1}, a needing block {0, 1}, anything else {0, 0}),
//   - the units since the last change of form (a unit is {1, form != last form}); a unit opens a
//     request when (that count - 1) is a multiple of max_units, and the units in the open request
//     are ((count - 1) mod max_units) + 1,
// and a fourth gives the items in the open request (a unit is {items, opens}).  The walk inside a
// block runs the last three over its runs.  The operator is associative with identity {0, 0}.
struct SegVal {
    uint64_t v;
    uint32_t f;
};
NFEC_ID_HD inline SegVal seg_combine(SegVal a, SegVal b)
{
    SegVal r;
    r.v = b.f ? b.v : a.v + b.v;
    r.f = a.f | b.f;
    return r;
}
// does the unit that is the `since`-th of its same-form stretch (1-based) open a request?
// ((since - 1) mod max_units == 0, without the division while the stretch is shorter than a request)
NFEC_ID_HD inline bool nack_opens(uint32_t since, uint32_t max_units)
{
    return since - 1u < max_units ? since == 1u : (since - 1u) % max_units == 0;
}

// What a call needs of its arguments to lay out bytes.
struct NackFormat {
    uint32_t id_kind = 0;         // the payload ID's layout (PAYLOAD_ID_*)
    uint32_t item_len = 0;        // nack_item_length(id_kind)
    uint32_t fec_id = 0;
    uint32_t object_id = 0;       // 16 bits
    uint32_t first_block_id = 0;
    uint32_t info = 0;            // REPAIR_INFO or 0: on every request
    uint32_t max_units = 0;
};

// The dwords of the content as memory holds them (byte j of a dword in its bits [8j, 8j + 8)).
// Request header: form (u8), flags (u8), length of the items (u16, big-endian) (Pack, normMessage.cpp:263).
NFEC_ID_HD inline uint32_t nack_header_word(uint32_t form, uint32_t flags, uint32_t length)
{
    return (form & 0xffu) | ((flags & 0xffu) << 8) | (bswap16(length) << 16);
}
// An item's first dword: fec_id (u8), reserved 0 (u8), object id (u16, big-endian) (normMessage.cpp:182-184);
// behind it payload_id()'s one or two dwords.
NFEC_ID_HD inline uint32_t nack_item_word(const NackFormat& f) { return (f.fec_id & 0xffu) | (bswap16(f.object_id) << 16); }

// ---- the serial walk (host entries; the kernels reach the same bytes by scans) ----

// Where the bytes go: nothing at or past capacity is written, `off` and `requests` count on.
struct NackWriter {
    uint8_t* content = nullptr;
    uint64_t capacity = 0;
    uint64_t off = 0, requests = 0;
    void put32(uint64_t at, uint32_t word) const
    {
        for (uint32_t j = 0; j < 4; ++j)
            if (at + j < capacity) content[at + j] = (uint8_t)(word >> (8 * j));
    }
    void put_item(uint64_t at, const NackFormat& f, uint32_t b, uint32_t s, uint32_t nd) const
    {
        const uint64_t id = payload_id(f.id_kind, f.first_block_id + b, s, nd);
        put32(at, nack_item_word(f));
        put32(at + 4, (uint32_t)id);
        if (f.item_len == 12) put32(at + 8, (uint32_t)(id >> 32));
    }
};

// A chain of units: the last form, the units since it changed, the items in the open request.
struct NackChain {
    uint32_t form = 0;
    uint32_t since = 0;
    uint32_t open_items = 0;
};
// the open request's header, which lies in front of its items (they are the last bytes written)
inline void nack_close(NackWriter& o, NackChain& c, const NackFormat& f, uint32_t flags)
{
    if (c.form) o.put32(o.off - (uint64_t)f.item_len * c.open_items - 4u, nack_header_word(c.form, flags | f.info, f.item_len * c.open_items));
    c = NackChain();
}
// one unit: a run of `len` from (b0, s0, nd0) to (b1, s1, nd1)
inline void nack_unit(NackWriter& o, NackChain& c, const NackFormat& f, uint32_t flags, uint64_t len, uint32_t b0,
                      uint32_t s0, uint32_t nd0, uint32_t b1, uint32_t s1, uint32_t nd1)
{
    const uint32_t form = nack_unit_form(len), items = nack_unit_items(len);
    const uint32_t since = form != c.form ? 1u : c.since + 1u;
    if (nack_opens(since, f.max_units)) {
        nack_close(o, c, f, flags);
        o.off += 4, ++o.requests;
    }
    o.put_item(o.off, f, b0, s0, nd0);
    if (items == 2) o.put_item(o.off + f.item_len, f, b1, s1, nd1);
    o.off += (uint64_t)f.item_len * items;
    c.form = form, c.since = since, c.open_items += items;
}

// A block's class and, for a needing block, its cut.  mask: the block's words of the reception mask.
inline uint32_t nack_block_class_host(const uint32_t* mask, uint32_t nd, uint32_t k, uint32_t m, NackCut* cut)
{
    if (nd < 1 || nd > k) return NACK_SILENT;
    uint32_t e = 0, p = 0, any = 0, seen = 0, mth = 0;
    for (uint32_t s = 0; s < nd + m; ++s) {
        const bool got = (mask[s >> 5] >> (s & 31u)) & 1u;
        any |= got;
        if (!got && ++seen == m) mth = s;
        if (s < nd) e += !got;
        else p += got;
    }
    *cut = nack_cut(nd, m, e, mth);
    return nack_class(nd, k, e, p, any);
}
// A needing block's requests (one chain, flag SEGMENT), block b of the call.  source(w): word w of
// what nack_request_word reads, the block's reception mask (or, for an advertisement, the sender's
// repair mask inverted: suppress_layout.hpp).
template <class Source>
inline void nack_block_emit_words(Source source, uint32_t nd, NackCut cut, uint32_t b, const NackFormat& f, NackWriter& o)
{
    NackChain c;
    uint32_t run = 0;
    for (uint32_t s = cut.lo; s <= cut.hi; ++s) {
        const bool in = s < cut.hi && ((nack_request_word(source(s >> 5), s >> 5, cut) >> (s & 31u)) & 1u);
        if (in) {
            ++run;
        } else if (run) {
            nack_unit(o, c, f, REPAIR_SEGMENT, run, b, s - run, nd, b, s - 1u, nd);
            run = 0;
        }
    }
    nack_close(o, c, f, REPAIR_SEGMENT);
}
inline void nack_block_emit_host(const uint32_t* mask, uint32_t nd, NackCut cut, uint32_t b, const NackFormat& f, NackWriter& o)
{
    nack_block_emit_words([mask](uint32_t w) { return mask[w]; }, nd, cut, b, f, o);
}

// ---- the parser (NormRepairRequest::Unpack, normMessage.cpp:279-305, and ::Iterator, :335-358) ----

struct NackItem {
    uint32_t object_id, block_id, block_len, symbol;
};
// Reads the requests of content[0, bytes).  Unit u < capacity gets unit_flags[u], unit_form[u] and
// first[u] / last[u] (an item of an ITEMS request is a unit with first = last; the arrays may be
// null).  Stops at a header that does not fit or whose length exceeds what is left, at a RANGES
// request with an odd item count, and at an item (a range: either item) with a foreign fec_id; a
// request's bytes behind its last whole item are skipped as the reference's iterator skips them.
// Returns the units read before the stop, *consumed the offset of the header or item it stopped at.
inline uint64_t nack_parse(uint32_t fec_id, uint32_t id_kind, const uint8_t* content, uint64_t bytes, uint8_t* unit_flags,
                           uint8_t* unit_form, NackItem* first, NackItem* last, uint64_t capacity, uint64_t* consumed)
{
    const uint32_t L = nack_item_length(id_kind);
    uint64_t at = 0, units = 0;
    auto word = [&](uint64_t o) {
        return (uint32_t)content[o] | ((uint32_t)content[o + 1] << 8) | ((uint32_t)content[o + 2] << 16) | ((uint32_t)content[o + 3] << 24);
    };
    auto item = [&](uint64_t o) {
        const RxId id = rx_id_decode(id_kind, word(o + 4), L == 12 ? word(o + 8) : 0u, 0u);
        NackItem it;
        it.object_id = ((uint32_t)content[o + 2] << 8) | content[o + 3];
        it.block_id = id.block, it.block_len = id.block_len, it.symbol = id.symbol;
        return it;
    };
    while (bytes - at >= 4) {
        const uint32_t form = content[at], flags = content[at + 1], len = ((uint32_t)content[at + 2] << 8) | content[at + 3];
        if (len > bytes - at - 4) break;
        const uint32_t count = len / L, step = form == REPAIR_RANGES ? 2u : 1u;
        if (form == REPAIR_RANGES && (count & 1u)) break;
        uint64_t o = at + 4;
        bool foreign = false;
        for (uint32_t i = 0; i < count; i += step, o += (uint64_t)step * L) {
            if (content[o] != fec_id || (step == 2 && content[o + L] != fec_id)) {
                foreign = true;
                break;
            }
            if (units < capacity) {
                if (unit_flags) unit_flags[units] = (uint8_t)flags;
                if (unit_form) unit_form[units] = (uint8_t)form;
                if (first) first[units] = item(o);
                if (last) last[units] = item(o + (uint64_t)(step - 1u) * L);
            }
            ++units;
        }
        if (foreign) {
            at = o;
            break;
        }
        at += 4u + (uint64_t)len;
    }
    if (consumed) *consumed = at;
    return units;
}

}  // namespace nfec
