// repair_layout.hpp -- the sender's repair state (nfec.h, "sender repair state on the device"): what
// a unit of a NACK's repair-request content does to a block's parity pair and repair mask, which
// units of a message form a stretch, what activation does to a block, and the end-of-block step.
// Shared by the host entries (tx_repair_host.cpp) and the kernels (kernels_txrepair.hip): what the
// CPU tests check of the rule is what the kernels run.
//
// Reference: NormSession::SenderHandleNackMessage, !holdoff (src/common/normSession.cpp:3706-4300),
// NormBlock::HandleSegmentRequest (src/common/normSegment.cpp:341-402), NormBlock::TxReset
// (:219-259), NormObject::ActivateRepairs (src/common/normObject.cpp:472-537) and ResetParityCount
// as NextSenderMsg calls it (:2079-2083).
#pragma once

#include "nack_layout.hpp"

namespace nfec {

enum { REPAIR_OBJECT = 0x08 };  // NormRepairRequest::OBJECT (normMessage.h:1562)
// the object word (NFEC_TX_REPAIR_OBJECT / _INFO, NFEC_TX_PENDING_INFO)
enum { TXR_OBJECT = 1u, TXR_INFO = 2u, TXR_PENDING_INFO = 4u };

// ---- a unit's level and whose it is ----

enum { LEVEL_NONE = 0, LEVEL_SEGMENT = 1, LEVEL_BLOCK = 2, LEVEL_OBJECT = 3, LEVEL_INFO = 4 };
// the reference's order (normSession.cpp:3763-3784)
NFEC_ID_HD inline uint32_t repair_level(uint32_t flags)
{
    return flags & REPAIR_SEGMENT ? LEVEL_SEGMENT
           : flags & REPAIR_BLOCK ? LEVEL_BLOCK
           : flags & REPAIR_OBJECT ? LEVEL_OBJECT
           : flags & REPAIR_INFO ? LEVEL_INFO
                                 : LEVEL_NONE;
}
// is a unit of `level` whose items name the objects first_obj / last_obj a unit of object_id?
NFEC_ID_HD inline bool repair_own(uint32_t level, uint32_t object_id, uint32_t first_obj, uint32_t last_obj)
{
    if (level == LEVEL_OBJECT || level == LEVEL_INFO)
        return ((object_id - first_obj) & 0xffffu) <= ((last_obj - first_obj) & 0xffffu);
    return first_obj == (object_id & 0xffffu);
}
// the block of the batch of a block id as the wire holds it (rx_id_decode's inverse of first_block_id + b)
NFEC_ID_HD inline uint32_t repair_block_of(uint32_t id_kind, uint32_t block_id, uint32_t first_block_id)
{
    const uint32_t d = block_id - first_block_id;
    return id_kind == PAYLOAD_ID_BLOCK24 ? d & 0x00ffffffu : id_kind == PAYLOAD_ID_BLOCK16 ? d & 0xffffu : d;
}

// ---- the stretch rule over a message ----
//
// What a unit is to the SEGMENT-level unit behind it: transparent (a BLOCK-, OBJECT- or INFO-level
// unit of this object, or a unit of a request without a level), a break (a foreign unit, or a
// SEGMENT-level unit that cannot be applied whatever the state holds), or a SEGMENT-level unit for
// block b that is applied unless its stretch meets a set block_repair bit.
enum { MARK_TRANSPARENT = 0, MARK_BREAK = 1, MARK_SEGMENT = 2 };
struct UnitMark {
    uint32_t kind, block;
};
// nd: the block's numData where level is SEGMENT and b < nblocks
NFEC_ID_HD inline UnitMark repair_mark(uint32_t level, bool own, uint32_t b, uint32_t nblocks, uint32_t nd, uint32_t k,
                                       uint32_t first_symbol, uint32_t last_symbol)
{
    if (level == LEVEL_NONE) return UnitMark{MARK_TRANSPARENT, 0u};
    if (!own) return UnitMark{MARK_BREAK, 0u};
    if (level != LEVEL_SEGMENT) return UnitMark{MARK_TRANSPARENT, 0u};
    if (b >= nblocks || nd < 1 || nd > k || last_symbol < first_symbol) return UnitMark{MARK_BREAK, 0u};
    return UnitMark{MARK_SEGMENT, b};
}
// The last mark that was not transparent, as one word the scans can carry: a break is all ones (no
// block of a batch has that index: nblocks fits 32 bits), a SEGMENT-level unit its block.
constexpr uint32_t kMarkBreak = 0xffffffffu;
NFEC_ID_HD inline uint32_t repair_mark_word(UnitMark mk) { return mk.kind == MARK_SEGMENT ? mk.block : kMarkBreak; }
// A SEGMENT-level unit for block b opens a stretch (is fresh) unless the last mark in front of it
// is a SEGMENT-level unit for b.  (That unit was applied, or it met the block_repair bit, and then
// this one meets it too: the bit is never cleared by handling.)
NFEC_ID_HD inline bool repair_opens_stretch(uint32_t last_mark_word, uint32_t b) { return last_mark_word != b; }

// A unit's key in the order of the call: message index, then index in the message (a message holds
// at most 65535 bytes, so fewer than 2^16 units).
NFEC_ID_HD inline uint64_t repair_key(uint64_t message, uint32_t index) { return (message << 16) | index; }

// ---- NormBlock::HandleSegmentRequest on (parity pair, mask) ----

struct ParityPair {
    uint32_t offset, count;
};
// the slots a unit sets: [lo0, hi0) and [lo1, hi1), clipped at nd + m (either may be empty)
struct RepairSlots {
    uint32_t lo0, hi0, lo1, hi1;
};
NFEC_ID_HD inline RepairSlots repair_segment_request(ParityPair& p, uint32_t first, uint32_t last, uint32_t nd, uint32_t m,
                                                     uint32_t E)
{
    const uint32_t end = nd + m;
    RepairSlots r = {0u, 0u, 0u, 0u};
    auto named = [&](uint64_t from) {  // the slots [from, last], explicitly
        r.lo1 = (uint32_t)(from < end ? from : end);
        r.hi1 = last + 1u < end ? last + 1u : end;
        if (r.hi1 < r.lo1) r.hi1 = r.lo1;
    };
    if (first < nd) {
        p.offset = p.count = m;  // explicit data repair: no parity repair this cycle
        named(first);
        return r;
    }
    const uint32_t avail = p.offset < m ? m - p.offset : 0u;
    if (E <= avail) {
        if (E > p.count) {  // fresh parity
            r.lo0 = nd + p.offset + p.count, r.hi0 = nd + p.offset + E;
            p.count = E;
        }
    } else {
        uint64_t from = first;
        if (p.count < avail) {  // any remaining fresh parity ...
            r.lo0 = nd + p.offset + p.count, r.hi0 = end;
            p.count = avail;
            from += avail;
        }
        named(from);  // ... and explicit repair for the rest
    }
    return r;
}
// the bits of mask word w a unit sets
NFEC_ID_HD inline uint32_t repair_slot_bits(uint32_t w, RepairSlots r)
{
    return nack_range_bits(w, r.lo0, r.hi0) | nack_range_bits(w, r.lo1, r.hi1);
}

// ---- activation, per mask word ----

NFEC_ID_HD inline uint32_t repair_valid_bits(uint32_t w, uint32_t nd, uint32_t m) { return nack_range_bits(w, 0u, nd + m); }
// NormBlock::TxReset: does word w of the pending mask differ from the bits [0, nd + auto_parity)?
NFEC_ID_HD inline bool repair_reset_differs(uint32_t pending, uint32_t w, uint32_t nd, uint32_t m, uint32_t auto_parity)
{
    return (pending & repair_valid_bits(w, nd, m)) != nack_range_bits(w, 0u, nd + auto_parity);
}
// ... the word after a reset with a change
NFEC_ID_HD inline uint32_t repair_reset_word(uint32_t pending, uint32_t w, uint32_t nd, uint32_t m, uint32_t auto_parity)
{
    return (pending & ~repair_valid_bits(w, nd, m)) | nack_range_bits(w, 0u, nd + auto_parity);
}
// what activation does to one block: reset it (object bit, or its block_repair bit), activate its
// segment repairs (no object bit)
NFEC_ID_HD inline bool repair_block_resets(uint32_t object_word, bool block_bit) { return (object_word & TXR_OBJECT) || block_bit; }
NFEC_ID_HD inline bool repair_block_activates(uint32_t object_word) { return !(object_word & TXR_OBJECT); }
// the object word behind an activation in which `changed` blocks were reset with a change
NFEC_ID_HD inline uint32_t repair_object_after(uint32_t object_word, uint64_t changed)
{
    uint32_t w = object_word & ~(uint32_t)(TXR_OBJECT | TXR_INFO);
    if ((object_word & TXR_INFO) || changed) w |= TXR_PENDING_INFO;
    return w;
}

// ---- end of block (ResetParityCount) ----

NFEC_ID_HD inline ParityPair repair_end_block(ParityPair p, uint32_t m)
{
    const uint32_t sum = p.offset + p.count;
    return ParityPair{sum < m ? sum : m, 0u};
}

}  // namespace nfec
