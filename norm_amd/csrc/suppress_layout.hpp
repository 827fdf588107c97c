// suppress_layout.hpp -- NACK suppression and repair advertisements (nfec.h, "NACK suppression and
// repair advertisements on the device"): what a unit of overheard repair-request content does to a
// receiver's suppression state, which blocks are still pending behind it, whether the receiver
// sends, and where the class and the request words of a block come from when the sender advertises
// its repair state.  Shared by the host entries (suppress_host.cpp, nack_host.cpp) and the kernels
// (kernels_suppress.hip, kernels_nack.hip): what the CPU tests check of the rule is what the
// kernels run.
//
// Reference: NormSenderNode::HandleRepairContent (src/common/normNode.cpp:1069-1187),
// NormObject::SetRepairs / SetRepairInfo (include/normObject.h:274-279), NormBlock::SetRepairs
// (include/normSegment.h:216-222), NormObject::IsRepairPending (src/common/normObject.cpp:1137-1177),
// NormBlock::IsRepairPending (src/common/normSegment.cpp:174-216), NormObject::AppendRepairAdv
// (normObject.cpp:540-683), NormBlock::AppendRepairAdv (normSegment.cpp:405-493) and
// NormSession::SenderBuildRepairAdv (src/common/normSession.cpp:4598-4708).
#pragma once

#include "repair_layout.hpp"

namespace nfec {

// the receiver's object word (NFEC_RX_REPAIR_OBJECT / _INFO)
enum { RXR_OBJECT = 1u, RXR_INFO = 2u };

// ---- HandleRepairContent: what a unit sets ----

// The bits a unit of this object sets in the object word (normNode.cpp:1131-1146, :1157, :1172):
// an INFO-level unit and a BLOCK- or SEGMENT-level unit of a request that carries INFO set
// repair_info (the SEGMENT-level one whether or not a block is found: SetRepairInfo stands in
// front of FindBlock); an OBJECT-level unit names the object and its INFO flag is not looked at.
NFEC_ID_HD inline uint32_t suppress_object_bits(uint32_t level, uint32_t flags)
{
    if (level == LEVEL_OBJECT) return RXR_OBJECT;
    if (level == LEVEL_INFO) return RXR_INFO;
    if (level == LEVEL_BLOCK || level == LEVEL_SEGMENT) return flags & REPAIR_INFO ? (uint32_t)RXR_INFO : 0u;
    return 0u;
}
// Does a BLOCK-level unit over the blocks [b0, b1] set anything, and up to which block?
NFEC_ID_HD inline bool suppress_block_range(uint32_t b0, uint32_t b1, uint32_t nblocks, uint32_t* hi)
{
    if (b0 > b1 || b0 >= nblocks) return false;
    *hi = b1 < nblocks - 1u ? b1 : nblocks - 1u;
    return true;
}
// the bits of block_repair word w for the blocks [lo, hi] (hi < 2^32 - 1: hi < nblocks)
NFEC_ID_HD inline uint32_t suppress_block_bits(uint32_t w, uint32_t lo, uint32_t hi) { return nack_range_bits(w, lo, hi + 1u); }
// A SEGMENT-level unit that repair_mark lets through is applied when its block is held: the
// receiver has a NormBlock exactly for its needing blocks (an absent block has none, a complete or
// decodable one was decoded and released), so FindBlock (normNode.cpp:1176) finds those alone.
NFEC_ID_HD inline bool suppress_block_held(uint32_t cls) { return cls == NACK_NEEDING; }
// the bits of repair word w an applied unit [first, last] sets, clipped at nd + m
NFEC_ID_HD inline uint32_t suppress_segment_bits(uint32_t w, uint32_t first, uint32_t last, uint32_t nd, uint32_t m)
{
    const uint32_t end = nd + m;
    return nack_range_bits(w, first, last + 1u < end ? last + 1u : end);
}

// ---- IsRepairPending: the decision at the end of the back-off ----

// Word w of what a needing block would ask for and nobody has asked for yet.  NormBlock::
// IsRepairPending presets the pending slots its request does not name and XCopies: what is left is
// the request set (nack_cut / nack_request_word) without the overheard repair bits.
NFEC_ID_HD inline uint32_t suppress_residual_word(uint32_t received, uint32_t repair, uint32_t w, NackCut cut)
{
    return nack_request_word(received, w, cut) & ~repair;
}
// Is a block of class cls pending?  block_bit: its block_repair bit; residual: some word of
// suppress_residual_word is not zero (a needing block's).
NFEC_ID_HD inline bool suppress_block_pending(uint32_t cls, bool block_bit, bool residual)
{
    if (cls == NACK_SILENT || block_bit) return false;
    return cls == NACK_ABSENT || residual;
}
// Does the receiver send? (OnRepairTimeout, normNode.cpp:2362-2390: an object named in
// rx_repair_mask is skipped; IsRepairPending, normObject.cpp:1140: pending_info && !repair_info)
NFEC_ID_HD inline bool suppress_sends(uint32_t object_word, bool info_pending, uint64_t pending_blocks)
{
    if (object_word & RXR_OBJECT) return false;
    return (info_pending && !(object_word & RXR_INFO)) || pending_blocks != 0;
}

// ---- AppendRepairAdv: the walk of nack_layout.hpp over the sender's repair state ----

// A block's class for the advertisement: a block whose block_repair bit is set is a whole block
// (what an absent block is to a NACK: normObject.cpp:581-586), one with a repair bit in [0, nd + m)
// has segment requests (:642-654), anything else says nothing.  `any`: some repair bit of [0, nd + m).
NFEC_ID_HD inline uint32_t adv_class(uint32_t nd, uint32_t k, bool block_bit, uint32_t any)
{
    if (nd < 1 || nd > k) return NACK_SILENT;
    if (block_bit) return NACK_ABSENT;
    return any ? NACK_NEEDING : NACK_SILENT;
}
// ... and its requested slots are its repair bits of [0, nd + m): with this cut and the repair
// word inverted, nack_request_word gives them (it asks for the clear bits of a reception mask).
NFEC_ID_HD inline NackCut adv_cut(uint32_t nd, uint32_t m) { return NackCut{0u, nd + m}; }
NFEC_ID_HD inline uint32_t adv_source_word(uint32_t repair) { return ~repair; }
// the request of an object that is repaired as a whole (normSession.cpp:4602, :4662): ITEMS, flag
// OBJECT without INFO, one item {object id, block 0, block length k, symbol 0}
NFEC_ID_HD inline bool adv_whole_object(uint32_t object_word) { return (object_word & TXR_OBJECT) != 0; }
NFEC_ID_HD inline uint32_t adv_info(uint32_t object_word) { return object_word & TXR_INFO ? (uint32_t)REPAIR_INFO : 0u; }

}  // namespace nfec
