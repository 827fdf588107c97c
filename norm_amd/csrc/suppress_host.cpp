// suppress_host.cpp -- NACK suppression on the host (no GPU, no codec): overheard repair-request
// content into a receiver's suppression state, and the decision at the end of the back-off, as
// loops over the rule of suppress_layout.hpp.  The kernels of nfec_rx_handle_repair_content and
// nfec_rx_repair_pending (kernels_suppress.hip) run the same functions.  (The advertisement's
// host entry stands beside the walk it shares, in nack_host.cpp.)
//
// Reference: NormSenderNode::HandleRepairContent (src/common/normNode.cpp:1069-1187),
// NormSenderNode::OnRepairTimeout (:2362-2390), NormObject::IsRepairPending
// (src/common/normObject.cpp:1137-1177), NormBlock::IsRepairPending (src/common/normSegment.cpp:174-216).
#include "nfec_internal.hpp"
#include "suppress_layout.hpp"

#include <vector>

using namespace nfec;

namespace nfec {

int rx_repair_check(uint32_t k, uint32_t m, uint32_t nblocks, uint32_t mask_stride, const uint32_t* received,
                    const nfec_rx_repair_state* state, const uint64_t* totals, const char* what)
{
    if (k == 0 || m == 0 || (uint64_t)k + m > 65536) return fail(NFEC_EINVAL, std::string(what) + ": bad k or m");
    if (!state) return fail(NFEC_EINVAL, std::string(what) + ": null state");
    if (nblocks && (!state->repair || !state->block_repair || !state->object))
        return fail(NFEC_EINVAL, std::string(what) + ": null state array");
    if (nblocks && !received) return fail(NFEC_EINVAL, std::string(what) + ": null received mask");
    if ((uint64_t)mask_stride * 32u < (uint64_t)k + m)
        return fail(NFEC_EINVAL, std::string(what) + ": mask_stride smaller than (k + m + 31) / 32");
    if (!totals) return fail(NFEC_EINVAL, std::string(what) + ": null totals");
    return NFEC_OK;
}

int rx_content_check(const nfec_rx_messages* messages, uint8_t fec_id, uint8_t fec_m, uint32_t* id_kind)
{
    if (!messages) return fail(NFEC_EINVAL, "rx_handle_repair_content: null messages");
    *id_kind = payload_id_kind(fec_id, fec_m);
    if (*id_kind == PAYLOAD_ID_NONE) return fail(NFEC_EINVAL, "rx_handle_repair_content: bad fec_id / fec_m");
    if (messages->count && (!messages->payloads || !messages->offsets || !messages->length))
        return fail(NFEC_EINVAL, "rx_handle_repair_content: null messages array");
    return NFEC_OK;
}

}  // namespace nfec

extern "C" int nfec_rx_handle_repair_content_host(uint32_t k, uint32_t m, const nfec_rx_messages* messages, uint8_t fec_id,
                                                  uint8_t fec_m, uint16_t object_id, uint32_t first_block_id,
                                                  const uint32_t* received, uint32_t mask_stride, const uint16_t* num_data,
                                                  uint32_t nblocks, const nfec_rx_repair_state* state, uint64_t* totals)
{
    uint32_t kind = 0;
    int rc = rx_content_check(messages, fec_id, fec_m, &kind);
    if (rc || (rc = rx_repair_check(k, m, nblocks, mask_stride, received, state, totals, "rx_handle_repair_content_host"))) return rc;
    for (int j = 0; j < 6; ++j) totals[j] = 0;
    if (messages->count == 0 || nblocks == 0) return NFEC_OK;
    const uint64_t count = messages->count_dev ? std::min<uint64_t>(messages->count, *messages->count_dev) : messages->count;
    const uint8_t* wire = static_cast<const uint8_t*>(messages->payloads);
    std::vector<uint8_t> flags;
    std::vector<NackItem> first, last;
    uint64_t units = 0, applied = 0, ignored = 0, newly = 0, cut_short = 0, unreadable = 0;
    for (uint64_t i = 0; i < count; ++i) {
        const uint64_t off = messages->offsets[i];
        const uint32_t len = messages->length[i];
        if (!rx_readable(off, len, 0u, messages->payload_bytes)) {
            ++unreadable;
            continue;
        }
        uint64_t consumed = 0;
        const uint64_t n = nack_parse(fec_id, kind, wire + off, len, nullptr, nullptr, nullptr, nullptr, 0, &consumed);
        flags.resize(n), first.resize(n), last.resize(n);
        nack_parse(fec_id, kind, wire + off, len, flags.data(), nullptr, first.data(), last.data(), n, nullptr);
        units += n, cut_short += consumed != len;
        for (uint64_t u = 0; u < n; ++u) {
            const uint32_t level = repair_level(flags[u]);
            const bool own = level != LEVEL_NONE && repair_own(level, object_id, first[u].object_id, last[u].object_id);
            if (!own) {
                ++ignored;
                continue;
            }
            *state->object |= suppress_object_bits(level, flags[u]);
            const uint32_t b0 = repair_block_of(kind, first[u].block_id, first_block_id);
            if (level == LEVEL_BLOCK) {
                uint32_t hi = 0;
                if (suppress_block_range(b0, repair_block_of(kind, last[u].block_id, first_block_id), nblocks, &hi))
                    for (uint32_t w = b0 >> 5; w <= hi >> 5; ++w) {
                        const uint32_t bits = suppress_block_bits(w, b0, hi);
                        newly += __builtin_popcount(bits & ~state->block_repair[w]);
                        state->block_repair[w] |= bits;
                    }
            }
            if (level != LEVEL_SEGMENT) continue;
            const uint32_t nd = b0 < nblocks ? (num_data ? num_data[b0] : k) : 0u;
            const UnitMark mk = repair_mark(level, own, b0, nblocks, nd, k, first[u].symbol, last[u].symbol);
            NackCut cut;
            if (mk.kind != MARK_SEGMENT ||
                !suppress_block_held(nack_block_class_host(received + (size_t)b0 * mask_stride, nd, k, m, &cut))) {
                ++ignored;
                continue;
            }
            uint32_t* mask = state->repair + (size_t)b0 * mask_stride;
            for (uint32_t w = 0; w < (nd + m + 31u) / 32u; ++w) mask[w] |= suppress_segment_bits(w, first[u].symbol, last[u].symbol, nd, m);
            ++applied;
        }
    }
    totals[0] = units, totals[1] = applied, totals[2] = ignored, totals[3] = newly, totals[4] = cut_short, totals[5] = unreadable;
    return NFEC_OK;
}

extern "C" int nfec_rx_repair_pending_host(uint32_t k, uint32_t m, const uint32_t* received, uint32_t mask_stride,
                                           const uint16_t* num_data, uint32_t nblocks, const nfec_rx_repair_state* state,
                                           uint32_t flags, uint32_t* pending_blocks, uint64_t* totals)
{
    int rc = rx_repair_check(k, m, nblocks, mask_stride, received, state, totals, "rx_repair_pending_host");
    if (rc) return rc;
    if (flags & ~(uint32_t)NFEC_NACK_INFO) return fail(NFEC_EINVAL, "rx_repair_pending_host: unknown flags");
    for (int j = 0; j < 4; ++j) totals[j] = 0;
    if (nblocks == 0) return NFEC_OK;
    if (pending_blocks)
        for (uint32_t w = 0; w < (nblocks + 31u) / 32u; ++w) pending_blocks[w] = 0;
    for (uint32_t b = 0; b < nblocks; ++b) {
        const uint32_t nd = num_data ? num_data[b] : k;
        const uint32_t* mask = received + (size_t)b * mask_stride;
        const uint32_t* rep = state->repair + (size_t)b * mask_stride;
        NackCut cut = {0, 0};
        const uint32_t cls = nack_block_class_host(mask, nd, k, m, &cut);
        const bool bit = (state->block_repair[b >> 5] >> (b & 31u)) & 1u;
        uint32_t residual = 0;
        if (cls == NACK_NEEDING)
            for (uint32_t w = 0; w < (nd + m + 31u) / 32u; ++w) residual |= suppress_residual_word(mask[w], rep[w], w, cut);
        if (suppress_block_pending(cls, bit, residual != 0)) {
            ++totals[1];
            if (pending_blocks) pending_blocks[b >> 5] |= 1u << (b & 31u);
        } else {
            totals[2] += cls == NACK_NEEDING, totals[3] += cls == NACK_ABSENT;
        }
    }
    totals[0] = suppress_sends(*state->object, (flags & NFEC_NACK_INFO) != 0, totals[1]);
    return NFEC_OK;
}
