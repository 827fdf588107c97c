// tx_repair_host.cpp -- the sender's repair state on the host (no GPU, no codec): the NACKs of a
// repair cycle into the repair state, its activation into the pending masks, and the end-of-block
// step, as loops over the rule of repair_layout.hpp.  The kernels of nfec_tx_handle_nacks,
// nfec_tx_activate_repairs and nfec_tx_end_blocks (kernels_txrepair.hip) run the same functions.
//
// Reference: NormSession::SenderHandleNackMessage, !holdoff (src/common/normSession.cpp:3706-4300),
// NormSession::OnRepairTimeout (:4720-4750), NormObject::NextSenderMsg (src/common/normObject.cpp:2079-2083).
#include "nfec_internal.hpp"
#include "repair_layout.hpp"

#include <vector>

using namespace nfec;

namespace nfec {

int tx_repair_check(uint32_t k, uint32_t m, uint32_t nblocks, uint32_t mask_stride, const nfec_tx_repair_state* state,
                    const char* what)
{
    if (k == 0 || m == 0 || (uint64_t)k + m > 65536) return fail(NFEC_EINVAL, std::string(what) + ": bad k or m");
    if (!state) return fail(NFEC_EINVAL, std::string(what) + ": null state");
    if (nblocks && (!state->repair || !state->parity || !state->block_repair || !state->object))
        return fail(NFEC_EINVAL, std::string(what) + ": null state array");
    if ((uint64_t)mask_stride * 32u < (uint64_t)k + m)
        return fail(NFEC_EINVAL, std::string(what) + ": mask_stride smaller than (k + m + 31) / 32");
    return NFEC_OK;
}

int tx_nack_check(const nfec_rx_messages* nacks, uint8_t fec_id, uint8_t fec_m, uint32_t extra_parity, const uint64_t* totals,
                  uint32_t* id_kind)
{
    if (!nacks) return fail(NFEC_EINVAL, "tx_handle_nacks: null nacks");
    *id_kind = payload_id_kind(fec_id, fec_m);
    if (*id_kind == PAYLOAD_ID_NONE) return fail(NFEC_EINVAL, "tx_handle_nacks: bad fec_id / fec_m");
    if (nacks->count && (!nacks->payloads || !nacks->offsets || !nacks->length))
        return fail(NFEC_EINVAL, "tx_handle_nacks: null nacks array");
    if (extra_parity > 65535u) return fail(NFEC_EINVAL, "tx_handle_nacks: extra_parity above 65535");
    if (!totals) return fail(NFEC_EINVAL, "tx_handle_nacks: null totals");
    return NFEC_OK;
}

}  // namespace nfec

extern "C" int nfec_tx_handle_nacks_host(uint32_t k, uint32_t m, const nfec_rx_messages* nacks, uint8_t fec_id, uint8_t fec_m,
                                         uint16_t object_id, uint32_t first_block_id, const uint16_t* num_data,
                                         uint32_t nblocks, uint32_t mask_stride, uint32_t extra_parity,
                                         const nfec_tx_repair_state* state, uint32_t unit_capacity, uint64_t* totals)
{
    uint32_t kind = 0;
    int rc = tx_nack_check(nacks, fec_id, fec_m, extra_parity, totals, &kind);
    if (rc || (rc = tx_repair_check(k, m, nblocks, mask_stride, state, "tx_handle_nacks_host"))) return rc;
    for (int j = 0; j < 6; ++j) totals[j] = 0;
    if (nacks->count == 0 || nblocks == 0) return NFEC_OK;
    const uint64_t count = nacks->count_dev ? std::min<uint64_t>(nacks->count, *nacks->count_dev) : nacks->count;
    const uint8_t* wire = static_cast<const uint8_t*>(nacks->payloads);

    // the units of the call: nothing is applied unless all of them fit
    uint64_t units = 0, cut = 0, unreadable = 0;
    for (uint64_t i = 0; i < count; ++i) {
        const uint64_t off = nacks->offsets[i];
        const uint32_t len = nacks->length[i];
        if (!rx_readable(off, len, 0u, nacks->payload_bytes)) {
            ++unreadable;
            continue;
        }
        uint64_t consumed = 0;
        units += nack_parse(fec_id, kind, wire + off, len, nullptr, nullptr, nullptr, nullptr, 0, &consumed);
        cut += consumed != len;
    }
    totals[0] = units, totals[4] = cut, totals[5] = unreadable;
    if (units > unit_capacity) return NFEC_OK;

    std::vector<uint8_t> flags;
    std::vector<NackItem> first, last;
    uint64_t applied = 0, ignored = 0, newly = 0;
    uint32_t object_word = *state->object;
    auto block_bit = [&](uint32_t b) { return (state->block_repair[b >> 5] >> (b & 31u)) & 1u; };
    for (uint64_t i = 0; i < count; ++i) {
        const uint64_t off = nacks->offsets[i];
        const uint32_t len = nacks->length[i];
        if (!rx_readable(off, len, 0u, nacks->payload_bytes)) continue;
        const uint64_t n = nack_parse(fec_id, kind, wire + off, len, nullptr, nullptr, nullptr, nullptr, 0, nullptr);
        flags.resize(n), first.resize(n), last.resize(n);
        nack_parse(fec_id, kind, wire + off, len, flags.data(), nullptr, first.data(), last.data(), n, nullptr);
        bool prev_applied = false;  // the previous SEGMENT-level unit was applied, and to prev_block
        uint32_t prev_block = 0, E = 0;
        for (uint64_t u = 0; u < n; ++u) {
            const uint32_t level = repair_level(flags[u]);
            const bool own = level != LEVEL_NONE && repair_own(level, object_id, first[u].object_id, last[u].object_id);
            const uint32_t b0 = repair_block_of(kind, first[u].block_id, first_block_id);
            const uint32_t nd = level == LEVEL_SEGMENT && b0 < nblocks ? (num_data ? num_data[b0] : k) : 0u;
            const UnitMark mk = repair_mark(level, own, b0, nblocks, nd, k, first[u].symbol, last[u].symbol);
            if (level == LEVEL_NONE) {
                ++ignored;
                continue;
            }
            if (!own) {
                ++ignored, prev_applied = false;
                continue;
            }
            if (flags[u] & REPAIR_INFO) object_word |= TXR_INFO;
            if (level == LEVEL_OBJECT) object_word |= TXR_OBJECT;
            if (level == LEVEL_BLOCK) {
                const uint32_t b1 = repair_block_of(kind, last[u].block_id, first_block_id);
                if (b0 <= b1 && b0 < nblocks)
                    for (uint32_t b = b0; b <= std::min(b1, nblocks - 1u); ++b) {
                        newly += !block_bit(b);
                        state->block_repair[b >> 5] |= 1u << (b & 31u);
                    }
            }
            if (level != LEVEL_SEGMENT) continue;
            const bool fresh = !(prev_applied && prev_block == b0);
            if (mk.kind != MARK_SEGMENT || (fresh && block_bit(b0))) {
                ++ignored, prev_applied = false;
                continue;
            }
            if (fresh) E = extra_parity;
            E += last[u].symbol - first[u].symbol + 1u;
            uint16_t* pair = state->parity + 2 * (size_t)b0;
            ParityPair p = {pair[0], pair[1]};
            const RepairSlots r = repair_segment_request(p, first[u].symbol, last[u].symbol, nd, m, E);
            pair[0] = (uint16_t)p.offset, pair[1] = (uint16_t)p.count;
            uint32_t* mask = state->repair + (size_t)b0 * mask_stride;
            for (uint32_t w = 0; w < (nd + m + 31u) / 32u; ++w) mask[w] |= repair_slot_bits(w, r);
            ++applied, prev_applied = true, prev_block = b0;
        }
    }
    *state->object = object_word;
    totals[1] = applied, totals[2] = ignored, totals[3] = newly;
    return NFEC_OK;
}

extern "C" int nfec_tx_activate_repairs_host(uint32_t k, uint32_t m, const uint16_t* num_data, uint32_t nblocks,
                                             uint32_t auto_parity, uint32_t* pending, uint32_t mask_stride,
                                             const nfec_tx_repair_state* state, uint64_t* totals)
{
    int rc = tx_repair_check(k, m, nblocks, mask_stride, state, "tx_activate_repairs_host");
    if (rc) return rc;
    if (!totals || (nblocks && !pending)) return fail(NFEC_EINVAL, "tx_activate_repairs_host: null pending or totals");
    if (auto_parity > m) return fail(NFEC_EINVAL, "tx_activate_repairs_host: auto_parity above m");
    totals[0] = totals[1] = totals[2] = 0;
    if (nblocks == 0) return NFEC_OK;
    const uint32_t object_word = *state->object;
    for (uint32_t b = 0; b < nblocks; ++b) {
        const uint32_t nd = num_data ? num_data[b] : k;
        if (nd < 1 || nd > k) continue;
        const uint32_t words = (nd + m + 31u) / 32u;
        uint32_t* pend = pending + (size_t)b * mask_stride;
        uint32_t* rep = state->repair + (size_t)b * mask_stride;
        if (repair_block_resets(object_word, (state->block_repair[b >> 5] >> (b & 31u)) & 1u)) {
            bool differs = false;
            for (uint32_t w = 0; w < words; ++w) differs |= repair_reset_differs(pend[w], w, nd, m, auto_parity);
            for (uint32_t w = 0; w < words; ++w) {
                if (differs) pend[w] = repair_reset_word(pend[w], w, nd, m, auto_parity);
                rep[w] &= ~repair_valid_bits(w, nd, m);
            }
            if (differs) state->parity[2 * (size_t)b] = (uint16_t)auto_parity, state->parity[2 * (size_t)b + 1] = (uint16_t)m;
            totals[0] += differs;
        }
        if (repair_block_activates(object_word)) {
            bool any = false;
            for (uint32_t w = 0; w < words; ++w) {
                const uint32_t bits = rep[w] & repair_valid_bits(w, nd, m);
                any |= bits != 0;
                pend[w] |= bits, rep[w] &= ~bits;
            }
            totals[1] += any;
        }
        for (uint32_t w = 0; w < words; ++w) totals[2] += __builtin_popcount(pend[w] & repair_valid_bits(w, nd, m));
    }
    for (uint32_t w = 0; w < (nblocks + 31u) / 32u; ++w) state->block_repair[w] = 0;
    *state->object = repair_object_after(object_word, totals[0]);
    return NFEC_OK;
}

extern "C" int nfec_tx_end_blocks_host(uint32_t k, uint32_t m, const uint16_t* num_data, uint32_t nblocks,
                                       const uint32_t* pending, uint32_t mask_stride, const nfec_tx_repair_state* state)
{
    if (k == 0 || m == 0 || (uint64_t)k + m > 65536) return fail(NFEC_EINVAL, "tx_end_blocks_host: bad k or m");
    if (!state || (nblocks && (!state->parity || !pending))) return fail(NFEC_EINVAL, "tx_end_blocks_host: null pending or state");
    if ((uint64_t)mask_stride * 32u < (uint64_t)k + m)
        return fail(NFEC_EINVAL, "tx_end_blocks_host: mask_stride smaller than (k + m + 31) / 32");
    for (uint32_t b = 0; b < nblocks; ++b) {
        const uint32_t nd = num_data ? num_data[b] : k;
        if (nd < 1 || nd > k) continue;
        uint32_t any = 0;
        for (uint32_t w = 0; w < (nd + m + 31u) / 32u; ++w) any |= pending[(size_t)b * mask_stride + w] & repair_valid_bits(w, nd, m);
        if (any) continue;
        uint16_t* pair = state->parity + 2 * (size_t)b;
        const ParityPair p = repair_end_block(ParityPair{pair[0], pair[1]}, m);
        pair[0] = (uint16_t)p.offset, pair[1] = (uint16_t)p.count;
    }
    return NFEC_OK;
}
