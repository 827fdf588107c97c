// nack_host.cpp -- the repair-request content of a NORM_NACK from reception masks, on the host (no
// GPU), and the parser of such content.
//
// The walk NormObject::AppendRepairRequest makes with flush set (reference
// src/common/normObject.cpp:1179-1381): blocks ascending; a run of blocks without a NormBlock
// becomes one BLOCK-level unit where the walk learns that the run has ended (:1210-1213), a block
// that still needs segments closes the open BLOCK request and appends its own SEGMENT requests
// (NormBlock::AppendRepairRequest, src/common/normSegment.cpp:524-630).  nack_layout.hpp holds the
// rule; the kernels of nfec_rx_repair_requests (kernels_nack.hip) apply it to masks in device memory.
// NormObject::AppendRepairAdv (:540-683) makes the same walk over the sender's repair state:
// nfec_tx_repair_adv_host runs it here with the classes and words of suppress_layout.hpp.
#include "nack_layout.hpp"
#include "nfec_internal.hpp"
#include "suppress_layout.hpp"

using namespace nfec;

namespace nfec {

int nack_format(uint8_t fec_id, uint8_t fec_m, uint16_t object_id, uint32_t first_block_id, uint32_t flags,
                uint32_t max_units, NackFormat* f)
{
    f->id_kind = payload_id_kind(fec_id, fec_m);
    if (f->id_kind == PAYLOAD_ID_NONE) return fail(NFEC_EINVAL, "repair_requests: bad fec_id / fec_m");
    if (flags & ~(uint32_t)NFEC_NACK_INFO) return fail(NFEC_EINVAL, "repair_requests: unknown flags");
    if (max_units == 0 || max_units > nack_max_units_limit(f->id_kind))
        return fail(NFEC_EINVAL, "repair_requests: max_units outside [1, 65535 / (2 * item length)]");
    f->item_len = nack_item_length(f->id_kind);
    f->fec_id = fec_id;
    f->object_id = object_id;
    f->first_block_id = first_block_id;
    f->info = (flags & NFEC_NACK_INFO) ? (uint32_t)REPAIR_INFO : 0u;
    f->max_units = max_units;
    return NFEC_OK;
}

}  // namespace nfec

namespace {

// The walk over the blocks, whatever a block's class and request words come from: a reception mask
// (AppendRepairRequest) or the sender's repair state (AppendRepairAdv, normObject.cpp:540-683, the
// same walk).  classify(b, nd, &cut): the block's class and, for class 1, its cut; source(b): what
// nack_block_emit_words reads the block's words from.
template <class Classify, class Source>
void nack_walk_host(Classify classify, Source source, uint32_t k, const uint16_t* num_data, uint32_t nblocks, const NackFormat& f,
                    void* content, uint64_t capacity, uint64_t* block_start, uint64_t* totals)
{
    // the classes first: a run of absent blocks ends where the next block is not absent
    uint64_t needing = 0, absent = 0;
    NackCut cut = {0, 0};
    for (uint32_t b = 0; b < nblocks; ++b) {
        const uint32_t cls = classify(b, num_data ? num_data[b] : k, &cut);
        block_start[2 * (size_t)b + 1] = cls;
        needing += cls == NACK_NEEDING, absent += cls == NACK_ABSENT;
    }
    NackWriter o;
    o.content = static_cast<uint8_t*>(content), o.capacity = capacity;
    NackChain chain;
    uint64_t run = 0;
    for (uint32_t b = 0; b < nblocks; ++b) {
        block_start[2 * (size_t)b] = o.off;
        const uint32_t cls = (uint32_t)block_start[2 * (size_t)b + 1];
        const uint32_t nd = num_data ? num_data[b] : k;
        if (cls == NACK_ABSENT) {
            ++run;
            if (b + 1 == nblocks || block_start[2 * (size_t)b + 3] != NACK_ABSENT) {
                const uint32_t b0 = b - (uint32_t)(run - 1u);
                nack_unit(o, chain, f, REPAIR_BLOCK, run, b0, 0, num_data ? num_data[b0] : k, b, 0, nd);
                run = 0;
            }
        } else if (cls == NACK_NEEDING) {
            nack_close(o, chain, f, REPAIR_BLOCK);
            classify(b, nd, &cut);
            nack_block_emit_words(source(b), nd, cut, b, f, o);
        }
    }
    nack_close(o, chain, f, REPAIR_BLOCK);
    if (o.off == 0 && f.info && nblocks) {  // the INFO-only request (normObject.cpp:1365-1372, :670-681): block 0, length 0, symbol 0
        NackFormat g = f;
        g.first_block_id = 0;
        o.put32(0, nack_header_word(REPAIR_ITEMS, REPAIR_INFO, f.item_len));
        o.put_item(4, g, 0, 0, 0);
        o.off = 4u + f.item_len, o.requests = 1;
    }
    block_start[2 * (size_t)nblocks] = o.off;
    block_start[2 * (size_t)nblocks + 1] = o.requests;
    totals[0] = o.off, totals[1] = o.requests, totals[2] = needing, totals[3] = absent;
}

}  // namespace

extern "C" int nfec_rx_repair_requests_host(uint32_t k, uint32_t m, const uint32_t* received, uint32_t mask_stride,
                                            const uint16_t* num_data, uint32_t nblocks, uint8_t fec_id, uint8_t fec_m,
                                            uint16_t object_id, uint32_t first_block_id, uint32_t flags,
                                            uint32_t max_units, void* content, uint64_t capacity, uint64_t* block_start,
                                            uint64_t* totals)
{
    if (k == 0 || m == 0 || (uint64_t)k + m > 65536) return fail(NFEC_EINVAL, "repair_requests_host: bad k or m");
    NackFormat f;
    int rc = nack_format(fec_id, fec_m, object_id, first_block_id, flags, max_units, &f);
    if (rc) return rc;
    if ((uint64_t)mask_stride * 32u < (uint64_t)k + m)
        return fail(NFEC_EINVAL, "repair_requests_host: mask_stride smaller than (k + m + 31) / 32");
    if (!block_start || !totals) return fail(NFEC_EINVAL, "repair_requests_host: null block_start or totals");
    if (capacity && !content) return fail(NFEC_EINVAL, "repair_requests_host: null content");
    if (nblocks && !received) return fail(NFEC_EINVAL, "repair_requests_host: null received mask");
    auto block = [&](uint32_t b) { return received + (size_t)b * mask_stride; };
    nack_walk_host([&](uint32_t b, uint32_t nd, NackCut* cut) { return nack_block_class_host(block(b), nd, k, m, cut); },
                   [&](uint32_t b) {
                       const uint32_t* mask = block(b);
                       return [mask](uint32_t w) { return mask[w]; };
                   },
                   k, num_data, nblocks, f, content, capacity, block_start, totals);
    return NFEC_OK;
}

// The repair-request content of a NORM_CMD(REPAIR_ADV) from the sender's repair state
// (suppress_layout.hpp: adv_class, adv_cut, adv_source_word).
extern "C" int nfec_tx_repair_adv_host(uint32_t k, uint32_t m, const nfec_tx_repair_state* state, uint32_t mask_stride,
                                       const uint16_t* num_data, uint32_t nblocks, uint8_t fec_id, uint8_t fec_m,
                                       uint16_t object_id, uint32_t first_block_id, uint32_t max_units, void* content,
                                       uint64_t capacity, uint64_t* block_start, uint64_t* totals)
{
    if (k == 0 || m == 0 || (uint64_t)k + m > 65536) return fail(NFEC_EINVAL, "tx_repair_adv_host: bad k or m");
    NackFormat f;
    int rc = nack_format(fec_id, fec_m, object_id, first_block_id, 0, max_units, &f);
    if (rc) return rc;
    if ((uint64_t)mask_stride * 32u < (uint64_t)k + m)
        return fail(NFEC_EINVAL, "tx_repair_adv_host: mask_stride smaller than (k + m + 31) / 32");
    if (!block_start || !totals) return fail(NFEC_EINVAL, "tx_repair_adv_host: null block_start or totals");
    if (capacity && !content) return fail(NFEC_EINVAL, "tx_repair_adv_host: null content");
    if (!state || (nblocks && (!state->repair || !state->block_repair || !state->object)))
        return fail(NFEC_EINVAL, "tx_repair_adv_host: null state");
    const uint32_t object_word = nblocks ? *state->object : 0u;
    f.info = adv_info(object_word);
    if (adv_whole_object(object_word)) {  // one OBJECT request and nothing of the blocks (normSession.cpp:4681)
        for (uint32_t b = 0; b < nblocks; ++b) block_start[2 * (size_t)b] = 0, block_start[2 * (size_t)b + 1] = NACK_SILENT;
        NackWriter o;
        o.content = static_cast<uint8_t*>(content), o.capacity = capacity;
        NackFormat g = f;
        g.first_block_id = 0;
        o.put32(0, nack_header_word(REPAIR_ITEMS, REPAIR_OBJECT, f.item_len));
        o.put_item(4, g, 0, 0, k);
        block_start[2 * (size_t)nblocks] = totals[0] = 4u + f.item_len;
        block_start[2 * (size_t)nblocks + 1] = totals[1] = 1;
        totals[2] = totals[3] = 0;
        return NFEC_OK;
    }
    auto block = [&](uint32_t b) { return state->repair + (size_t)b * mask_stride; };
    nack_walk_host(
        [&](uint32_t b, uint32_t nd, NackCut* cut) {
            if (nd < 1 || nd > k) return (uint32_t)NACK_SILENT;
            uint32_t any = 0;
            for (uint32_t w = 0; w < (nd + m + 31u) / 32u; ++w) any |= block(b)[w] & nack_range_bits(w, 0u, nd + m);
            *cut = adv_cut(nd, m);
            return adv_class(nd, k, (state->block_repair[b >> 5] >> (b & 31u)) & 1u, any);
        },
        [&](uint32_t b) {
            const uint32_t* mask = block(b);
            return [mask](uint32_t w) { return adv_source_word(mask[w]); };
        },
        k, num_data, nblocks, f, content, capacity, block_start, totals);
    return NFEC_OK;
}

extern "C" int nfec_repair_parse_host(uint8_t fec_id, uint8_t fec_m, const void* content, uint64_t bytes,
                                      uint8_t* unit_flags, uint8_t* unit_form, uint32_t* first, uint32_t* last,
                                      uint32_t capacity, uint64_t* consumed)
{
    const uint32_t kind = payload_id_kind(fec_id, fec_m);
    if (kind == PAYLOAD_ID_NONE) return fail(NFEC_EINVAL, "repair_parse_host: bad fec_id / fec_m");
    if (bytes && !content) return fail(NFEC_EINVAL, "repair_parse_host: null content");
    static_assert(sizeof(NackItem) == 4 * sizeof(uint32_t), "an item is four uint32");
    const uint64_t units = nack_parse(fec_id, kind, static_cast<const uint8_t*>(content), bytes, unit_flags, unit_form,
                                      reinterpret_cast<NackItem*>(first), reinterpret_cast<NackItem*>(last), capacity, consumed);
    if (units > 0x7fffffffu) return fail(NFEC_ERANGE, "repair_parse_host: more than 2^31 - 1 units");
    return (int)units;
}

// the scans' operator (nack_layout.hpp), for the host test of its associativity
extern "C" void nfec_nack_scan_combine_host(const uint64_t a[2], const uint64_t b[2], uint64_t out[2])
{
    const SegVal r = seg_combine(SegVal{a[0], (uint32_t)a[1]}, SegVal{b[0], (uint32_t)b[1]});
    out[0] = r.v, out[1] = r.f;
}
