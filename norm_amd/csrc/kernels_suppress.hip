// kernels_suppress.hip -- NACK suppression on the device (nfec.h, "NACK suppression and repair
// advertisements on the device"): overheard repair-request content into the receiver's suppression
// state, and the decision at the end of the back-off, by the rule of suppress_layout.hpp
// (NormSenderNode::HandleRepairContent, reference src/common/normNode.cpp:1069-1187;
// NormObject::IsRepairPending, src/common/normObject.cpp:1137-1177; NormBlock::IsRepairPending,
// src/common/normSegment.cpp:174-216).  (The advertisement is the repair-request walk over another
// mask: kernels_nack.hip.)
//
// handle:  one wave per message, stepping from request to request; its lanes take a request's
//          units, 64 a round (the loads and the walk of tx_nack_walk_kernel).  Every update is an
//          OR, so nothing is ordered and nothing is kept between the units: a BLOCK-level unit has
//          the wave stride over the words of its range, a SEGMENT-level unit ORs its bits into its
//          block's repair words once the block's class is known.  The class comes from one pass
//          over the block's reception words, made once for all units of a round that name the
//          block and kept for the rounds behind it.
// pending: one wave per word of pending_blocks, a block at a time with the lanes over its mask
//          words; the wave is the word's only writer.  A second launch of one thread turns the
//          counts into the decision.
// Counters go through LDS once per workgroup, at most kBlockGroups workgroups.
#include "message_wave.hpp"
#include "repair_wave.hpp"
#include "suppress_layout.hpp"

namespace nfec {

namespace {

// ---- handle: one wave per message ----

__global__ __launch_bounds__(256) void rx_repair_content_kernel(RxRepairContentArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = uniform(blockIdx.x * 4u + (threadIdx.x >> 6));
    const uint32_t nwaves = gridDim.x * 4u;
    const uint64_t count = message_count(a.count, a.count_dev);
    const uint32_t L = nack_item_length(a.id_kind);
    // units, SEGMENT units applied, units not applied or ignored, block bits newly set, cut short, unreadable
    uint64_t n[6] = {0, 0, 0, 0, 0, 0};
    uint32_t newly = 0, object_bits = 0;
    uint32_t known_block = 0xffffffffu, known_class = NACK_SILENT;  // the block whose class the wave holds
    for (uint64_t i = wave; i < count; i += nwaves) {
        const uint64_t off = uniform64(a.offsets[i]);
        const uint32_t len = uniform(a.length[i]);
        if (!rx_readable(off, len, 0u, a.payload_bytes)) {
            ++n[5];
            continue;
        }
        const uint8_t* __restrict__ msg = a.payloads + off;
        uint32_t at = 0;
        bool stopped = false;
        while (!stopped && len - at >= 4u) {
            // the request header (NormRepairRequest::Unpack): every lane reads the same dword
            const uint32_t hdr = uniform(load32(msg + at));
            const uint32_t form = hdr & 0xffu, flags = (hdr >> 8) & 0xffu, rlen = bswap16(hdr >> 16);
            if (rlen > len - at - 4u) break;
            const uint32_t items = rlen / L, step = form == REPAIR_RANGES ? 2u : 1u;
            if (step == 2u && (items & 1u)) break;
            const uint32_t nunits = items / step, level = repair_level(flags);
            for (uint32_t u0 = 0; u0 < nunits; u0 += 64) {
                const uint32_t u = u0 + lane;
                WireItem first = {0, 0, 0, 0}, last = {0, 0, 0, 0};
                bool bad = false;
                if (u < nunits) {
                    const uint8_t* __restrict__ p = msg + at + 4u + u * step * L;  // (inside the request's rlen bytes)
                    first = load_item(a.id_kind, a.first_block_id, p, L);
                    last = step == 2u ? load_item(a.id_kind, a.first_block_id, p + L, L) : first;
                    bad = first.fec_id != a.fec_id || last.fec_id != a.fec_id;
                }
                // the walk ends at the first item with a foreign fec_id; the units in front of it stand
                const uint64_t badmask = __ballot(bad);
                const uint32_t nvalid = badmask ? (uint32_t)__ffsll((unsigned long long)badmask) - 1u : min(64u, nunits - u0);
                const bool valid = lane < nvalid;
                const bool own = valid && level != LEVEL_NONE && repair_own(level, a.object_id, first.object_id, last.object_id);
                n[0] += nvalid;
                if (__any(own)) object_bits |= suppress_object_bits(level, flags);

                const uint32_t b0 = first.block;
                if (level == LEVEL_BLOCK) {
                    // the wave strides over the words of each unit's range: whole words in the
                    // middle, partial ones at the ends
                    uint32_t hi = 0;
                    const bool sets = own && suppress_block_range(b0, last.block, a.nblocks, &hi);
                    uint64_t todo = __ballot(sets);
                    while (todo) {
                        const uint32_t j = (uint32_t)__ffsll((unsigned long long)todo) - 1u;
                        todo &= todo - 1u;
                        const uint32_t lo_j = uniform(__shfl(b0, j, 64)), hi_j = uniform(__shfl(hi, j, 64));
                        for (uint64_t w = (uint64_t)(lo_j >> 5) + lane; w <= (hi_j >> 5); w += 64) {
                            const uint32_t bits = suppress_block_bits((uint32_t)w, lo_j, hi_j);
                            // (a word that holds the bits already is left alone; the count is the atomic's)
                            if (bits & ~a.state.block_repair[w]) newly += __popc(bits & ~atomicOr(a.state.block_repair + w, bits));
                        }
                    }
                } else if (level == LEVEL_SEGMENT) {
                    uint32_t nd = 0;
                    if (own && b0 < a.nblocks) nd = a.num_data ? a.num_data[b0] : a.k;
                    const UnitMark mk = repair_mark(level, own, b0, a.nblocks, nd, a.k, first.symbol, last.symbol);
                    const bool is_seg = valid && mk.kind == MARK_SEGMENT;
                    bool applied = false;
                    // the class of each block the round names, decided once
                    uint64_t todo = __ballot(is_seg);
                    while (todo) {
                        const uint32_t j = (uint32_t)__ffsll((unsigned long long)todo) - 1u;
                        const uint32_t b = uniform(__shfl(b0, j, 64));
                        if (b != known_block) {
                            const uint32_t nd_b = uniform(__shfl(nd, j, 64));
                            known_class = block_shape(a.k, a.m, a.received + (uint64_t)b * a.mask_stride, nd_b, lane).cls;
                            known_block = b;
                        }
                        const bool mine = is_seg && b0 == b;
                        todo &= ~__ballot(mine);
                        applied |= mine && suppress_block_held(known_class);
                    }
                    if (applied) {
                        uint32_t* __restrict__ mask = a.state.repair + (uint64_t)b0 * a.mask_stride;
                        const uint32_t w_end = (nd + a.m + 31u) >> 5;
                        for (uint32_t w = first.symbol >> 5; w <= (last.symbol >> 5) && w < w_end; ++w) {
                            const uint32_t bits = suppress_segment_bits(w, first.symbol, last.symbol, nd, a.m);
                            if (bits & ~mask[w]) atomicOr(mask + w, bits);
                        }
                    }
                    n[1] += (uint32_t)__popcll((unsigned long long)__ballot(applied));
                    n[2] += (uint32_t)__popcll((unsigned long long)__ballot(valid && own && !applied));
                }
                n[2] += (uint32_t)__popcll((unsigned long long)__ballot(valid && !own));

                if (badmask) {
                    at += 4u + (u0 + nvalid) * step * L;
                    stopped = true;
                    break;
                }
            }
            if (!stopped) at += 4u + rlen;
        }
        n[4] += at != len;
    }
    // the lanes' newly set bits into lane 0's count
    n[3] = __shfl(wave_scan(newly, lane), 63, 64);
    if (lane == 0 && (object_bits & ~*a.state.object)) atomicOr(a.state.object, object_bits);
    group_add<6>(a.totals, n, lane);
}

// ---- pending: one wave per word of pending_blocks ----

// is block b pending?  counts: blocks pending, needing blocks suppressed, absent blocks suppressed
__device__ __forceinline__ bool pending_block(const RxRepairPendingArgs& a, uint32_t b, bool bit, uint32_t lane, uint64_t (&counts)[3])
{
    const uint32_t nd = a.num_data ? uniform(a.num_data[b]) : a.k;
    const uint32_t* __restrict__ mask = a.received + (uint64_t)b * a.mask_stride;
    const uint32_t* __restrict__ rep = a.state.repair + (uint64_t)b * a.mask_stride;
    uint32_t word0 = 0;
    const BlockShape sh = block_shape(a.k, a.m, mask, nd, lane, &word0);
    bool residual = false;
    if (sh.cls == NACK_NEEDING && !bit) {
        // the words of the first round are still in the lanes: one pass for a block of up to 2,048 slots
        const uint32_t w_end = (nd + a.m + 31u) >> 5;
        uint32_t left = lane < w_end ? suppress_residual_word(word0, rep[lane], lane, sh.cut) : 0u;
        for (uint32_t w = 64u + lane; w < w_end; w += 64) left |= suppress_residual_word(mask[w], rep[w], w, sh.cut);
        residual = __any(left != 0u);
    }
    const bool pending = suppress_block_pending(sh.cls, bit, residual);
    counts[0] += pending;
    counts[1] += !pending && sh.cls == NACK_NEEDING;
    counts[2] += !pending && sh.cls == NACK_ABSENT;
    return pending;
}

__global__ __launch_bounds__(256) void rx_repair_pending_kernel(RxRepairPendingArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = uniform(blockIdx.x * 4u + (threadIdx.x >> 6));
    const uint32_t nwaves = gridDim.x * 4u;
    const uint32_t words = (uint32_t)(((uint64_t)a.nblocks + 31u) >> 5);
    uint64_t counts[3] = {0, 0, 0};
    for (uint32_t w = wave; w < words; w += nwaves) {
        const uint32_t bits = uniform(a.state.block_repair[w]);
        const uint32_t b_end = min(32u, a.nblocks - (w << 5));
        uint32_t out = 0;
        for (uint32_t j = 0; j < b_end; ++j)
            if (pending_block(a, (w << 5) + j, (bits >> j) & 1u, lane, counts)) out |= 1u << j;
        if (a.pending_blocks && lane == 0) a.pending_blocks[w] = out;
    }
    group_add<3>(a.totals + 1, counts, lane);
}

// behind the blocks' counts: the decision
__global__ void rx_repair_pending_finish_kernel(RxRepairPendingArgs a)
{
    if (threadIdx.x == 0) a.totals[0] = suppress_sends(*a.state.object, a.info_pending != 0u, a.totals[1]);
}

constexpr uint32_t kMaxGroups = 2048;  // the kernels that count: about what the chip holds at once

}  // namespace

// (the ABI entries have checked the arguments)
int launch_rx_repair_content(const RxRepairContentArgs& a, hipStream_t s)
{
    NFEC_HIP(hipMemsetAsync(a.totals, 0, 6 * sizeof(uint64_t), s));
    if (a.count == 0 || a.nblocks == 0) return NFEC_OK;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(((uint64_t)a.count + 3u) / 4u, kMaxGroups);
    hipLaunchKernelGGL(rx_repair_content_kernel, dim3(grid), dim3(256), 0, s, a);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? NFEC_OK : hip_fail(e, "rx_handle_repair_content launch");
}

int launch_rx_repair_pending(const RxRepairPendingArgs& a, hipStream_t s)
{
    NFEC_HIP(hipMemsetAsync(a.totals, 0, 4 * sizeof(uint64_t), s));
    if (a.nblocks == 0) return NFEC_OK;
    const uint64_t words = ((uint64_t)a.nblocks + 31u) / 32u;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((words + 3u) / 4u, kMaxGroups);
    hipLaunchKernelGGL(rx_repair_pending_kernel, dim3(grid), dim3(256), 0, s, a);
    hipLaunchKernelGGL(rx_repair_pending_finish_kernel, dim3(1), dim3(64), 0, s, a);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? NFEC_OK : hip_fail(e, "rx_repair_pending launch");
}

}  // namespace nfec
