// kernels_txrepair.hip -- sender repair state on the device (nfec.h, "sender repair state on the
// device"): the NACKs of a repair cycle into the repair state, its activation into the pending
// masks and the end-of-block step, by the rule of repair_layout.hpp (NormSession::
// SenderHandleNackMessage, !holdoff, reference src/common/normSession.cpp:3706-4300;
// NormBlock::HandleSegmentRequest and TxReset, src/common/normSegment.cpp:341-402, :219-259;
// NormObject::ActivateRepairs, src/common/normObject.cpp:472-537).
//
// Handling has two dependences: inside a message the walk is sequential over the request headers
// and carries the stretch's erasure count, and across messages a block's units must meet its state
// in message order.  Two kernels take one each.
// walk:   one wave per message.  The wave steps from request to request; its lanes take a
//         request's units, 64 a round.  Two segmented scans over the wave, carried between rounds
//         and requests, give every SEGMENT-level unit the last mark in front of it (does it open a
//         stretch?) and its erasure count.  Every such unit that can be applied is left as a record
//         {key, first, last, E, opens a stretch} on its block's list; the key is the unit's place
//         in the order of the call.  A BLOCK-level unit leaves, per covered block, the smallest of
//         such keys: the moment the block's bit became set.  Nothing of the state is written.
// apply:  one wave per block.  It ranks its block's records by key (every lane counts the keys
//         below its own while the wave walks the list), takes them 64 at a time in that order, and
//         applies them one after the other: the parity pair in scalar registers, the lanes over
//         the mask words.  "The block's bit is set at that moment" is "it was set before the call,
//         or the smallest BLOCK-level key of the block is below mine".  When the call's units
//         exceed the capacity it applies nothing, which makes the call all or nothing.
// What the atomics of `walk` leave does not depend on the order in which they land: sums, an OR, a
// maximum, and lists whose order is not used.
//
// activate / end of block: one wave per block, lanes over the mask words; `finish` rewrites the
// object word and clears block_repair behind the blocks' reads of both.
#include "message_wave.hpp"
#include "repair_layout.hpp"
#include "repair_wave.hpp"

namespace nfec {

namespace {

// ---- the workspace of a handle call ----

struct NackWsHeader {
    uint32_t alloc;                // records taken so far (may pass the capacity)
    uint32_t object_bits;          // TXR_OBJECT | TXR_INFO, as the units asked
    unsigned long long ignored;    // units ignored, and SEGMENT-level units no state can make apply
    uint32_t reserved[12];
};
static_assert(sizeof(NackWsHeader) == 64, "the header is one 64-byte line");

struct alignas(16) UnitRecord {
    uint64_t key;                  // repair_key(message, index in the message)
    uint32_t span;                 // first symbol | last symbol << 16
    uint32_t E;
    uint32_t next;                 // the list: 1 + the next record's index, 0 at its end
    uint32_t opens;                // the unit opens a stretch
    uint32_t rank;                 // apply's: the number of the block's keys below this one
    uint32_t reserved;
};
static_assert(sizeof(UnitRecord) == 32, "a record is two 16-byte chunks");

struct NackWs {
    NackWsHeader* header;
    unsigned long long* inv_min;   // [nblocks]: ~(the smallest BLOCK-level key), 0 = none
    uint32_t* head;                // [nblocks]: 1 + the index of the list's first record, 0 = empty
    UnitRecord* records;           // [unit_capacity]
};
__host__ __device__ inline uint64_t ws_head_offset(uint32_t nblocks) { return sizeof(NackWsHeader) + 8ull * nblocks; }
__host__ __device__ inline uint64_t ws_records_offset(uint32_t nblocks)
{
    return ws_head_offset(nblocks) + 4ull * (((uint64_t)nblocks + 3u) & ~3ull);
}
__device__ __forceinline__ NackWs ws_view(const TxNackArgs& a)
{
    NackWs w;
    w.header = reinterpret_cast<NackWsHeader*>(a.workspace);
    w.inv_min = reinterpret_cast<unsigned long long*>(a.workspace + sizeof(NackWsHeader));
    w.head = reinterpret_cast<uint32_t*>(a.workspace + ws_head_offset(a.nblocks));
    w.records = reinterpret_cast<UnitRecord*>(a.workspace + ws_records_offset(a.nblocks));
    return w;
}

__device__ __forceinline__ SegVal seg_up(SegVal x, uint32_t d) { return SegVal{lane_up(x.v, d), lane_up(x.f, d)}; }
__device__ __forceinline__ SegVal wave_seg_scan(SegVal x, uint32_t lane)
{
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const SegVal up = seg_up(x, d);
        if (lane >= d) x = seg_combine(up, x);
    }
    return x;
}
// the state in front of this lane's element: `carry` is the state in front of lane 0
__device__ __forceinline__ SegVal seg_before(SegVal inc, SegVal carry, uint32_t lane)
{
    SegVal up = seg_up(inc, 1);
    if (lane == 0) up = SegVal{0, 0};
    return seg_combine(carry, up);
}
__device__ __forceinline__ SegVal seg_behind(SegVal inc, SegVal carry)
{
    const SegVal last = {(uint64_t)__shfl((unsigned long long)inc.v, 63, 64), (uint32_t)__shfl(inc.f, 63, 64)};
    return seg_combine(carry, last);
}

// ---- walk: one wave per message ----

__global__ __launch_bounds__(256) void tx_nack_walk_kernel(TxNackArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = uniform(blockIdx.x * 4u + (threadIdx.x >> 6));
    const uint32_t nwaves = gridDim.x * 4u;
    const uint64_t count = message_count(a.count, a.count_dev);
    const uint32_t L = nack_item_length(a.id_kind);
    const NackWs ws = ws_view(a);
    uint64_t n_units = 0, n_ignored = 0;
    uint32_t n_cut = 0, n_unreadable = 0, object_bits = 0;
    for (uint64_t i = wave; i < count; i += nwaves) {
        const uint64_t off = uniform64(a.offsets[i]);
        const uint32_t len = uniform(a.length[i]);
        if (!rx_readable(off, len, 0u, a.payload_bytes)) {
            ++n_unreadable;
            continue;
        }
        const uint8_t* __restrict__ msg = a.payloads + off;
        uint32_t at = 0, index = 0;
        SegVal c_mark = {kMarkBreak, 1}, c_E = {0, 0};
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
                const bool have = u < nunits;
                WireItem first = {0, 0, 0, 0}, last = {0, 0, 0, 0};
                bool bad = false;
                if (have) {
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
                const uint32_t b0 = first.block;
                uint32_t nd = 0;
                if (own && level == LEVEL_SEGMENT && b0 < a.nblocks) nd = a.num_data ? a.num_data[b0] : a.k;
                UnitMark mk = {MARK_TRANSPARENT, 0u};
                if (valid) mk = repair_mark(level, own, b0, a.nblocks, nd, a.k, first.symbol, last.symbol);
                const bool is_seg = mk.kind == MARK_SEGMENT;

                // the last mark in front of each unit: does it open a stretch?
                const SegVal x = mk.kind == MARK_TRANSPARENT ? SegVal{0, 0} : SegVal{repair_mark_word(mk), 1};
                const SegVal inc_mark = wave_seg_scan(x, lane);
                const uint32_t mark0 = (uint32_t)seg_before(inc_mark, c_mark, lane).v;
                c_mark = seg_behind(inc_mark, c_mark);
                const bool opens = is_seg && repair_opens_stretch(mark0, b0);
                // the widths of the stretch so far
                const SegVal y = {is_seg ? (uint64_t)(last.symbol - first.symbol + 1u) : 0u, opens};
                const SegVal inc_E = wave_seg_scan(y, lane);
                const uint32_t E = a.extra_parity + (uint32_t)seg_combine(c_E, inc_E).v;
                c_E = seg_behind(inc_E, c_E);

                n_units += nvalid;
                const bool ignored = valid && (level == LEVEL_NONE || !own || (level == LEVEL_SEGMENT && !is_seg));
                n_ignored += (uint32_t)__popcll((unsigned long long)__ballot(ignored));
                if (__any(own && (flags & REPAIR_INFO))) object_bits |= TXR_INFO;
                if (__any(own && level == LEVEL_OBJECT)) object_bits |= TXR_OBJECT;

                // BLOCK level: the wave strides over each unit's blocks
                const uint32_t b1 = last.block;
                uint64_t todo = __ballot(own && level == LEVEL_BLOCK && b0 <= b1 && b0 < a.nblocks);
                while (todo) {
                    const uint32_t j = (uint32_t)__ffsll((unsigned long long)todo) - 1u;
                    todo &= todo - 1u;
                    const uint32_t lo = uniform(__shfl(b0, j, 64)), hi = min(uniform(__shfl(b1, j, 64)), a.nblocks - 1u);
                    const unsigned long long inv = ~(unsigned long long)repair_key(i, index + j);
                    for (uint64_t b = (uint64_t)lo + lane; b <= hi; b += 64) atomicMax(ws.inv_min + b, inv);
                }

                // SEGMENT level: one record per unit, the wave's records allocated by one add
                const uint64_t segs = __ballot(is_seg);
                if (segs) {
                    uint32_t base = 0;
                    if (lane == 0) base = atomicAdd(&ws.header->alloc, (uint32_t)__popcll((unsigned long long)segs));
                    base = __builtin_amdgcn_readfirstlane(base);
                    const uint32_t slot = base + (uint32_t)__popcll((unsigned long long)(segs & ((1ull << lane) - 1ull)));
                    // (an alloc that wrapped has passed the capacity: apply looks at no list then)
                    if (is_seg && slot >= base && slot < a.unit_capacity) {
                        UnitRecord r;
                        r.key = repair_key(i, index + lane);
                        r.span = first.symbol | (last.symbol << 16);
                        r.E = E;
                        r.opens = opens;
                        r.rank = 0, r.reserved = 0;
                        r.next = atomicExch(ws.head + b0, slot + 1u);
                        ws.records[slot] = r;
                    }
                }

                index += nvalid;
                if (badmask) {
                    at += 4u + (u0 + nvalid) * step * L;
                    stopped = true;
                    break;
                }
            }
            if (!stopped) at += 4u + rlen;
        }
        n_cut += at != len;
    }
    if (lane == 0) {
        add64(a.totals + 0, n_units);
        add64(a.totals + 4, n_cut);
        add64(a.totals + 5, n_unreadable);
        if (n_ignored) atomicAdd(&ws.header->ignored, (unsigned long long)n_ignored);
        if (object_bits) atomicOr(&ws.header->object_bits, object_bits);
    }
}

// ---- apply: one wave per block, the waves striding over the blocks ----

// counts: SEGMENT units applied, dropped, block bits newly set
__device__ __forceinline__ void apply_block(const TxNackArgs& a, const NackWs& ws, uint32_t b, uint32_t lane, uint64_t (&counts)[3])
{
    if (b == 0 && lane == 0) {
        const uint32_t bits = ws.header->object_bits;
        if (bits) *a.state.object |= bits;
        add64(a.totals + 2, ws.header->ignored);
    }
    const uint64_t inv = uniform64(ws.inv_min[b]);
    const uint64_t min_block_key = ~inv;  // (no BLOCK-level unit: above every key)
    const uint32_t head = uniform(ws.head[b]);
    const bool was_set = (uniform(a.state.block_repair[b >> 5]) >> (b & 31u)) & 1u;
    uint32_t applied = 0, dropped = 0;
    if (head) {
        const UnitRecord* recs = ws.records;
        const uint32_t nd = a.num_data ? uniform(a.num_data[b]) : a.k;  // (walk has checked it: inside [1, k])
        const uint32_t words = (nd + a.m + 31u) >> 5;
        uint32_t* __restrict__ mask = a.state.repair + (uint64_t)b * a.mask_stride;
        ParityPair pair = {uniform(a.state.parity[2 * (uint64_t)b]), uniform(a.state.parity[2 * (uint64_t)b + 1])};
        uint32_t n = 0;
        for (uint32_t cur = head; cur && n < a.unit_capacity; cur = uniform(recs[cur - 1u].next)) ++n;

        // ranks: the records 64 at a time in list order, each lane counting the keys below its own
        // over a walk of the whole list.  A list of up to 64 keeps its records in the lanes.
        UnitRecord mine = {};
        bool have = false;
        uint32_t cur = head;
        for (uint32_t c0 = 0; c0 < n; c0 += 64) {
            have = false;
            uint32_t at = 0;
            for (uint32_t j = 0; j < 64u && cur; ++j) {
                const UnitRecord r = recs[cur - 1u];
                if (lane == j) mine = r, have = true, at = cur;
                cur = uniform(r.next);
            }
            uint32_t rank = 0, left = n;
            for (uint32_t w = head; w && left; --left) {
                const uint64_t key = uniform64(recs[w - 1u].key);
                rank += key < mine.key;
                w = uniform(recs[w - 1u].next);
            }
            mine.rank = rank;
            if (n > 64u && have) ws.records[at - 1u].rank = rank;
        }

        if (n > 64u) __threadfence_block();  // the ranks are read back by other lanes of the wave
        bool prev_applied = false;
        for (uint32_t t0 = 0; t0 < n; t0 += 64) {
            if (n > 64u) {  // the records of ranks [t0, t0 + 64) into the lanes
                have = false;
                uint32_t left = n;
                for (uint32_t w = head; w && left; --left) {
                    const UnitRecord r = ws.records[w - 1u];
                    if (r.rank >= t0 && r.rank - t0 == lane) mine = r, have = true;
                    w = uniform(r.next);
                }
            }
            const uint32_t cnt = min(64u, n - t0);
            for (uint32_t j = 0; j < cnt; ++j) {
                const uint64_t owner = __ballot(have && mine.rank == t0 + j);
                if (!owner) continue;  // (keys are distinct: every rank has an owner)
                const int src = __ffsll((unsigned long long)owner) - 1;
                const uint64_t key = uniform64(__shfl((unsigned long long)mine.key, src, 64));
                const uint32_t span = uniform(__shfl(mine.span, src, 64)), E = uniform(__shfl(mine.E, src, 64));
                const bool opens = uniform(__shfl(mine.opens, src, 64)) != 0u;
                // a unit that opens a stretch meets the block's bit; one that continues a stretch
                // shares the fate of the unit in front of it (the bit is never cleared here)
                const bool ok = opens ? !(was_set || min_block_key < key) : prev_applied;
                if (ok) {
                    const RepairSlots slots = repair_segment_request(pair, span & 0xffffu, span >> 16, nd, a.m, E);
                    for (uint32_t w = lane; w < words; w += 64) {
                        const uint32_t bits = repair_slot_bits(w, slots);
                        if (bits) mask[w] |= bits;
                    }
                    ++applied;
                } else {
                    ++dropped;
                }
                prev_applied = ok;
            }
        }
        if (lane == 0 && applied) {
            a.state.parity[2 * (uint64_t)b] = (uint16_t)pair.offset;
            a.state.parity[2 * (uint64_t)b + 1] = (uint16_t)pair.count;
        }
    }
    const bool newly = inv != 0 && !was_set;
    if (newly && lane == 0) atomicOr(a.state.block_repair + (b >> 5), 1u << (b & 31u));
    counts[0] += applied, counts[1] += dropped, counts[2] += newly;
}

__global__ __launch_bounds__(256) void tx_nack_apply_kernel(TxNackArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = uniform(blockIdx.x * 4u + (threadIdx.x >> 6));
    const uint32_t nwaves = gridDim.x * 4u;
    if (uniform64(a.totals[0]) > a.unit_capacity) return;  // all or nothing (every wave of the grid alike)
    const NackWs ws = ws_view(a);
    uint64_t counts[3] = {0, 0, 0};
    for (uint64_t b = wave; b < a.nblocks; b += nwaves) apply_block(a, ws, (uint32_t)b, lane, counts);
    group_add<3>(a.totals + 1, counts, lane);
}

// ---- activation and end of block: one wave per block ----

// counts: blocks reset with a change, blocks whose segment repairs were activated, pending bits
__device__ __forceinline__ void activate_block(const TxActivateArgs& a, uint32_t b, uint32_t lane, uint64_t (&counts)[3])
{
    const uint32_t nd = a.num_data ? uniform(a.num_data[b]) : a.k;
    if (nd < 1 || nd > a.k) return;
    const uint32_t words = (nd + a.m + 31u) >> 5;
    uint32_t* __restrict__ pend = a.pending + (uint64_t)b * a.mask_stride;
    uint32_t* __restrict__ rep = a.state.repair + (uint64_t)b * a.mask_stride;
    const uint32_t object_word = uniform(*a.state.object);
    const bool bit = (uniform(a.state.block_repair[b >> 5]) >> (b & 31u)) & 1u;
    const bool resets = repair_block_resets(object_word, bit), activates = repair_block_activates(object_word);
    bool differs = false;
    if (resets) {
        for (uint32_t w = lane; w < words; w += 64) differs |= repair_reset_differs(pend[w], w, nd, a.m, a.auto_parity);
        differs = __any(differs);
    }
    bool activated = false;
    uint32_t bits_after = 0;
    for (uint32_t w = lane; w < words; w += 64) {
        const uint32_t p0 = pend[w], r0 = rep[w], valid = repair_valid_bits(w, nd, a.m);
        uint32_t p = p0, r = r0;
        if (resets) {
            if (differs) p = repair_reset_word(p, w, nd, a.m, a.auto_parity);
            r &= ~valid;
        }
        if (activates) {
            const uint32_t bits = r & valid;
            activated |= bits != 0u;
            p |= bits, r &= ~bits;
        }
        if (p != p0) pend[w] = p;
        if (r != r0) rep[w] = r;
        bits_after += __popc(p & valid);
    }
    bits_after = __shfl(wave_scan(bits_after, lane), 63, 64);
    activated = __any(activated);
    if (lane == 0 && differs) {
        a.state.parity[2 * (uint64_t)b] = (uint16_t)a.auto_parity;
        a.state.parity[2 * (uint64_t)b + 1] = (uint16_t)a.m;
    }
    counts[0] += differs, counts[1] += activated, counts[2] += uniform(bits_after);
}

__global__ __launch_bounds__(256) void tx_activate_kernel(TxActivateArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = uniform(blockIdx.x * 4u + (threadIdx.x >> 6));
    const uint32_t nwaves = gridDim.x * 4u;
    uint64_t counts[3] = {0, 0, 0};
    for (uint64_t b = wave; b < a.nblocks; b += nwaves) activate_block(a, (uint32_t)b, lane, counts);
    group_add<3>(a.totals, counts, lane);
}

// behind the blocks' reads of both: the object word, and block_repair cleared
__global__ __launch_bounds__(256) void tx_activate_finish_kernel(TxActivateArgs a)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t == 0) *a.state.object = repair_object_after(*a.state.object, a.totals[0]);
    if (t < (a.nblocks + 31u) / 32u) a.state.block_repair[t] = 0u;
}

__global__ __launch_bounds__(256) void tx_end_blocks_kernel(TxActivateArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t b = uniform(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (b >= a.nblocks) return;
    const uint32_t nd = a.num_data ? uniform(a.num_data[b]) : a.k;
    if (nd < 1 || nd > a.k) return;
    const uint32_t words = (nd + a.m + 31u) >> 5;
    const uint32_t* __restrict__ pend = a.pending + (uint64_t)b * a.mask_stride;
    uint32_t any = 0;
    for (uint32_t w = lane; w < words; w += 64) any |= pend[w] & repair_valid_bits(w, nd, a.m);
    if (__any(any != 0u) || lane) return;
    uint16_t* pair = a.state.parity + 2 * (uint64_t)b;
    const ParityPair p = repair_end_block(ParityPair{pair[0], pair[1]}, a.m);
    pair[0] = (uint16_t)p.offset, pair[1] = (uint16_t)p.count;
}

constexpr uint32_t kMaxGroups = 8192;  // (kernels_rx.hip: enough waves to fill the chip many times over)
// the per-block kernels that count: about what the chip holds at once, so the counters cost a few
// thousand atomics whatever the batch
constexpr uint32_t kBlockGroups = 2048;

}  // namespace

uint64_t tx_nack_workspace_bytes(uint32_t unit_capacity, uint32_t nblocks)
{
    return ws_records_offset(nblocks) + (uint64_t)sizeof(UnitRecord) * unit_capacity;
}

// (the ABI entries have checked the arguments)
int launch_tx_handle_nacks(const TxNackArgs& a, hipStream_t s)
{
    NFEC_HIP(hipMemsetAsync(a.totals, 0, 6 * sizeof(uint64_t), s));
    if (a.count == 0 || a.nblocks == 0) return NFEC_OK;
    NFEC_HIP(hipMemsetAsync(a.workspace, 0, ws_records_offset(a.nblocks), s));
    const uint32_t grid = (uint32_t)std::min<uint64_t>(((uint64_t)a.count + 3u) / 4u, kMaxGroups);
    hipLaunchKernelGGL(tx_nack_walk_kernel, dim3(grid), dim3(256), 0, s, a);
    const uint32_t groups = (uint32_t)std::min<uint64_t>(((uint64_t)a.nblocks + 3u) / 4u, kBlockGroups);
    hipLaunchKernelGGL(tx_nack_apply_kernel, dim3(groups), dim3(256), 0, s, a);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? NFEC_OK : hip_fail(e, "tx_handle_nacks launch");
}

int launch_tx_activate_repairs(const TxActivateArgs& a, hipStream_t s)
{
    NFEC_HIP(hipMemsetAsync(a.totals, 0, 3 * sizeof(uint64_t), s));
    if (a.nblocks == 0) return NFEC_OK;
    const uint32_t groups = (uint32_t)std::min<uint64_t>(((uint64_t)a.nblocks + 3u) / 4u, kBlockGroups);
    hipLaunchKernelGGL(tx_activate_kernel, dim3(groups), dim3(256), 0, s, a);
    const uint32_t words = (uint32_t)(((uint64_t)a.nblocks + 31u) / 32u);
    hipLaunchKernelGGL(tx_activate_finish_kernel, dim3((words + 255u) / 256u), dim3(256), 0, s, a);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? NFEC_OK : hip_fail(e, "tx_activate_repairs launch");
}

int launch_tx_end_blocks(const TxActivateArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(tx_end_blocks_kernel, dim3((uint32_t)(((uint64_t)a.nblocks + 3u) / 4u)), dim3(256), 0, s, a);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? NFEC_OK : hip_fail(e, "tx_end_blocks launch");
}

}  // namespace nfec
