// kernels_nack.hip -- repair requests on the device (nfec.h, "repair requests on the device"): the
// repair-request content of a NORM_NACK from the reception masks in HBM, by the rule of
// nack_layout.hpp (NormObject::AppendRepairRequest, reference src/common/normObject.cpp:1179-1381,
// and NormBlock::AppendRepairRequest, src/common/normSegment.cpp:524-630).
//
// count:  one wave per block, lanes over the mask words: the block's class and, for a needing
//         block, the bytes and requests of its own chain.
// scan:   one workgroup over the blocks in tiles with running carries: the byte offsets, and the
//         chains of block-level units (runs of absent blocks) as segmented scans.
// expand: one wave per block: a needing block's wave writes its requests, the wave of the block
//         that ends a run of absent blocks writes the run's unit.
//
// No unit looks ahead: a request's header is written by whoever closes it -- the unit that opens
// the next request, the needing block that ends the chain, or the end of the walk -- because the
// closed request's items are the bytes right in front of the closer.
//
// ADV: the same three kernels over the sender's repair state give the repair-request content of a
// NORM_CMD(REPAIR_ADV) (NormObject::AppendRepairAdv, normObject.cpp:540-683, the same walk): a
// block's class and request words come from its block_repair bit and its repair mask
// (suppress_layout.hpp), INFO from the object word, and an object that is repaired as a whole is
// one OBJECT request written where the walk ends.
#include "nack_layout.hpp"
#include "nfec_internal.hpp"
#include "repair_wave.hpp"
#include "suppress_layout.hpp"
#include "wave.hpp"

namespace nfec {

namespace {

// ---- bytes ----

// (content is 4-byte aligned and every offset a multiple of 4; a capacity that is not cuts a dword)
__device__ __forceinline__ void put32(const NackArgs& a, uint64_t at, uint32_t word)
{
    if (at < a.capacity && at + 4u <= a.capacity) {  // (an offset that wrapped writes nothing)
        *reinterpret_cast<uint32_t*>(a.content + at) = word;
    } else {
        for (uint32_t j = 0; j < 4; ++j)
            if (at + j < a.capacity) a.content[at + j] = (uint8_t)(word >> (8 * j));
    }
}

__device__ __forceinline__ void put_item(const NackArgs& a, uint64_t at, uint32_t b, uint32_t s, uint32_t nd)
{
    NackFormat f;
    f.fec_id = a.fec_id, f.object_id = a.object_id;
    const uint64_t id = payload_id(a.id_kind, a.first_block_id + b, s, nd);
    put32(a, at, nack_item_word(f));
    put32(a, at + 4, (uint32_t)id);
    if (a.item_len == 12) put32(a, at + 8, (uint32_t)(id >> 32));
}

// ---- segmented scans over a wave (nack_layout.hpp's operator) ----

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
// the state behind lane 63
__device__ __forceinline__ SegVal seg_behind(SegVal inc, SegVal carry)
{
    const SegVal last = {(uint64_t)__shfl((unsigned long long)inc.v, 63, 64), (uint32_t)__shfl(inc.f, 63, 64)};
    return seg_combine(carry, last);
}

// ---- one block ----

// The chain of a needing block.  Lane L of a round takes the runs that start in its word: from the
// word, the top bits of the one before and the low bits of the one behind it has the run starts and
// their three length classes as bit masks.  Three segmented scans over the wave, each seeded by
// the one before and carried between rounds, give every run its place in the chain: the form in
// front of it, the units since the form changed (so whether it opens a request) and the items in
// the open request; two sums give the requests and items in front of it, that is its byte offset.
// WRITE: the lane writes its runs' items and closes the requests its runs end; a long run's end
// item is written by the lane whose word holds the end, at the offset of the last unit in front
// of its own.  Serial work per lane: the run starts of its one word.
// ADV: mask is the block's repair mask, whose set bits are the requested slots.
template <bool WRITE, bool ADV>
__device__ __forceinline__ void block_requests(const NackArgs& a, uint32_t info, const uint32_t* __restrict__ mask, uint32_t b,
                                               uint32_t nd, NackCut cut, uint32_t lane, uint64_t base, uint32_t* out_reqs,
                                               uint32_t* out_items)
{
    const uint32_t L = a.item_len, M = a.max_units, flags = REPAIR_SEGMENT | info;
    const uint32_t w_first = cut.lo >> 5, w_last = (cut.hi + 31u) >> 5;  // the words with request bits
    SegVal c_form = {0, 0}, c_since = {0, 0}, c_open = {0, 0};
    uint32_t c_reqs = 0, c_items = 0;
    auto rword = [&](uint32_t w) {
        return w >= w_first && w < w_last ? nack_request_word(ADV ? adv_source_word(mask[w]) : mask[w], w, cut) : 0u;
    };
    for (uint32_t w0 = w_first; w0 < w_last; w0 += 64) {
        const uint32_t w = w0 + lane;
        const uint32_t R = rword(w), Rm = rword(w - 1u), Rp = rword(w + 1u);
        const uint64_t X = R | ((uint64_t)Rp << 32);
        const uint32_t cin = Rm >> 31;
        const uint32_t S = R & ~((R << 1) | cin);              // run starts
        const uint32_t two = S & (uint32_t)(X >> 1);           // ... of runs of 2 or more: two items
        const uint32_t lng = two & (uint32_t)(X >> 2);         // ... of runs of 3 or more: RANGES
        auto form_at = [&](uint32_t i) { return (lng >> i) & 1u ? (uint32_t)REPAIR_RANGES : (uint32_t)REPAIR_ITEMS; };
        auto items_at = [&](uint32_t i) { return (two >> i) & 1u ? 2u : 1u; };

        // the form in front of the lane's first run
        const SegVal inc_form = wave_seg_scan(SegVal{S ? form_at(31u - __clz(S)) : 0u, S != 0u}, lane);
        const uint32_t form0 = (uint32_t)seg_before(inc_form, c_form, lane).v;
        c_form = seg_behind(inc_form, c_form);

        // the units since the form changed, in front of the lane's first run
        SegVal mine = {0, 0};
        uint32_t pf = form0;
        for (uint32_t rest = S; rest; rest &= rest - 1u) {
            const uint32_t f = form_at(__ffs(rest) - 1u);
            mine = seg_combine(mine, SegVal{1, f != pf});
            pf = f;
        }
        const SegVal inc_since = wave_seg_scan(mine, lane);
        const uint32_t since0 = (uint32_t)seg_before(inc_since, c_since, lane).v;
        c_since = seg_behind(inc_since, c_since);

        // the requests the lane's runs open and their items
        mine = SegVal{0, 0};
        uint32_t nreq = 0, nit = 0, since = since0;
        pf = form0;
        for (uint32_t rest = S; rest; rest &= rest - 1u) {
            const uint32_t i = __ffs(rest) - 1u, f = form_at(i), it = items_at(i);
            since = f != pf ? 1u : since + 1u;
            const bool opens = nack_opens(since, M);
            mine = seg_combine(mine, SegVal{it, opens});
            nreq += opens, nit += it, pf = f;
        }
        const SegVal inc_open = wave_seg_scan(mine, lane);
        const uint32_t open0 = (uint32_t)seg_before(inc_open, c_open, lane).v;
        c_open = seg_behind(inc_open, c_open);
        const uint32_t inc_reqs = wave_scan(nreq, lane), inc_items = wave_scan(nit, lane);
        const uint32_t reqs0 = c_reqs + inc_reqs - nreq, items0 = c_items + inc_items - nit;
        c_reqs += __shfl(inc_reqs, 63, 64), c_items += __shfl(inc_items, 63, 64);

        if (WRITE) {
            // a run that came in from the word before and ends here: its end item, if it is long
            if (cin && (R & 1u)) {
                const uint64_t inv = ~X;
                const uint32_t ones = inv ? (uint32_t)__builtin_ctzll(inv) : 64u;
                if (ones <= 32u && (ones >= 2u || ((Rm >> 30) & 1u)))
                    put_item(a, base + 4ull * reqs0 + (uint64_t)L * (items0 - 1u), b, (w << 5) + ones - 1u, nd);
            }
            uint32_t open = open0, rq = reqs0, done = items0;
            since = since0, pf = form0;
            for (uint32_t rest = S; rest; rest &= rest - 1u) {
                const uint32_t i = __ffs(rest) - 1u, f = form_at(i), it = items_at(i), s = (w << 5) + i;
                since = f != pf ? 1u : since + 1u;
                if (nack_opens(since, M)) {
                    if (pf)
                        put32(a, base + 4ull * rq + (uint64_t)L * done - (uint64_t)L * open - 4u,
                              nack_header_word(pf, flags, L * open));
                    open = 0, ++rq;
                }
                const uint64_t at = base + 4ull * rq + (uint64_t)L * done;
                put_item(a, at, b, s, nd);
                if (it == 2) {
                    if (f == REPAIR_ITEMS) {
                        put_item(a, at + L, b, s + 1u, nd);
                    } else {
                        const uint64_t inv = ~(X >> i);
                        const uint32_t ones = inv ? (uint32_t)__builtin_ctzll(inv) : 64u;
                        if (ones <= 32u - i) put_item(a, at + L, b, s + ones - 1u, nd);  // the run ends in this word
                    }
                }
                open += it, done += it, pf = f;
            }
        }
    }
    // the chain's last request is closed by the block's end
    if (WRITE && c_form.v && lane == 0)
        put32(a, base + 4ull * c_reqs + (uint64_t)L * c_items - L * c_open.v - 4u,
              nack_header_word((uint32_t)c_form.v, flags, L * (uint32_t)c_open.v));
    *out_reqs = c_reqs, *out_items = c_items;
}

// Where a block's class, its cut and INFO come from.  A NACK: the reception mask and the call's
// flags.  ADV: the block_repair bit, the repair mask (a.received) and the object word; with the
// whole object under repair every block is silent and the scan writes the one OBJECT request.
template <bool ADV>
__device__ __forceinline__ uint32_t source_info(const NackArgs& a)
{
    return ADV ? adv_info(uniform(*a.object)) : a.info;
}
template <bool ADV>
__device__ __forceinline__ BlockShape source_shape(const NackArgs& a, const uint32_t* __restrict__ mask, uint32_t b, uint32_t nd,
                                                   uint32_t lane)
{
    if (!ADV) return block_shape(a.k, a.m, mask, nd, lane);
    BlockShape r = {NACK_SILENT, {0u, 0u}};
    if (nd < 1 || nd > a.k || adv_whole_object(uniform(*a.object))) return r;
    const uint32_t n = nd + a.m, w_end = (n + 31u) >> 5;
    uint32_t any = 0;
    for (uint32_t w = lane; w < w_end; w += 64) any |= mask[w] & nack_range_bits(w, 0, n);
    const bool bit = (uniform(a.block_repair[b >> 5]) >> (b & 31u)) & 1u;
    r.cls = adv_class(nd, a.k, bit, __any(any != 0u));
    r.cut = adv_cut(nd, a.m);
    return r;
}

// per block: block_start[b][1] = class | the requests of the block's own chain << 8 | its items << 28
// (a block has at most (k + m + 1) / 2 units of two items: both fit 20 bits)
template <bool ADV>
__global__ __launch_bounds__(256) void nack_count_kernel(NackArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t b = uniform(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (b >= a.nblocks) return;
    const uint32_t nd = a.num_data ? uniform(a.num_data[b]) : a.k;
    const uint32_t* mask = a.received + (uint64_t)b * a.mask_stride;
    const BlockShape sh = source_shape<ADV>(a, mask, b, nd, lane);
    uint32_t reqs = 0, items = 0;
    if (sh.cls == NACK_NEEDING) block_requests<false, ADV>(a, source_info<ADV>(a), mask, b, nd, sh.cut, lane, 0, &reqs, &items);
    if (lane == 0) a.rows[2 * (uint64_t)b + 1] = sh.cls | ((uint64_t)reqs << 8) | ((uint64_t)items << 28);
}

// ---- the scan over the blocks ----

constexpr uint32_t kNackScanThreads = 512;  // a tile: kNackScanItems consecutive blocks per thread
constexpr uint32_t kNackScanItems = 16;
constexpr uint32_t kNackScanWaves = kNackScanThreads / 64;
constexpr uint32_t kNackScanTile = kNackScanThreads * kNackScanItems;

// N segmented scans over the threads' totals behind one barrier: before = the state in front of
// the thread's first element, carry the state behind the tile.
template <int N>
__device__ __forceinline__ void tile_scan(const SegVal (&x)[N], SegVal (&carry)[N], SegVal (&before)[N],
                                          SegVal (*sums)[kNackScanWaves], uint32_t lane, uint32_t wv)
{
    SegVal inc[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        inc[j] = wave_seg_scan(x[j], lane);
        if (lane == 63) sums[j][wv] = inc[j];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < N; ++j) {
        SegVal base = carry[j], total = carry[j];
#pragma unroll
        for (uint32_t v = 0; v < kNackScanWaves; ++v) {
            const SegVal s = sums[j][v];
            if (v < wv) base = seg_combine(base, s);
            total = seg_combine(total, s);
        }
        before[j] = seg_before(inc[j], base, lane);
        carry[j] = total;
    }
}

// what the scan leaves the expansion in a row's second column, which the expansion turns back into
// the class: class, whether the run that ends here opens a request, the chain's form and open items
// in front of the block, and the length of the run of absent blocks that ends here (0: none does)
__device__ __forceinline__ uint64_t row_pack(uint32_t cls, bool opens, uint32_t form, uint32_t items, uint32_t run)
{
    return cls | ((uint64_t)opens << 2) | ((uint64_t)form << 3) | ((uint64_t)items << 8) | ((uint64_t)run << 32);
}

// Rows [0, nblocks) -> {byte offset of what is emitted at the block's position, packed chain state},
// row nblocks -> {bytes, requests}; totals.  A run of absent blocks is emitted at its last block.
// A thread takes kNackScanItems consecutive blocks: it folds them serially into a total, the
// threads' totals are scanned over the workgroup, and the thread walks its blocks again from the
// state in front of them; the running carries take the state to the next tile.  Four barriers a
// tile, each scan seeded by the one before (nack_layout.hpp, the operator): the run length, the
// chain's last form, the units since the form changed, and the open request's items together with
// the sums.  What a later scan needs of an earlier one stays in registers as bit fields: the
// classes and the forms two bits a block, the units, their item counts and the openers one; the
// run lengths are walked a second time where the rows are written.  (Each barrier's sums have
// an array of their own: the next tile's write of it lies behind three other barriers.)
template <bool ADV>
__global__ __launch_bounds__(kNackScanThreads) void nack_scan_kernel(NackArgs a)
{
    constexpr int K = kNackScanItems;
    __shared__ SegVal sums_run[1][kNackScanWaves], sums_form[1][kNackScanWaves], sums_since[1][kNackScanWaves],
        sums_rest[4][kNackScanWaves];
    __shared__ uint32_t own[kNackScanItems][kNackScanThreads];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t info = source_info<ADV>(a);
    const uint32_t L = a.item_len, bflags = REPAIR_BLOCK | info;
    SegVal c_run[1] = {{0, 0}}, c_form[1] = {{0, 0}}, c_since[1] = {{0, 0}};
    SegVal c_rest[4] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}};
    for (uint64_t t0 = 0; t0 <= a.nblocks; t0 += kNackScanTile) {
        const uint64_t i0 = t0 + (uint64_t)threadIdx.x * K;
        // the classes of the thread's blocks, and what the count kernel left of a needing block,
        // requests | items << 16, into the thread's own column of LDS (both fit 16 bits: a unit and
        // the gap behind it take two slots of 65,536); then the class of the block behind them (the
        // next thread's first, which that thread overwrites behind this tile's barriers)
        uint64_t classes = 0;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const uint64_t left = i0 + j < a.nblocks ? a.rows[2 * (i0 + j) + 1] : (uint64_t)NACK_SILENT;
            classes |= (left & 3u) << (2 * j);
            own[j][threadIdx.x] = ((uint32_t)(left >> 8) & 0xffffu) | ((uint32_t)(left >> 28) << 16);
        }
        const uint32_t behind = i0 + K < a.nblocks ? (uint32_t)a.rows[2 * (i0 + K) + 1] & 3u : (uint32_t)NACK_SILENT;
        auto cls = [&](int j) { return j < K ? (uint32_t)(classes >> (2 * j)) & 3u : behind; };
        SegVal acc, tot[1], pre[1];

        // the run of absent blocks so far
        uint32_t two = 0, lng = 0;  // the blocks whose run so far holds two items / has the RANGES form
        acc = SegVal{0, 0};
#pragma unroll 2
        for (int j = 0; j < K; ++j) acc = seg_combine(acc, cls(j) == NACK_ABSENT ? SegVal{1, 0} : SegVal{0, 1});
        tot[0] = acc;
        tile_scan<1>(tot, c_run, pre, sums_run, lane, wv);
        const SegVal run0 = acc = pre[0];
#pragma unroll 2
        for (int j = 0; j < K; ++j) {
            acc = seg_combine(acc, cls(j) == NACK_ABSENT ? SegVal{1, 0} : SegVal{0, 1});
            two |= (uint32_t)(nack_unit_items(acc.v) == 2u) << j;
            lng |= (uint32_t)(nack_unit_form(acc.v) == REPAIR_RANGES) << j;
        }
        auto form = [&](int j) { return (lng >> j) & 1u ? (uint32_t)REPAIR_RANGES : (uint32_t)REPAIR_ITEMS; };

        // the chain's last form in front of each block; a run ends, and is a unit, at its last block
        uint32_t units = 0;
        uint64_t forms = 0;
        auto form_element = [&](int j) {
            return cls(j) == NACK_NEEDING ? SegVal{0, 1} : (units >> j) & 1u ? SegVal{form(j), 1} : SegVal{0, 0};
        };
        acc = SegVal{0, 0};
#pragma unroll 2
        for (int j = 0; j < K; ++j) {
            units |= (uint32_t)(cls(j) == NACK_ABSENT && cls(j + 1) != NACK_ABSENT) << j;
            acc = seg_combine(acc, form_element(j));
        }
        tot[0] = acc;
        tile_scan<1>(tot, c_form, pre, sums_form, lane, wv);
        acc = pre[0];
#pragma unroll 2
        for (int j = 0; j < K; ++j) {
            forms |= (acc.v & 3u) << (2 * j);
            acc = seg_combine(acc, form_element(j));
        }
        auto form0 = [&](int j) { return (uint32_t)(forms >> (2 * j)) & 3u; };

        // the units since the form changed: which units open a request
        uint32_t opens = 0;
        auto since_element = [&](int j) {
            const bool unit = (units >> j) & 1u;
            return SegVal{unit, unit && form(j) != form0(j)};
        };
        acc = SegVal{0, 0};
#pragma unroll 2
        for (int j = 0; j < K; ++j) acc = seg_combine(acc, since_element(j));
        tot[0] = acc;
        tile_scan<1>(tot, c_since, pre, sums_since, lane, wv);
        acc = pre[0];
#pragma unroll 2
        for (int j = 0; j < K; ++j) {
            acc = seg_combine(acc, since_element(j));
            if (((units >> j) & 1u) && nack_opens((uint32_t)acc.v, a.max_units)) opens |= 1u << j;
        }

        // the open request's items, and the sums: bytes, requests, needing | absent blocks << 32
        SegVal state[4] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}}, before[4];
        auto add = [&](SegVal (&st)[4], int j) {
            const bool unit = (units >> j) & 1u, open = (opens >> j) & 1u, needing = cls(j) == NACK_NEEDING;
            const uint32_t items = (two >> j) & 1u ? 2u : 1u;
            st[0] = seg_combine(st[0], SegVal{unit ? items : 0u, open});
            const uint32_t mine = own[j][threadIdx.x], own_reqs = mine & 0xffffu, own_items = mine >> 16;
            st[1].v += needing ? 4ull * own_reqs + (uint64_t)L * own_items : unit ? (open ? 4u : 0u) + (uint64_t)L * items : 0u;
            st[2].v += needing ? own_reqs : (uint32_t)open;
            st[3].v += (uint64_t)needing | ((uint64_t)(cls(j) == NACK_ABSENT) << 32);
        };
#pragma unroll 2
        for (int j = 0; j < K; ++j) add(state, j);
        tile_scan<4>(state, c_rest, before, sums_rest, lane, wv);
        acc = run0;
#pragma unroll 2
        for (int j = 0; j < K; ++j) {
            const uint64_t i = i0 + j;
            acc = seg_combine(acc, cls(j) == NACK_ABSENT ? SegVal{1, 0} : SegVal{0, 1});  // the run again
            SegVal after[4] = {before[0], before[1], before[2], before[3]};
            add(after, j);
            const uint32_t items0 = (uint32_t)before[0].v;
            uint64_t bytes = before[1].v, reqs = before[2].v;
            if (i < a.nblocks) {
                a.rows[2 * i] = bytes;
                a.rows[2 * i + 1] = row_pack(cls(j), (opens >> j) & 1u, form0(j), items0, (units >> j) & 1u ? (uint32_t)acc.v : 0u);
            } else if (i == a.nblocks) {
                // the last chain's open request is closed by the end of the walk
                if (form0(j)) put32(a, bytes - (uint64_t)L * items0 - 4u, nack_header_word(form0(j), bflags, L * items0));
                if (ADV && adv_whole_object(uniform(*a.object))) {  // one OBJECT request (normSession.cpp:4602, :4662)
                    NackArgs g = a;
                    g.first_block_id = 0;
                    put32(a, 0, nack_header_word(REPAIR_ITEMS, REPAIR_OBJECT, L));
                    put_item(g, 4, 0, 0, a.k);
                    bytes = 4u + L, reqs = 1;
                } else if (bytes == 0 && info && a.nblocks) {  // the INFO-only request (normObject.cpp:1365-1372, :670-681)
                    NackArgs g = a;
                    g.first_block_id = 0;
                    put32(a, 0, nack_header_word(REPAIR_ITEMS, REPAIR_INFO, L));
                    put_item(g, 4, 0, 0, 0);
                    bytes = 4u + L, reqs = 1;
                }
                a.rows[2 * i] = bytes, a.rows[2 * i + 1] = reqs;
                a.totals[0] = bytes, a.totals[1] = reqs;
                a.totals[2] = (uint32_t)before[3].v, a.totals[3] = before[3].v >> 32;
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) before[q] = after[q];
        }
    }
}

// per block: its bytes, from block_start[b] on
template <bool ADV>
__global__ __launch_bounds__(256) void nack_expand_kernel(NackArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t b = uniform(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (b >= a.nblocks) return;
    const uint64_t packed = uniform64(a.rows[2 * (uint64_t)b + 1]);
    uint64_t off = uniform64(a.rows[2 * (uint64_t)b]);
    const uint32_t cls = (uint32_t)packed & 3u;
    if (lane == 0 && packed != cls) a.rows[2 * (uint64_t)b + 1] = cls;  // the row's second column is the class again
    if (cls == NACK_SILENT) return;
    const uint32_t info = source_info<ADV>(a);
    const uint32_t L = a.item_len, bflags = REPAIR_BLOCK | info;
    const bool opens = (packed >> 2) & 1u;
    const uint32_t form0 = (uint32_t)(packed >> 3) & 3u, items0 = (uint32_t)(packed >> 8) & 0xffffu;
    const uint32_t run = (uint32_t)(packed >> 32);
    // whatever closes the chain's open request writes its header, which lies in front of `off`
    const bool closes = form0 && (cls == NACK_NEEDING || (run && opens));
    if (closes && lane == 0) put32(a, off - (uint64_t)L * items0 - 4u, nack_header_word(form0, bflags, L * items0));
    if (off >= a.capacity) return;
    if (cls == NACK_ABSENT) {
        if (!run || run > b + 1u || lane) return;
        if (opens) off += 4;
        const uint32_t b0 = b - (run - 1u);
        put_item(a, off, b0, 0, a.num_data ? a.num_data[b0] : a.k);
        if (run >= 2) put_item(a, off + L, b, 0, a.num_data ? a.num_data[b] : a.k);
        return;
    }
    const uint32_t nd = a.num_data ? uniform(a.num_data[b]) : a.k;
    const uint32_t* mask = a.received + (uint64_t)b * a.mask_stride;
    const NackCut cut = ADV ? adv_cut(nd, a.m) : block_shape(a.k, a.m, mask, nd, lane).cut;
    uint32_t reqs, items;
    block_requests<true, ADV>(a, info, mask, b, nd, cut, lane, off, &reqs, &items);
}

}  // namespace

template <bool ADV>
static int launch_walk(const NackArgs& a, hipStream_t s, const char* what)
{
    const dim3 grid((a.nblocks + 3u) / 4u);
    if (a.nblocks) hipLaunchKernelGGL(nack_count_kernel<ADV>, grid, dim3(256), 0, s, a);
    hipLaunchKernelGGL(nack_scan_kernel<ADV>, dim3(1), dim3(kNackScanThreads), 0, s, a);
    if (a.nblocks) hipLaunchKernelGGL(nack_expand_kernel<ADV>, grid, dim3(256), 0, s, a);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? NFEC_OK : hip_fail(e, what);
}

// (the ABI entries have checked the arguments)
int launch_nack(const NackArgs& a, hipStream_t s) { return launch_walk<false>(a, s, "rx_repair_requests launch"); }

// a.received: the sender's repair mask; a.block_repair and a.object: the rest of its state
int launch_repair_adv(const NackArgs& a, hipStream_t s)
{
    if (a.nblocks == 0) {  // (no state to read: the totals and the last row of block_start are zero)
        NFEC_HIP(hipMemsetAsync(a.totals, 0, 4 * sizeof(uint64_t), s));
        NFEC_HIP(hipMemsetAsync(a.rows, 0, 2 * sizeof(uint64_t), s));
        return NFEC_OK;
    }
    return launch_walk<true>(a, s, "tx_repair_adv launch");
}

}  // namespace nfec
