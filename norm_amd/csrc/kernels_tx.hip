// kernels_tx.hip -- sender assembly on the device (nfec.h, "sender assembly on the device").
//
// list: the walk NormObject::NextSenderMsg makes once the parity exists (reference
//       src/common/normObject.cpp:1877, :1989): blocks ascending, within a block the pending slots
//       ascending; a source segment goes out at its own length, a parity segment at the block's
//       seg_size_max (:2035, :2050, :2071).  Every entry gets its packed wire offset.
// emit: each listed slot goes to its byte offset of the wire buffer behind its FEC payload ID
//       (:2078), and its pending bit is cleared (UnsetPending, :2075).
#include <algorithm>

#include "message_wave.hpp"
#include "rx_parse.hpp"
#include "segment_copy.hpp"

namespace nfec {

namespace {

// ---- the transmission list ----

// the block's seg_size_max: the longest of its nd source segments, pending or not
__device__ __forceinline__ uint32_t seg_size_max(const uint16_t* __restrict__ lens, uint32_t nd, uint32_t lane)
{
    uint32_t mx = 0;
    for (uint32_t s = lane; s < nd; s += 64) mx = max(mx, (uint32_t)lens[s]);
#pragma unroll
    for (uint32_t d = 32; d; d >>= 1) mx = max(mx, (uint32_t)__shfl_xor(mx, d, 64));
    return mx;
}

// What one lane holds of a block in one round: the pending bits of mask word w that lie in
// [0, n), how many they are, and the wire bytes of their messages (gap + payload each).
struct WordPart {
    uint32_t bits, count;
    uint64_t bytes;
};

__device__ __forceinline__ uint32_t slot_length(const TxListArgs& a, const uint16_t* __restrict__ lens, uint32_t s,
                                                uint32_t nd, uint32_t smax)
{
    return s >= nd ? smax : lens ? (uint32_t)lens[s] : a.vec;
}

__device__ __forceinline__ WordPart word_part(const TxListArgs& a, const uint32_t* __restrict__ mask,
                                              const uint16_t* __restrict__ lens, uint32_t w, uint32_t w_end, uint32_t n,
                                              uint32_t nd, uint32_t smax)
{
    WordPart r = {0u, 0u, 0u};
    if (w >= w_end) return r;
    const uint32_t first = w << 5;  // slot of bit 0
    r.bits = mask[w];
    if (n - first < 32u) r.bits &= (1u << (n - first)) - 1u;  // the partial last word
    r.count = __popc(r.bits);
    uint64_t sum = 0;
    if (!lens) {
        sum = (uint64_t)r.count * a.vec;
    } else {
        for (uint32_t rest = r.bits; rest; rest &= rest - 1u)
            sum += slot_length(a, lens, first + (__ffs(rest) - 1u), nd, smax);
    }
    r.bytes = sum + (uint64_t)r.count * a.gap;
    return r;
}

// per block: block_start[b] = {pending slots, their wire bytes}.  One wave per block, lanes over
// mask words, 64 words per round.
__global__ __launch_bounds__(256) void tx_count_kernel(TxListArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t b = uniform(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (b >= a.nblocks) return;
    const uint32_t nd = a.num_data ? uniform(a.num_data[b]) : a.k;
    uint64_t count = 0, bytes = 0;
    if (nd >= 1 && nd <= a.k) {
        const uint32_t* mask = a.pending + (uint64_t)b * a.mask_stride;
        const uint16_t* lens = a.seg_length ? a.seg_length + (uint64_t)b * a.length_stride : nullptr;
        const uint32_t smax = lens ? seg_size_max(lens, nd, lane) : a.vec;
        const uint32_t n = nd + a.m, w_end = (n + 31u) >> 5;
        for (uint32_t w0 = 0; w0 < w_end; w0 += 64) {
            const WordPart p = word_part(a, mask, lens, w0 + lane, w_end, n, nd, smax);
            count += p.count;
            bytes += p.bytes;
        }
        count = __shfl((unsigned long long)wave_scan(count, lane), 63, 64);
        bytes = __shfl((unsigned long long)wave_scan(bytes, lane), 63, 64);
    }
    if (lane == 0) a.block_start[2 * (uint64_t)b] = count, a.block_start[2 * (uint64_t)b + 1] = bytes;
}

// block_start rows [0, nblocks) -> their exclusive prefix sums, row nblocks -> the totals.  One
// workgroup of 1024 threads walks the rows in tiles of 1024 with a running carry: a megabyte for
// 65,536 blocks, which is microseconds beside the emission the list is for.
constexpr uint32_t kScanThreads = 1024;

__global__ __launch_bounds__(kScanThreads) void tx_scan_kernel(uint64_t* __restrict__ rows, uint32_t nblocks)
{
    __shared__ uint64_t wave_sum[2][kScanThreads / 64][2];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    uint64_t carry_c = 0, carry_y = 0;
    uint32_t flip = 0;
    for (uint64_t t0 = 0; t0 <= nblocks; t0 += kScanThreads, flip ^= 1u) {
        const uint64_t i = t0 + threadIdx.x;
        uint64_t c = 0, y = 0;
        if (i < nblocks) c = rows[2 * i], y = rows[2 * i + 1];
        const uint64_t inc_c = wave_scan(c, lane), inc_y = wave_scan(y, lane);
        if (lane == 63) wave_sum[flip][wv][0] = inc_c, wave_sum[flip][wv][1] = inc_y;
        __syncthreads();  // (the other half of wave_sum is the previous tile's: no second barrier)
        uint64_t base_c = carry_c, base_y = carry_y;
        for (uint32_t v = 0; v < kScanThreads / 64; ++v) {
            const uint64_t sc = wave_sum[flip][v][0], sy = wave_sum[flip][v][1];
            if (v < wv) base_c += sc, base_y += sy;
            carry_c += sc, carry_y += sy;
        }
        if (i <= nblocks) rows[2 * i] = base_c + inc_c - c, rows[2 * i + 1] = base_y + inc_y - y;
    }
}

// per block: its entries, from block_start[b] = {first entry, first byte} on.  Each lane prefix-
// sums the lengths of its word's pending bits, a wave scan places the words, and the lane walks
// its bits.  Entries at or past `capacity` are not written.
__global__ __launch_bounds__(256) void tx_expand_kernel(TxListArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t b = uniform(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (b >= a.nblocks) return;
    const uint32_t nd = a.num_data ? uniform(a.num_data[b]) : a.k;
    if (nd < 1 || nd > a.k) return;
    uint64_t at0 = a.block_start[2 * (uint64_t)b], byte0 = a.block_start[2 * (uint64_t)b + 1];
    if (at0 >= a.capacity) return;
    const uint32_t* mask = a.pending + (uint64_t)b * a.mask_stride;
    const uint16_t* lens = a.seg_length ? a.seg_length + (uint64_t)b * a.length_stride : nullptr;
    const uint32_t smax = lens ? seg_size_max(lens, nd, lane) : a.vec;
    const uint32_t n = nd + a.m, w_end = (n + 31u) >> 5;
    for (uint32_t w0 = 0; w0 < w_end; w0 += 64) {
        const uint32_t w = w0 + lane;
        const WordPart p = word_part(a, mask, lens, w, w_end, n, nd, smax);
        const uint32_t inc_n = wave_scan(p.count, lane);
        const uint64_t inc_y = wave_scan(p.bytes, lane);
        uint64_t at = at0 + (inc_n - p.count), byte = byte0 + (inc_y - p.bytes);
        for (uint32_t rest = p.bits; rest && at < a.capacity; rest &= rest - 1u, ++at) {
            const uint32_t s = (w << 5) + (__ffs(rest) - 1u);
            const uint32_t len = slot_length(a, lens, s, nd, smax);
            a.offsets[at] = byte + a.gap;
            a.block_index[at] = b;
            a.symbol_id[at] = (uint16_t)s;
            a.length[at] = (uint16_t)len;
            byte += (uint64_t)a.gap + len;
        }
        at0 += __shfl(inc_n, 63, 64);
        byte0 += __shfl((unsigned long long)inc_y, 63, 64);
    }
}

// ---- emission ----

// One message by one wave: the payload ID and the slot's first `len` bytes to the wire bytes [dst,
// dst + idlen + len).  rx_place's copy turned round (segment_copy.hpp, the scatter rule): lane L
// takes the aligned 16-byte pieces L, L + 64, ... of the wire bytes.  The shift between the slot
// and the wire is the same for every piece, so the rule's funnel shift and dword pick are
// wave-uniform.
__device__ __forceinline__ void emit_message(uint8_t* __restrict__ dst, const uint8_t* __restrict__ slot, uint32_t len,
                                             uint64_t id, uint32_t idlen, uint32_t lane)
{
    const uint32_t pieces = scatter_pieces(dst, idlen + len);
    for (uint32_t p = lane; p < pieces; p += 64) scatter_piece(dst, slot, len, id, idlen, p);
}

// One wave per entry (message_wave.hpp): the next entry's descriptor is requested before this one
// is copied; stats: emitted, rejected.
__global__ __launch_bounds__(256) void tx_emit_kernel(TxEmitArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = uniform(blockIdx.x * 4u + (threadIdx.x >> 6));
    const uint32_t nwaves = gridDim.x * 4u;
    const uint32_t idlen = payload_id_length(a.id_kind);
    const uint64_t count = message_count(a.count, a.count_dev);
    uint32_t n_emitted = 0, n_rej = 0;
    Descriptor next;
    if (wave < count) next.request(a, wave);
    for (uint64_t i = wave; i < count; i += nwaves) {
        const Descriptor d = next.taken();
        if (i + nwaves < count) next.request(a, i + nwaves);
        const uint32_t nd = d.len <= a.batch.vec && rx_readable(d.off, d.len, idlen, a.payload_bytes)
                                ? slot_num_data(a.batch, d.b, d.s)
                                : 0;
        if (!nd) {
            ++n_rej;
            continue;
        }
        ++n_emitted;
        if (a.pending && lane == 0)
            atomicAnd(a.pending + (uint64_t)d.b * a.mask_stride + (d.s >> 5), ~(1u << (d.s & 31u)));
        emit_message(a.payloads + (d.off - idlen), slot_address(a.batch, d.b, d.s), d.len,
                     payload_id(a.id_kind, a.first_block_id + d.b, d.s, nd), idlen, lane);
    }
    flush_stats(a.stats, lane, n_emitted, n_rej);
}

}  // namespace

int launch_tx_list(const TxListArgs& a, hipStream_t s)
{
    if (!a.block_start) return fail(NFEC_EINVAL, "tx_list: null block_start");
    if (a.nblocks) {
        if (!a.pending) return fail(NFEC_EINVAL, "tx_list: null pending mask");
        if ((uint64_t)a.mask_stride * 32u < (uint64_t)a.k + a.m)
            return fail(NFEC_EINVAL, "tx_list: mask_stride smaller than (k + m + 31) / 32");
        if (a.seg_length && a.length_stride < a.k) return fail(NFEC_EINVAL, "tx_list: length_stride < k");
        if (a.capacity && (!a.offsets || !a.block_index || !a.symbol_id || !a.length))
            return fail(NFEC_EINVAL, "tx_list: null output array");
        hipLaunchKernelGGL(tx_count_kernel, dim3((a.nblocks + 3u) / 4u), dim3(256), 0, s, a);
    }
    hipLaunchKernelGGL(tx_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, a.block_start, a.nblocks);
    if (a.nblocks && a.capacity) hipLaunchKernelGGL(tx_expand_kernel, dim3((a.nblocks + 3u) / 4u), dim3(256), 0, s, a);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? NFEC_OK : hip_fail(e, "tx_list launch");
}

// (the ABI entry has checked the arguments and returned for an empty batch or list)
int launch_tx_emit(const TxEmitArgs& a, hipStream_t s)
{
    constexpr uint32_t kMaxGroups = 8192;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(((uint64_t)a.count + 3u) / 4u, kMaxGroups);
    hipLaunchKernelGGL(tx_emit_kernel, dim3(grid), dim3(256), 0, s, a);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? NFEC_OK : hip_fail(e, "tx_emit launch");
}

}  // namespace nfec
