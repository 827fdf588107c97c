// kernels_tx.hip -- sender assembly on the device (nfec.h, "sender assembly on the device").
//
// list: the walk NormObject::NextSenderMsg makes once the parity exists (reference
//       src/common/normObject.cpp:1877, :1989): blocks ascending, within a block the pending slots
//       ascending; a source segment goes out at its own length, a parity segment at the block's
//       seg_size_max (:2035, :2050, :2071).  Every entry gets its packed wire offset.
// emit: each listed slot goes to its byte offset of the wire buffer behind its FEC payload ID
//       (:2078), and its pending bit is cleared (UnsetPending, :2075).
#include <algorithm>

#include "nfec_internal.hpp"

namespace nfec {

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t uniform(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }

// ---- the transmission list ----

// inclusive prefix sum of v over the wave's 64 lanes
__device__ __forceinline__ uint64_t wave_scan64(uint64_t v, uint32_t lane)
{
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint64_t up = __shfl_up((unsigned long long)v, d, 64);
        if (lane >= d) v += up;
    }
    return v;
}

__device__ __forceinline__ uint32_t wave_scan32(uint32_t v, uint32_t lane)
{
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(v, d, 64);
        if (lane >= d) v += up;
    }
    return v;
}

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
        count = __shfl((unsigned long long)wave_scan64(count, lane), 63, 64);
        bytes = __shfl((unsigned long long)wave_scan64(bytes, lane), 63, 64);
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
        const uint64_t inc_c = wave_scan64(c, lane), inc_y = wave_scan64(y, lane);
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
        const uint32_t inc_n = wave_scan32(p.count, lane);
        const uint64_t inc_y = wave_scan64(p.bytes, lane);
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

// One message by one wave: `idlen` bytes of payload ID (byte j of it is bits [8j, 8j + 8) of `id`)
// and the slot's first `len` bytes go to the wire bytes [dst, dst + idlen + len), dst at any byte
// alignment.  rx_place's copy turned round: here the source is aligned and the destination is
// not.  The wire bytes are cut into the aligned 16-byte pieces that hold them; lane L takes pieces
// L, L + 64, ...  A piece's slot bytes start `sh` bytes into a 16-byte step of the slot, the same
// sh for every piece, so the funnel shift (v_alignbyte_b32) and the dword pick are wave-uniform.
// Loads are 8-byte chunks of the slot (a slot is 8-byte, not 16-byte, aligned, and it may end the
// allocation): three cover a piece's 16 bytes at any shift, and a chunk is loaded only when it
// holds a payload byte the piece stores, which keeps every load inside [slot, slot + len rounded
// up to 8) and so inside seg_stride.  A piece wholly inside the message is one 16-byte store; the
// first and the last piece store only their own bytes, as dwords where a whole dword is theirs and
// bytes elsewhere: the neighbouring message, written by another wave at the same time, may share
// the piece, so nothing outside the message is stored or read.
__device__ __forceinline__ void emit_message(uint8_t* __restrict__ dst, const uint8_t* __restrict__ slot, uint32_t len,
                                             uint64_t id, uint32_t idlen, uint32_t lane)
{
    const uint32_t total = idlen + len;
    if (total == 0) return;
    const uint32_t dres = (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u);
    uint8_t* __restrict__ piece0 = dst - dres;
    // slot byte 0 lies q bytes into piece 0: piece p holds slot bytes [16 (p - pb) + sh, + 16)
    const uint32_t q = dres + idlen;
    const int32_t pb = (int32_t)((q + 15u) >> 4);
    const uint32_t sh = (0u - q) & 15u;
    const uint32_t dsh = (sh >> 2) & 1u, bsh = sh & 3u;
    const uint32_t pieces = (dres + total + 15u) >> 4;
    const u32x2* __restrict__ chunk = reinterpret_cast<const u32x2*>(slot);
    for (uint32_t p = lane; p < pieces; p += 64) {
        const int32_t sidx = 16 * ((int32_t)p - pb) + (int32_t)sh;  // the piece's first slot byte (may be < 0)
        const int32_t need_lo = max(sidx, 0), need_hi = min(sidx + 16, (int32_t)len);
        const int32_t c0 = 2 * ((int32_t)p - pb) + (int32_t)(sh >> 3);
        uint32_t e[6];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int32_t c = c0 + j;
            u32x2 v = {0u, 0u};
            if (8 * c < need_hi && 8 * c + 8 > need_lo) v = __builtin_nontemporal_load(chunk + c);
            e[2 * j] = v.x, e[2 * j + 1] = v.y;
        }
        uint32_t o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            o[j] = __builtin_amdgcn_alignbyte(dsh ? e[j + 2] : e[j + 1], dsh ? e[j + 1] : e[j], bsh);
        const uint32_t first = p * 16u;  // the piece's first byte, counted from piece 0
        if (first < q) {
            // the piece holds ID bytes: byte t of it is message byte first + t - dres
#pragma unroll
            for (int w = 0; w < 4; ++w)
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const uint32_t j = first + 4u * w + t - dres;  // (wraps below the message: j >= idlen)
                    if (j < idlen) o[w] = (o[w] & ~(0xffu << (8 * t))) | ((uint32_t)((id >> (8u * j)) & 0xffu) << (8 * t));
                }
        }
        // the piece's own bytes [lo, hi)
        const uint32_t lo = p == 0 ? dres : 0u;
        const uint32_t hi = min(16u, dres + total - first);
        uint8_t* d = piece0 + first;
        if (lo == 0 && hi == 16) {
            *reinterpret_cast<u32x4*>(d) = u32x4{o[0], o[1], o[2], o[3]};
        } else {
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const uint32_t at = 4u * w;
                if (lo <= at && at + 4u <= hi) {
                    *reinterpret_cast<uint32_t*>(d + at) = o[w];
                } else {
#pragma unroll
                    for (int t = 0; t < 4; ++t)
                        if (lo <= at + t && at + t < hi) d[at + t] = (uint8_t)(o[w] >> (8 * t));
                }
            }
        }
    }
}

__device__ __forceinline__ uint32_t bswap16(uint32_t v) { return ((v & 0xffu) << 8) | ((v >> 8) & 0xffu); }

// the FEC payload ID as nfec_payload_id_write lays it out (wire.cpp), byte j in bits [8j, 8j + 8)
__device__ __forceinline__ uint64_t payload_id(uint32_t kind, uint32_t block_id, uint32_t s, uint32_t nd)
{
    switch (kind) {
    case TX_ID_BLOCK24: return __builtin_bswap32((block_id << 8) | (s & 0xffu));
    case TX_ID_BLOCK16: return bswap16(block_id & 0xffffu) | (bswap16(s) << 16);
    case TX_ID_BLOCK32_LEN:
        return (uint64_t)__builtin_bswap32(block_id) | ((uint64_t)(bswap16(nd) | (bswap16(s) << 16)) << 32);
    default: return 0;
    }
}

// A few thousand workgroups of four waves; each wave takes entries wave, wave + nwaves, ... one at
// a time, requests the next descriptor before it copies this one, and adds its emitted / rejected
// counts to `stats` once, at its end.
__global__ __launch_bounds__(256) void tx_emit_kernel(TxEmitArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = uniform(blockIdx.x * 4u + (threadIdx.x >> 6));
    const uint32_t nwaves = gridDim.x * 4u;
    const uint32_t idlen = a.id_kind == TX_ID_NONE ? 0u : a.id_kind == TX_ID_BLOCK32_LEN ? 8u : 4u;
    uint64_t count = a.count;
    if (a.count_dev) {
        const uint64_t v = *a.count_dev;
        const uint64_t have = ((uint64_t)uniform((uint32_t)(v >> 32)) << 32) | uniform((uint32_t)v);
        count = min(count, have);
    }
    uint32_t n_emitted = 0, n_rej = 0;
    uint32_t v_b = 0, v_s = 0, v_len = 0;
    uint64_t v_off = 0;
    if (wave < count) v_b = a.block_index[wave], v_s = a.symbol_id[wave], v_len = a.length[wave], v_off = a.offsets[wave];
    for (uint64_t i = wave; i < count; i += nwaves) {
        const uint32_t b = uniform(v_b), s = uniform(v_s), len = uniform(v_len);
        const uint64_t off = ((uint64_t)uniform((uint32_t)(v_off >> 32)) << 32) | uniform((uint32_t)v_off);
        const uint64_t nxt = i + nwaves;
        if (nxt < count) v_b = a.block_index[nxt], v_s = a.symbol_id[nxt], v_len = a.length[nxt], v_off = a.offsets[nxt];
        bool ok = b < a.nblocks && len <= a.vec && off >= idlen && off <= a.payload_bytes && len <= a.payload_bytes - off;
        uint32_t nd = 0;
        if (ok) {
            nd = a.num_data ? uniform(a.num_data[b]) : a.k;
            ok = nd >= 1 && nd <= a.k && s < nd + a.m;
        }
        if (!ok) {
            ++n_rej;
            continue;
        }
        ++n_emitted;
        if (a.pending && lane == 0) atomicAnd(a.pending + (uint64_t)b * a.mask_stride + (s >> 5), ~(1u << (s & 31u)));
        emit_message(a.payloads + (off - idlen), a.base + (uint64_t)b * a.block_stride + (uint64_t)s * a.seg_stride, len,
                     payload_id(a.id_kind, a.first_block_id + b, s, nd), idlen, lane);
    }
    if (a.stats && lane == 0) {
        if (n_emitted) atomicAdd(a.stats + 0, n_emitted);
        if (n_rej) atomicAdd(a.stats + 1, n_rej);
    }
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

int launch_tx_emit(const TxEmitArgs& a, hipStream_t s)
{
    if (a.count == 0 || a.nblocks == 0) return NFEC_OK;
    if (!a.base) return fail(NFEC_EINVAL, "tx_emit: null blocks pointer");
    if (!a.payloads) return fail(NFEC_EINVAL, "tx_emit: null payloads");
    if (!a.offsets) return fail(NFEC_EINVAL, "tx_emit: null offsets");
    if (!a.block_index) return fail(NFEC_EINVAL, "tx_emit: null block_index");
    if (!a.symbol_id) return fail(NFEC_EINVAL, "tx_emit: null symbol_id");
    if (!a.length) return fail(NFEC_EINVAL, "tx_emit: null length");
    if (a.pending && (uint64_t)a.mask_stride * 32u < (uint64_t)a.k + a.m)
        return fail(NFEC_EINVAL, "tx_emit: mask_stride smaller than (k + m + 31) / 32");
    if ((reinterpret_cast<uintptr_t>(a.base) | a.block_stride | a.seg_stride) & 7)
        return fail(NFEC_EINVAL, "tx_emit: blocks, seg_stride and block_stride must be multiples of 8 bytes");
    if (a.seg_stride < a.vec) return fail(NFEC_EINVAL, "tx_emit: seg_stride < vector_size");
    constexpr uint32_t kMaxGroups = 8192;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(((uint64_t)a.count + 3u) / 4u, kMaxGroups);
    hipLaunchKernelGGL(tx_emit_kernel, dim3(grid), dim3(256), 0, s, a);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? NFEC_OK : hip_fail(e, "tx_emit launch");
}

}  // namespace nfec
