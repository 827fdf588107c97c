// kernels_rx.hip -- receiver assembly on the device (nfec.h, "receiver assembly on the device").
//
// place:    received segments, in arrival order and at any byte offset of a payload buffer, go
//           into their (block, slot) of a device batch.  The slot is claimed by one atomic OR on
//           the block's reception mask (NORM's IsPending test at the top of
//           NormObject::HandleObjectMessage, reference src/common/normObject.cpp:1548-1644, made
//           race-free), so exactly one of several copies of a segment is written.
// erasures: the per-block erasure list NormObject builds from its mask before Decode
//           (normObject.cpp:1560-1606): missing source slots, then missing parity slots, and
//           nothing at all for a block whose source is complete.
#include <algorithm>

#include "nfec_internal.hpp"
#include "rx_parse.hpp"

namespace nfec {

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t uniform(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }

// the low n bytes of a dword (n <= 0: none, n >= 4: all)
__device__ __forceinline__ uint32_t low_bytes(int32_t n) { return n >= 4 ? ~0u : n <= 0 ? 0u : (1u << (8 * n)) - 1u; }

// One segment by one wave.  The slot is 8-byte aligned, the payload is not: lane L takes the 16
// destination bytes [16p, 16p + 16) (p = L, L + 64, ...) from the two aligned 16-byte source
// chunks that hold them, shifted by the payload's misalignment sh = 4 dsh + bsh (dsh picks the
// dwords -- wave-uniform, so a uniform branch -- and v_alignbyte_b32 funnels the bytes).  A chunk
// is loaded only when it holds a payload byte the piece needs: the chunk past a piece is skipped
// when sh == 0 or the payload ends before it, so every load stays on a page the payload touches.
// Bytes from `len` to `vec` are zeros (the reference's zero pad of a short segment); whole 8-byte
// pieces are stored as such, and only the piece that holds byte `vec` is stored by bytes, so the
// stride padding past `vec` keeps the caller's bytes.
__device__ __forceinline__ void place_segment(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, uint32_t len,
                                              uint32_t vec, uint32_t lane)
{
    const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(src) & 15u);
    const uint32_t dsh = sh >> 2, bsh = sh & 3u;
    const u32x4* __restrict__ chunk0 = reinterpret_cast<const u32x4*>(src - sh);
    const uint32_t pieces = (vec + 15u) / 16u;
    for (uint32_t p = lane; p < pieces; p += 64) {
        const uint32_t d0 = p * 16u;
        const int32_t nvalid = (int32_t)len - (int32_t)d0;  // payload bytes from d0 on (may be <= 0 or > 16)
        uint32_t o[4] = {0u, 0u, 0u, 0u};
        if (nvalid > 0) {
            const u32x4 q0 = __builtin_nontemporal_load(chunk0 + p);
            u32x4 q1 = {0u, 0u, 0u, 0u};
            if (sh != 0 && (int32_t)sh + nvalid > 16) q1 = __builtin_nontemporal_load(chunk0 + p + 1);
            uint32_t e[5];
            switch (dsh) {
            case 0: e[0] = q0.x, e[1] = q0.y, e[2] = q0.z, e[3] = q0.w, e[4] = q1.x; break;
            case 1: e[0] = q0.y, e[1] = q0.z, e[2] = q0.w, e[3] = q1.x, e[4] = q1.y; break;
            case 2: e[0] = q0.z, e[1] = q0.w, e[2] = q1.x, e[3] = q1.y, e[4] = q1.z; break;
            default: e[0] = q0.w, e[1] = q1.x, e[2] = q1.y, e[3] = q1.z, e[4] = q1.w; break;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
                o[j] = __builtin_amdgcn_alignbyte(e[j + 1], e[j], bsh) & low_bytes(nvalid - 4 * j);
        }
        const uint32_t nw = vec - d0;  // bytes of this piece inside the vector (> 0; >= 16: all)
        uint8_t* d = dst + d0;
        if (nw >= 16) {
            *reinterpret_cast<u32x2*>(d) = u32x2{o[0], o[1]};
            *reinterpret_cast<u32x2*>(d + 8) = u32x2{o[2], o[3]};
        } else {
            uint32_t lo = o[0], hi = o[1], done = 0;
            if (nw >= 8) {
                *reinterpret_cast<u32x2*>(d) = u32x2{o[0], o[1]};
                lo = o[2], hi = o[3], done = 8;
            }
            const uint64_t v = ((uint64_t)hi << 32) | lo;
            for (uint32_t t = done; t < nw; ++t) d[t] = (uint8_t)(v >> (8 * (t - done)));
        }
    }
}

// A few thousand workgroups of four waves; each wave takes segments wave, wave + nwaves, ... one
// at a time and adds its placed / duplicate / rejected counts to `stats` once, at its end (one
// atomic per wave and counter instead of one per segment on a single address).
__global__ __launch_bounds__(256) void rx_place_kernel(RxPlaceArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = uniform(blockIdx.x * 4u + (threadIdx.x >> 6));
    const uint32_t nwaves = gridDim.x * 4u;
    uint32_t n_placed = 0, n_dup = 0, n_rej = 0;
    // the descriptor: every lane reads the same words (one request each); the next segment's is
    // requested before this one's copy, so its latency hides behind the copy
    uint32_t v_b = 0, v_s = 0, v_len = 0;
    uint64_t v_off = 0;
    if (wave < a.count) v_b = a.block_index[wave], v_s = a.symbol_id[wave], v_len = a.length[wave], v_off = a.offsets[wave];
    for (uint64_t i = wave; i < a.count; i += nwaves) {
        const uint32_t b = uniform(v_b), s = uniform(v_s), len = uniform(v_len);
        const uint64_t off = ((uint64_t)uniform((uint32_t)(v_off >> 32)) << 32) | uniform((uint32_t)v_off);
        const uint64_t nxt = i + nwaves;
        if (nxt < a.count) v_b = a.block_index[nxt], v_s = a.symbol_id[nxt], v_len = a.length[nxt], v_off = a.offsets[nxt];
        bool ok = b < a.nblocks && len <= a.vec;
        if (ok) {
            const uint32_t nd = a.num_data ? uniform(a.num_data[b]) : a.k;
            ok = nd >= 1 && nd <= a.k && s < nd + a.m;
        }
        if (!ok) {
            ++n_rej;
            continue;
        }
        // lane 0 claims the slot; the outcome goes to the whole wave
        uint32_t was = 0;
        if (lane == 0) {
            const uint32_t bit = 1u << (s & 31u);
            was = atomicOr(a.received + (uint64_t)b * a.mask_stride + (s >> 5), bit) & bit;
        }
        was = __builtin_amdgcn_readlane(was, 0);
        if (was) {
            ++n_dup;
            continue;
        }
        ++n_placed;
        place_segment(a.base + (uint64_t)b * a.block_stride + (uint64_t)s * a.seg_stride, a.payloads + off, len, a.vec,
                      lane);
    }
    if (a.stats && lane == 0) {
        if (n_placed) atomicAdd(a.stats + 0, n_placed);
        if (n_dup) atomicAdd(a.stats + 1, n_dup);
        if (n_rej) atomicAdd(a.stats + 2, n_rej);
    }
}

// ---- intake: (block, slot) from the FEC payload ID in front of the payload ----

// The aligned 16-byte chunk that holds the ID's first byte and, when the ID straddles a chunk
// boundary, the one after it.  Every lane reads the same address: one request per chunk.  Both
// chunks hold an ID byte, so neither leaves a page the message touches.
struct IdChunks {
    u32x4 q0, q1;
};
__device__ __forceinline__ IdChunks load_id(const uint8_t* __restrict__ id, uint32_t idlen)
{
    const uint32_t res = (uint32_t)(reinterpret_cast<uintptr_t>(id) & 15u);
    const u32x4* __restrict__ chunk = reinterpret_cast<const u32x4*>(id - res);
    IdChunks c;
    c.q0 = chunk[0];
    c.q1 = u32x4{0u, 0u, 0u, 0u};
    if (res + idlen > 16u) c.q1 = chunk[1];
    return c;
}

// The ID's bytes 0-3 and 4-7 out of the chunks, as rx_id_decode takes them: the dword pick is a
// uniform branch (res is wave-uniform), v_alignbyte_b32 funnels the bytes, and the result goes to
// scalar registers.  A word past the ID's length may hold anything; rx_id_decode does not read it.
__device__ __forceinline__ void id_words(const IdChunks& c, uint32_t res, uint32_t& w0, uint32_t& w1)
{
    const uint32_t dsh = res >> 2, bsh = res & 3u;
    uint32_t e0, e1, e2;
    switch (dsh) {
    case 0: e0 = c.q0.x, e1 = c.q0.y, e2 = c.q0.z; break;
    case 1: e0 = c.q0.y, e1 = c.q0.z, e2 = c.q0.w; break;
    case 2: e0 = c.q0.z, e1 = c.q0.w, e2 = c.q1.x; break;
    default: e0 = c.q0.w, e1 = c.q1.x, e2 = c.q1.y; break;
    }
    w0 = uniform(__builtin_amdgcn_alignbyte(e1, e0, bsh));
    w1 = uniform(__builtin_amdgcn_alignbyte(e2, e1, bsh));
}

// rx_place_kernel's shape: one wave per message, four waves per workgroup, the workgroups striding
// over the messages, the counters added once per wave.  A message needs three dependent fetches
// before its copy (descriptor, ID, mask), so the wave runs them one message apart: message i + 1's
// ID chunks and message i + 2's (offset, length) are requested ahead of message i's claim and
// arrive with its answer, so a message costs the wave one round trip before its copy, as in
// rx_place_kernel, and a duplicate costs that round trip alone.
__global__ __launch_bounds__(256) void rx_ingest_kernel(RxIngestArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = uniform(blockIdx.x * 4u + (threadIdx.x >> 6));
    const uint32_t nwaves = gridDim.x * 4u;
    const uint32_t idlen = rx_id_length(a.id_kind);
    uint64_t count = a.count;
    if (a.count_dev) {
        const uint64_t v = *a.count_dev;
        const uint64_t have = ((uint64_t)uniform((uint32_t)(v >> 32)) << 32) | uniform((uint32_t)v);
        count = min(count, have);
    }
    if (wave >= count) return;
    uint32_t n_placed = 0, n_dup = 0, n_rej = 0;
    // message `wave`: its descriptor and its ID; then the next one's descriptor
    uint32_t v_len = a.length[wave];
    uint64_t v_off = a.offsets[wave];
    uint32_t len = uniform(v_len);
    uint64_t off = ((uint64_t)uniform((uint32_t)(v_off >> 32)) << 32) | uniform((uint32_t)v_off);
    bool readable = rx_readable(off, len, idlen, a.payload_bytes);
    IdChunks id{};
    if (readable) id = load_id(a.payloads + (off - idlen), idlen);
    if ((uint64_t)wave + nwaves < count) v_len = a.length[wave + nwaves], v_off = a.offsets[wave + nwaves];
    for (uint64_t i = wave; i < count; i += nwaves) {
        // message i + nwaves: its descriptor is here (requested an iteration ago, ahead of that
        // message's claim, whose round trip it shared); request its ID and the descriptor of the
        // message after it now, ahead of this message's claim
        const uint64_t nxt = i + nwaves;
        uint32_t n_len = 0;
        uint64_t n_off = 0;
        bool n_readable = false;
        IdChunks n_id{};
        if (nxt < count) {
            n_len = uniform(v_len);
            n_off = ((uint64_t)uniform((uint32_t)(v_off >> 32)) << 32) | uniform((uint32_t)v_off);
            n_readable = rx_readable(n_off, n_len, idlen, a.payload_bytes);
            if (n_readable) n_id = load_id(a.payloads + (n_off - idlen), idlen);
            if (nxt + nwaves < count) v_len = a.length[nxt + nwaves], v_off = a.offsets[nxt + nwaves];
        }
        // parse and claim message i: its ID was requested an iteration ago
        uint32_t b = 0xffffffffu, s = 0xffffu;
        bool place = false;
        if (readable) {
            uint32_t w0, w1;
            id_words(id, (uint32_t)(reinterpret_cast<uintptr_t>(a.payloads + (off - idlen)) & 15u), w0, w1);
            const RxId pid = rx_id_decode(a.id_kind, w0, w1, a.first_block_id);
            b = pid.block, s = pid.symbol;
            bool ok = b < a.nblocks && len <= a.vec;
            if (ok) {
                const uint32_t nd = a.num_data ? uniform(a.num_data[b]) : a.k;
                ok = nd >= 1 && nd <= a.k && s < nd + a.m && (a.id_kind != RX_ID_BLOCK32_LEN || pid.block_len == nd);
            }
            if (ok) {
                // lane 0 claims the slot; the outcome goes to the whole wave
                uint32_t was = 0;
                if (lane == 0) {
                    const uint32_t bit = 1u << (s & 31u);
                    was = atomicOr(a.received + (uint64_t)b * a.mask_stride + (s >> 5), bit) & bit;
                }
                was = __builtin_amdgcn_readlane(was, 0);
                if (was) ++n_dup;
                else ++n_placed, place = true;
            } else {
                ++n_rej;
            }
        } else {
            ++n_rej;
        }
        if (lane == 0) {
            if (a.block_index_out) a.block_index_out[i] = b;
            if (a.symbol_id_out) a.symbol_id_out[i] = (uint16_t)s;
        }
        if (place)
            place_segment(a.base + (uint64_t)b * a.block_stride + (uint64_t)s * a.seg_stride, a.payloads + off, len,
                          a.vec, lane);
        len = n_len, off = n_off, readable = n_readable, id = n_id;
    }
    if (a.stats && lane == 0) {
        if (n_placed) atomicAdd(a.stats + 0, n_placed);
        if (n_dup) atomicAdd(a.stats + 1, n_dup);
        if (n_rej) atomicAdd(a.stats + 2, n_rej);
    }
}

// exclusive prefix sum of v over the wave's 64 lanes; total: the sum over all of them
__device__ __forceinline__ uint32_t wave_scan(uint32_t v, uint32_t lane, uint32_t& total)
{
    uint32_t inc = v;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(inc, d, 64);
        if (lane >= d) inc += up;
    }
    total = __shfl(inc, 63, 64);
    return inc - v;
}

// the missing slots of [lo, hi) ascending into locs[pos ...] (entries at or past `stride` are
// counted, not written); returns how many.  Lanes take mask words, 64 words per round.
__device__ __forceinline__ uint32_t list_missing(const uint32_t* __restrict__ mask, uint32_t lo, uint32_t hi,
                                                 uint16_t* __restrict__ locs, uint32_t stride, uint32_t pos,
                                                 uint32_t lane)
{
    uint32_t found = 0;
    if (hi <= lo) return 0;
    const uint32_t w_end = (hi + 31u) >> 5;
    for (uint32_t w0 = lo >> 5; w0 < w_end; w0 += 64) {
        const uint32_t w = w0 + lane;
        uint32_t miss = 0;
        if (w < w_end) {
            const uint32_t first = w << 5;  // slot of bit 0
            miss = ~mask[w];
            if (first < lo) miss &= ~0u << (lo - first);            // the word that straddles lo
            if (hi - first < 32u) miss &= (1u << (hi - first)) - 1u; // the partial last word
        }
        uint32_t total;
        uint32_t at = pos + found + wave_scan(__popc(miss), lane, total);
        while (miss) {
            const uint32_t t = __ffs(miss) - 1u;
            if (at < stride) locs[at] = (uint16_t)((w << 5) + t);
            ++at;
            miss &= miss - 1u;
        }
        found += total;
    }
    return found;
}

__global__ __launch_bounds__(256) void rx_erasures_kernel(RxErasureArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t b = uniform(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (b >= a.nblocks) return;
    const uint32_t nd = a.num_data ? uniform(a.num_data[b]) : a.k;
    uint32_t count = 0;
    if (nd >= 1 && nd <= a.k) {
        const uint32_t* mask = a.received + (uint64_t)b * a.mask_stride;
        uint16_t* locs = a.locs + (uint64_t)b * a.stride;
        count = list_missing(mask, 0, nd, locs, a.stride, 0, lane);
        // a block with its source complete is not decoded: no list, missing parity or not
        if (count) count += list_missing(mask, nd, nd + a.m, locs, a.stride, count, lane);
    }
    if (lane == 0) a.counts[b] = (uint16_t)min(count, 65535u);
}

}  // namespace

int launch_rx_place(const RxPlaceArgs& a, hipStream_t s)
{
    if (a.count == 0 || a.nblocks == 0) return NFEC_OK;
    if (!a.base) return fail(NFEC_EINVAL, "rx_place: null blocks pointer");
    if (!a.payloads) return fail(NFEC_EINVAL, "rx_place: null payloads");
    if (!a.offsets) return fail(NFEC_EINVAL, "rx_place: null offsets");
    if (!a.block_index) return fail(NFEC_EINVAL, "rx_place: null block_index");
    if (!a.symbol_id) return fail(NFEC_EINVAL, "rx_place: null symbol_id");
    if (!a.length) return fail(NFEC_EINVAL, "rx_place: null length");
    if (!a.received) return fail(NFEC_EINVAL, "rx_place: null received mask");
    if ((uint64_t)a.mask_stride * 32u < (uint64_t)a.k + a.m)
        return fail(NFEC_EINVAL, "rx_place: mask_stride smaller than (k + m + 31) / 32");
    if ((reinterpret_cast<uintptr_t>(a.base) | a.block_stride | a.seg_stride) & 7)
        return fail(NFEC_EINVAL, "rx_place: blocks, seg_stride and block_stride must be multiples of 8 bytes");
    if (a.seg_stride < a.vec) return fail(NFEC_EINVAL, "rx_place: seg_stride < vector_size");
    // enough waves to fill the chip many times over, few enough that the stats see thousands of
    // atomics, not one per segment
    constexpr uint32_t kMaxGroups = 8192;
    const uint32_t grid = std::min<uint32_t>((a.count + 3u) / 4u, kMaxGroups);
    hipLaunchKernelGGL(rx_place_kernel, dim3(grid), dim3(256), 0, s, a);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? NFEC_OK : hip_fail(e, "rx_place launch");
}

int launch_rx_ingest(const RxIngestArgs& a, hipStream_t s)
{
    if (a.count == 0 || a.nblocks == 0) return NFEC_OK;
    if (a.id_kind != RX_ID_BLOCK24 && a.id_kind != RX_ID_BLOCK16 && a.id_kind != RX_ID_BLOCK32_LEN)
        return fail(NFEC_EINVAL, "rx_ingest: bad fec_id / fec_m");
    if (!a.base) return fail(NFEC_EINVAL, "rx_ingest: null blocks pointer");
    if (!a.payloads) return fail(NFEC_EINVAL, "rx_ingest: null payloads");
    if (!a.offsets) return fail(NFEC_EINVAL, "rx_ingest: null offsets");
    if (!a.length) return fail(NFEC_EINVAL, "rx_ingest: null length");
    if (!a.received) return fail(NFEC_EINVAL, "rx_ingest: null received mask");
    if ((uint64_t)a.mask_stride * 32u < (uint64_t)a.k + a.m)
        return fail(NFEC_EINVAL, "rx_ingest: mask_stride smaller than (k + m + 31) / 32");
    if ((reinterpret_cast<uintptr_t>(a.base) | a.block_stride | a.seg_stride) & 7)
        return fail(NFEC_EINVAL, "rx_ingest: blocks, seg_stride and block_stride must be multiples of 8 bytes");
    if (a.seg_stride < a.vec) return fail(NFEC_EINVAL, "rx_ingest: seg_stride < vector_size");
    // the grid of rx_place
    constexpr uint32_t kMaxGroups = 8192;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(((uint64_t)a.count + 3u) / 4u, kMaxGroups);
    hipLaunchKernelGGL(rx_ingest_kernel, dim3(grid), dim3(256), 0, s, a);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? NFEC_OK : hip_fail(e, "rx_ingest launch");
}

int launch_rx_erasures(const RxErasureArgs& a, hipStream_t s)
{
    if (a.nblocks == 0) return NFEC_OK;
    if (!a.received) return fail(NFEC_EINVAL, "rx_erasures: null received mask");
    if (!a.locs && a.stride) return fail(NFEC_EINVAL, "rx_erasures: null erasure_locs");
    if (!a.counts) return fail(NFEC_EINVAL, "rx_erasures: null erasure_counts");
    if ((uint64_t)a.mask_stride * 32u < (uint64_t)a.k + a.m)
        return fail(NFEC_EINVAL, "rx_erasures: mask_stride smaller than (k + m + 31) / 32");
    hipLaunchKernelGGL(rx_erasures_kernel, dim3((a.nblocks + 3u) / 4u), dim3(256), 0, s, a);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? NFEC_OK : hip_fail(e, "rx_erasures launch");
}

}  // namespace nfec
