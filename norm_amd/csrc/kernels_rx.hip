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

#include "message_wave.hpp"
#include "rx_parse.hpp"
#include "segment_copy.hpp"

namespace nfec {

namespace {

// One segment by one wave: lane L takes pieces L, L + 64, ... of the slot (segment_copy.hpp, the
// gather rule).  The payload's misalignment and the slot's are the same for every piece, so the
// rule's branches are uniform, the dword pick among them.
__device__ __forceinline__ void place_segment(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, uint32_t len,
                                              uint32_t vec, uint32_t lane)
{
    const uint32_t pieces = gather_pieces(vec);
    for (uint32_t p = lane; p < pieces; p += 64) gather_piece(dst, src, len, vec, p, PickUniform());
}

// One wave per segment (message_wave.hpp): the next segment's descriptor is requested before this
// one's claim and copy; stats: placed, duplicate, rejected.
__global__ __launch_bounds__(256) void rx_place_kernel(RxPlaceArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = uniform(blockIdx.x * 4u + (threadIdx.x >> 6));
    const uint32_t nwaves = gridDim.x * 4u;
    uint32_t n_placed = 0, n_dup = 0, n_rej = 0;
    Descriptor next;
    if (wave < a.count) next.request(a, wave);
    for (uint64_t i = wave; i < a.count; i += nwaves) {
        const Descriptor d = next.taken();
        if (i + nwaves < a.count) next.request(a, i + nwaves);
        if (d.len > a.batch.vec || !slot_num_data(a.batch, d.b, d.s)) {
            ++n_rej;
            continue;
        }
        if (claim_slot(a.received, a.mask_stride, d.b, d.s, lane)) {
            ++n_dup;
            continue;
        }
        ++n_placed;
        place_segment(slot_address(a.batch, d.b, d.s), a.payloads + d.off, d.len, a.batch.vec, lane);
    }
    flush_stats(a.stats, lane, n_placed, n_dup, n_rej);
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
// uniform branch (res is wave-uniform), alignbyte funnels the bytes, and the result goes to
// scalar registers.  A word past the ID's length may hold anything; rx_id_decode does not read it.
__device__ __forceinline__ void id_words(const IdChunks& c, uint32_t res, uint32_t& w0, uint32_t& w1)
{
    const uint32_t dsh = res >> 2, bsh = res & 3u;
    uint32_t e0, e1, e2;
    switch (dsh) {
    case 0: e0 = c.q0[0], e1 = c.q0[1], e2 = c.q0[2]; break;
    case 1: e0 = c.q0[1], e1 = c.q0[2], e2 = c.q0[3]; break;
    case 2: e0 = c.q0[2], e1 = c.q0[3], e2 = c.q1[0]; break;
    default: e0 = c.q0[3], e1 = c.q1[0], e2 = c.q1[1]; break;
    }
    w0 = uniform(alignbyte(e1, e0, bsh));
    w1 = uniform(alignbyte(e2, e1, bsh));
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
    const uint32_t idlen = payload_id_length(a.id_kind);
    const uint64_t count = message_count(a.count, a.count_dev);
    if (wave >= count) return;
    uint32_t n_placed = 0, n_dup = 0, n_rej = 0;
    // message `wave`: its descriptor and its ID; then the next one's descriptor
    uint32_t v_len = a.length[wave];
    uint64_t v_off = a.offsets[wave];
    uint32_t len = uniform(v_len);
    uint64_t off = uniform64(v_off);
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
            n_off = uniform64(v_off);
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
            const uint32_t nd = len <= a.batch.vec ? slot_num_data(a.batch, b, s) : 0;
            if (nd && (a.id_kind != PAYLOAD_ID_BLOCK32_LEN || pid.block_len == nd)) {
                if (claim_slot(a.received, a.mask_stride, b, s, lane)) ++n_dup;
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
        if (place) place_segment(slot_address(a.batch, b, s), a.payloads + off, len, a.batch.vec, lane);
        len = n_len, off = n_off, readable = n_readable, id = n_id;
    }
    flush_stats(a.stats, lane, n_placed, n_dup, n_rej);
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
        // the lane's first entry: behind those of the lanes below it (the exclusive sum)
        const uint32_t mine = __popc(miss), upto = wave_scan(mine, lane);
        uint32_t at = pos + found + upto - mine;
        while (miss) {
            const uint32_t t = __ffs(miss) - 1u;
            if (at < stride) locs[at] = (uint16_t)((w << 5) + t);
            ++at;
            miss &= miss - 1u;
        }
        found += __shfl(upto, 63, 64);
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

// enough waves to fill the chip many times over, few enough that the stats see thousands of
// atomics, not one per message
constexpr uint32_t kMaxGroups = 8192;

// (both: the ABI entry has checked the arguments and returned for an empty batch or list)
int launch_rx_place(const RxPlaceArgs& a, hipStream_t s)
{
    const uint32_t grid = std::min<uint32_t>((a.count + 3u) / 4u, kMaxGroups);
    hipLaunchKernelGGL(rx_place_kernel, dim3(grid), dim3(256), 0, s, a);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? NFEC_OK : hip_fail(e, "rx_place launch");
}

int launch_rx_ingest(const RxIngestArgs& a, hipStream_t s)
{
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
