// kernels_datamsg.hip -- whole NORM_DATA messages on the device (nfec.h, "NORM_DATA messages on the
// device"; data_msg.hpp holds the header's layout and the parse).
//
// emit:   tx_emit_kernel (kernels_tx.hip) with the message header, the FEC payload ID and the header
//         extension in front of the payload instead of the ID alone: what NormObject::NextSenderMsg
//         and NormSession::SendMessage put there (reference src/common/normObject.cpp:1808-1857,
//         :2078; src/common/normSession.cpp:4923-4924, :5013).
// ingest: rx_ingest_kernel (kernels_rx.hip) on raw datagrams: NormMsg::InitFromBuffer's validation
//         (src/common/normMessage.cpp:17-92), the sender / code / object filter, the ID at byte 16
//         and the payload at 4 * hdr_len, then the claim and the copy.
#include <algorithm>

#include "data_msg.hpp"
#include "message_wave.hpp"
#include "rx_parse.hpp"
#include "segment_copy.hpp"

namespace nfec {

namespace {

// ---- emission ----

// One wave per entry, as tx_emit_kernel: the next entry's descriptor is requested before this one
// is copied.  The header is formed in scalar registers from the call's constants, the entry's index
// and its payload ID, brought to the destination's residue once (scatter_header_image) and stored
// by the lanes whose pieces it reaches (the first four at the most) with the scatter rule's
// partial-piece stores: the wire buffer is never read.  stats: emitted, rejected.
__global__ __launch_bounds__(256) void tx_emit_data_kernel(TxEmitDataArgs ad)
{
    const TxEmitArgs& a = ad.tx;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = uniform(blockIdx.x * 4u + (threadIdx.x >> 6));
    const uint32_t nwaves = gridDim.x * 4u;
    const uint32_t H = ad.header.hdr_bytes;
    const uint64_t count = message_count(a.count, a.count_dev);
    uint32_t n_emitted = 0, n_rej = 0;
    Descriptor next;
    if (wave < count) next.request(a, wave);
    for (uint64_t i = wave; i < count; i += nwaves) {
        const Descriptor d = next.taken();
        if (i + nwaves < count) next.request(a, i + nwaves);
        const uint32_t nd = d.len <= a.batch.vec && d.len + H <= 65535u && rx_readable(d.off, d.len, H, a.payload_bytes)
                                ? slot_num_data(a.batch, d.b, d.s)
                                : 0;
        if (lane == 0) {
            if (ad.msg_offsets_out) ad.msg_offsets_out[i] = nd ? d.off - H : 0u;
            if (ad.msg_length_out) ad.msg_length_out[i] = (uint16_t)(nd ? d.len + H : 0u);
        }
        if (!nd) {
            ++n_rej;
            continue;
        }
        ++n_emitted;
        if (a.pending && lane == 0)
            atomicAnd(a.pending + (uint64_t)d.b * a.mask_stride + (d.s >> 5), ~(1u << (d.s & 31u)));
        uint8_t* dst = a.payloads + (d.off - H);
        uint32_t hdr[kDataHeaderWords], img[16];
        data_header_words(ad.header, (uint32_t)i, payload_id(ad.header.id_kind, a.first_block_id + d.b, d.s, nd), hdr);
        scatter_header_image(hdr, (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u), img);
        const uint8_t* slot = slot_address(a.batch, d.b, d.s);
        const uint32_t pieces = scatter_pieces(dst, H + d.len);
        for (uint32_t p = lane; p < pieces; p += 64) scatter_piece_header(dst, slot, d.len, img, H, p);
    }
    flush_stats(a.stats, lane, n_emitted, n_rej);
}

// ---- intake ----

// One segment by one wave (kernels_rx.hip's place_segment: the gather rule, uniform dword pick).
__device__ __forceinline__ void place_payload(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, uint32_t len,
                                              uint32_t vec, uint32_t lane)
{
    const uint32_t pieces = gather_pieces(vec);
    for (uint32_t p = lane; p < pieces; p += 64) gather_piece(dst, src, len, vec, p, PickUniform());
}

// The chunks of a datagram's first min(length, kParseBytes) bytes (data_msg.hpp: the only place
// their addresses are computed).  Every lane reads the same address: one request per chunk.
struct HeadChunks {
    u32x4 q[3];
};
__device__ __forceinline__ HeadChunks load_head(const uint8_t* __restrict__ dgram, uint32_t length)
{
    // (the pointer is stepped back, not rebuilt from an integer: it stays a global-memory pointer)
    const uint64_t at = reinterpret_cast<uintptr_t>(dgram);
    const u32x4* __restrict__ chunk = reinterpret_cast<const u32x4*>(dgram - (at - data_chunk_offset(at)));
    const uint32_t n = data_chunk_count(at, length);
    HeadChunks c;
#pragma unroll
    for (uint32_t j = 0; j < 3; ++j) {
        c.q[j] = u32x4{0u, 0u, 0u, 0u};
        if (j < n) c.q[j] = chunk[j];
    }
    return c;
}

// The datagram's first kParseWords words out of the chunks, into scalar registers: the dword pick is
// a uniform branch (res is), alignbyte funnels the bytes.  A word past the loaded bytes may hold
// anything; data_parse does not read it.
__device__ __forceinline__ void head_words(const HeadChunks& c, uint32_t res, uint32_t (&h)[kParseWords])
{
    const uint32_t dsh = res >> 2, bsh = res & 3u;
    uint32_t e[kParseWords + 1];
    switch (dsh) {
    case 0:
#pragma unroll
        for (uint32_t j = 0; j <= kParseWords; ++j) e[j] = c.q[j >> 2][j & 3u];
        break;
    case 1:
#pragma unroll
        for (uint32_t j = 0; j <= kParseWords; ++j) e[j] = c.q[(j + 1u) >> 2][(j + 1u) & 3u];
        break;
    case 2:
#pragma unroll
        for (uint32_t j = 0; j <= kParseWords; ++j) e[j] = c.q[(j + 2u) >> 2][(j + 2u) & 3u];
        break;
    default:
#pragma unroll
        for (uint32_t j = 0; j <= kParseWords; ++j) e[j] = c.q[(j + 3u) >> 2][(j + 3u) & 3u];
        break;
    }
#pragma unroll
    for (uint32_t j = 0; j < kParseWords; ++j) h[j] = uniform(alignbyte(e[j + 1], e[j], bsh));
}

// rx_ingest_kernel's shape and pipeline: datagram i + 1's header chunks and datagram i + 2's
// (offset, length) are requested ahead of datagram i's claim and arrive with its answer.  The
// payload's address depends on a loaded byte (hdr_len); the parse has it in a scalar register
// before the claim is sent, so the copy waits for the claim's answer alone, as in rx_ingest_kernel.
// A datagram that is not placed costs its header chunks alone.  The wave counts its datagrams per
// class in scalar registers and adds them to stats once; the first datagram with an FTI that the
// wave meets is its smallest (i ascends), so the wave sends one atomicMin.
__global__ __launch_bounds__(256) void rx_ingest_data_kernel(RxIngestDataArgs ad)
{
    const RxIngestArgs& a = ad.rx;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = uniform(blockIdx.x * 4u + (threadIdx.x >> 6));
    const uint32_t nwaves = gridDim.x * 4u;
    const uint64_t count = message_count(a.count, a.count_dev);
    if (wave >= count) return;
    uint32_t n_class[DGRAM_CLASSES] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t first_fti = ~(uint64_t)0;
    // datagram `wave`: its descriptor and its header; then the next one's descriptor
    uint32_t v_len = a.length[wave];
    uint64_t v_off = a.offsets[wave];
    uint32_t len = uniform(v_len);
    uint64_t off = uniform64(v_off);
    bool readable = data_readable(off, len, a.payload_bytes);
    HeadChunks head{};
    if (readable) head = load_head(a.payloads + off, len);
    if ((uint64_t)wave + nwaves < count) v_len = a.length[wave + nwaves], v_off = a.offsets[wave + nwaves];
    for (uint64_t i = wave; i < count; i += nwaves) {
        const uint64_t nxt = i + nwaves;
        uint32_t n_len = 0;
        uint64_t n_off = 0;
        bool n_readable = false;
        HeadChunks n_head{};
        if (nxt < count) {
            n_len = uniform(v_len);
            n_off = uniform64(v_off);
            n_readable = data_readable(n_off, n_len, a.payload_bytes);
            if (n_readable) n_head = load_head(a.payloads + n_off, n_len);
            if (nxt + nwaves < count) v_len = a.length[nxt + nwaves], v_off = a.offsets[nxt + nwaves];
        }
        // parse and claim datagram i: its header was requested an iteration ago
        uint32_t cls = DGRAM_UNREADABLE, b = 0xffffffffu, s = 0xffffu, seq = 0, plen = 0;
        uint64_t poff = 0;
        if (readable) {
            uint32_t h[kParseWords];
            head_words(head, (uint32_t)(reinterpret_cast<uintptr_t>(a.payloads + off) & 15u), h);
            const DataParse p = data_parse(h, len, ad.filter, a.first_block_id);
            cls = p.cls, seq = p.sequence;
            if (cls == DGRAM_PARSED) {
                b = p.id.block, s = p.id.symbol;
                plen = len - p.hdr_bytes, poff = off + p.hdr_bytes;
                if (p.fti && first_fti == ~(uint64_t)0) first_fti = i;
                const uint32_t nd = plen <= a.batch.vec ? slot_num_data(a.batch, b, s) : 0;
                if (nd && (ad.filter.id_kind != PAYLOAD_ID_BLOCK32_LEN || p.id.block_len == nd))
                    cls = claim_slot(a.received, a.mask_stride, b, s, lane) ? DGRAM_DUPLICATE : DGRAM_PLACED;
                else
                    cls = DGRAM_REJECTED;
            }
        }
#pragma unroll
        for (uint32_t c = 0; c < DGRAM_CLASSES; ++c) n_class[c] += cls == c ? 1u : 0u;
        if (lane == 0) {
            if (ad.class_out) ad.class_out[i] = (uint8_t)cls;
            if (ad.sequence_out && readable) ad.sequence_out[i] = (uint16_t)seq;
            if (a.block_index_out) a.block_index_out[i] = b;
            if (a.symbol_id_out) a.symbol_id_out[i] = (uint16_t)s;
        }
        if (cls == DGRAM_PLACED) place_payload(slot_address(a.batch, b, s), a.payloads + poff, plen, a.batch.vec, lane);
        len = n_len, off = n_off, readable = n_readable, head = n_head;
    }
    if (lane == 0) {
        if (a.stats) {
#pragma unroll
            for (uint32_t c = 0; c < DGRAM_CLASSES; ++c)
                if (n_class[c]) atomicAdd(a.stats + c, n_class[c]);
        }
        if (ad.totals && first_fti != ~(uint64_t)0) atomicMin((unsigned long long*)ad.totals, (unsigned long long)first_fti);
    }
}

}  // namespace

// (kernels_rx.hip's bound: enough waves to fill the chip many times over, few enough that the stats
// see thousands of atomics, not one per message)
constexpr uint32_t kMaxGroups = 8192;

// (both: the ABI entry has checked the arguments and returned for an empty batch or list)
int launch_tx_emit_data(const TxEmitDataArgs& a, hipStream_t s)
{
    const uint32_t grid = (uint32_t)std::min<uint64_t>(((uint64_t)a.tx.count + 3u) / 4u, kMaxGroups);
    hipLaunchKernelGGL(tx_emit_data_kernel, dim3(grid), dim3(256), 0, s, a);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? NFEC_OK : hip_fail(e, "tx_emit_data launch");
}

int launch_rx_ingest_data(const RxIngestDataArgs& a, hipStream_t s)
{
    const uint32_t grid = (uint32_t)std::min<uint64_t>(((uint64_t)a.rx.count + 3u) / 4u, kMaxGroups);
    hipLaunchKernelGGL(rx_ingest_data_kernel, dim3(grid), dim3(256), 0, s, a);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? NFEC_OK : hip_fail(e, "rx_ingest_data launch");
}

}  // namespace nfec
