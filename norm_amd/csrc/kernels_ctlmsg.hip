// kernels_ctlmsg.hip -- NORM_NACK and NORM_CMD(REPAIR_ADV) messages on the device (nfec.h, "NORM_NACK
// and NORM_CMD(REPAIR_ADV) messages on the device"; ctl_msg.hpp holds the headers, the cut and the
// parse).
//
// fragment: repair-request content into NORM_NACK messages (NormSenderNode::FragmentNack, reference
//           src/common/normNode.cpp:2676-2772).  The cut is a chain: where a message ends decides
//           where the next begins.  The chain is made short instead of walked:
//             1. the request index: the hint's request boundaries cut the content into stretches; one
//                lane per stretch counts its requests, one workgroup scans the counts, one lane per
//                stretch writes the offsets (frag_walk_kernel twice, frag_scan_kernel);
//             2. next[q] for every content dword q that is a state of the walk (ctl_msg.hpp: the first
//                unit a message can begin with), closed-form per state (frag_next_kernel);
//             3. next^64 by six doublings (frag_double_kernel);
//             4. one lane walks next^64 from the first state (every 64th message), then one lane per
//                such anchor walks its 64 messages and numbers them (frag_chain_kernel);
//             5. one wave per message writes it: the header, then a contiguous run of content dwords
//                with the first and at most one more replaced (frag_write_kernel).
// adv:      one wave walks the request headers of the first message and copies it behind the header.
// ingest:   one lane per control datagram: the aligned chunks of its first 24 bytes, the class, the
//           content entry.
#include <algorithm>

#include "ctl_msg.hpp"
#include "message_wave.hpp"

namespace nfec {

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// ---- the fragmenter's workspace ----

enum { WS_STOP = 0, WS_REQUESTS = 1, WS_END = 2, WS_MESSAGES = 3, WS_HEAD_WORDS = 8 };

struct FragWorkspace {
    uint64_t* head;     // [8]: where the walk stopped (all ones: nowhere), R, the index's end, messages
    uint32_t* rows;     // [rows]: a stretch's request count, then its first request's index
    uint32_t* req;      // [req_cap]: the request index, offsets in dwords
    uint32_t* next;     // [states]: the next state's dword, kCutEnd, or kCutNoState
    uint32_t* info;     // [states]: the message's content bytes | split << 16
    uint32_t* ja;       // [states]: the doubling's two tables
    uint32_t* jb;
    uint32_t* anchor;   // [anchor_cap]: the state of message 64 a
    uint32_t* msg;      // [msg_cap]: the state of message i
    uint64_t rows_n, req_cap, states, anchor_cap, msg_cap, bytes;
};

__host__ __device__ inline FragWorkspace frag_workspace(uint8_t* base, uint64_t content_capacity, uint32_t nblocks)
{
    FragWorkspace w;
    w.rows_n = (uint64_t)nblocks + 1u;
    w.states = content_capacity / 4u + 2u;
    w.req_cap = content_capacity / 4u + nblocks + 2u;
    w.anchor_cap = w.states / 64u + 2u;
    w.msg_cap = content_capacity / 8u + 2u;
    uint64_t at = 0;
    auto take = [&](uint64_t n) {
        uint8_t* p = base + at;
        at += (n * 4u + 7u) & ~(uint64_t)7u;
        return reinterpret_cast<uint32_t*>(p);
    };
    w.head = reinterpret_cast<uint64_t*>(base);
    at = WS_HEAD_WORDS * 8u;
    w.rows = take(w.rows_n);
    w.req = take(w.req_cap);
    w.next = take(w.states);
    w.info = take(w.states);
    w.ja = take(w.states);
    w.jb = take(w.states);
    w.anchor = take(w.anchor_cap);
    w.msg = take(w.msg_cap);
    w.bytes = at;
    return w;
}

// the content's length: what the producing call left in HBM, within the buffer
__device__ __forceinline__ uint64_t content_length(uint64_t capacity, const uint64_t* __restrict__ bytes_dev)
{
    const uint64_t n = bytes_dev ? *bytes_dev : capacity;
    return n < capacity ? n : capacity;
}

// The content's dwords.  No load at or past the content's length: with a hint that does not belong
// to the content the index may hold anything, and a request's offset out of it is checked here.
struct DeviceContent {
    const uint32_t* __restrict__ words;
    uint64_t bytes;
    __device__ __forceinline__ uint32_t operator()(uint64_t off) const { return off + 4u <= bytes ? words[off >> 2] : 0u; }
};

// ---- 1. the request index ----

// Row b of the hint is a request boundary when b is 0, when block b is needing (class 1) or when
// block b - 1 is: the bytes emitted at a needing block's position begin a chain, and what follows
// them begins another.  The stretch of a boundary row runs to the next boundary; without a hint row
// 0 is the only one and its stretch the whole content.
struct Stretch {
    uint64_t start, end;
};
__device__ __forceinline__ bool hint_needing(const NackFragmentArgs& a, uint64_t b)
{
    return b < a.nblocks && a.block_start[2 * b + 1] == NACK_NEEDING;
}
__device__ __forceinline__ uint64_t hint_offset(const NackFragmentArgs& a, uint64_t b, uint64_t C)
{
    const uint64_t o = b ? a.block_start[2 * b] & ~(uint64_t)3u : 0u;
    return o < C ? o : C;
}
__device__ __forceinline__ bool stretch_of(const NackFragmentArgs& a, uint64_t b, uint64_t C, Stretch& s)
{
    s.start = s.end = 0;
    if (!a.block_start) {
        s.end = C;
        return b == 0;
    }
    const bool needing = hint_needing(a, b);
    if (!(b == 0 || needing || hint_needing(a, b - 1u))) return false;
    s.start = hint_offset(a, b, C);
    if (needing) {
        s.end = hint_offset(a, b + 1u, C);
    } else {
        uint64_t e = b + 1u;
        while (e < a.nblocks && !hint_needing(a, e)) ++e;
        s.end = e < a.nblocks ? hint_offset(a, e, C) : C;
    }
    return true;
}

// One lane per row walks its stretch's request headers.  Pass 0 counts them into rows[] and records
// where the walk stops (the smallest such offset of the call); pass 1 writes the offsets of the
// requests in front of that stop at the stretch's place in the index.
template <int PASS>
__global__ __launch_bounds__(256) void frag_walk_kernel(NackFragmentArgs a)
{
    const FragWorkspace w = frag_workspace(a.workspace, a.content_capacity, a.nblocks);
    const uint64_t b = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (b >= w.rows_n) return;
    const uint64_t C = content_length(a.content_capacity, a.content_bytes_dev);
    Stretch s;
    const bool mine = stretch_of(a, b, C, s);
    const DeviceContent load{a.content, C};
    uint32_t n = 0;
    uint64_t stop = PASS ? w.head[WS_STOP] : 0, at = PASS ? w.rows[b] : 0;
    const uint64_t R = PASS ? w.head[WS_REQUESTS] : 0;
    if (mine) {
        uint64_t off = s.start;
        while (off < s.end) {
            CutRequest q;
            if (C - off < 4u || !cut_request(load(off), C - off - 4u, a.cut.L, q)) {
                if (!PASS) atomicMin((unsigned long long*)(w.head + WS_STOP), (unsigned long long)off);
                break;
            }
            if (PASS) {
                if (off >= stop || at + n >= R) break;
                w.req[at + n] = (uint32_t)(off >> 2);
            }
            ++n;
            off += 4u + q.len;
        }
    }
    if (!PASS) w.rows[b] = n;
}

// One workgroup: the stretches' counts into the index of each one's first request.  A stretch that
// begins at or behind the stop has no request in the index; one that begins in front of it has all
// of its own (its walk ended at the stop at the latest).
__global__ __launch_bounds__(1024) void frag_scan_kernel(NackFragmentArgs a)
{
    __shared__ uint64_t part[1024];
    const FragWorkspace w = frag_workspace(a.workspace, a.content_capacity, a.nblocks);
    const uint64_t C = content_length(a.content_capacity, a.content_bytes_dev);
    const uint64_t stop = w.head[WS_STOP];
    const uint64_t per = (w.rows_n + 1023u) / 1024u;
    const uint64_t lo = threadIdx.x * per, hi = lo + per < w.rows_n ? lo + per : w.rows_n;
    uint64_t sum = 0;
    for (uint64_t b = lo; b < hi; ++b) {
        const uint64_t start = a.block_start ? hint_offset(a, b, C) : 0u;
        const uint32_t n = start < stop ? w.rows[b] : 0u;
        w.rows[b] = n;
        sum += n;
    }
    part[threadIdx.x] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {
        const uint64_t up = threadIdx.x >= d ? part[threadIdx.x - d] : 0u;
        __syncthreads();
        part[threadIdx.x] += up;
        __syncthreads();
    }
    uint64_t at = part[threadIdx.x] - sum;
    for (uint64_t b = lo; b < hi; ++b) {
        const uint32_t n = w.rows[b];
        w.rows[b] = (uint32_t)(at < w.req_cap ? at : w.req_cap);
        at += n;
    }
    if (threadIdx.x == 1023) {
        const uint64_t total = part[1023];
        w.head[WS_REQUESTS] = total < w.req_cap ? total : w.req_cap;
        w.head[WS_END] = stop != ~(uint64_t)0 ? stop : C;
    }
}

__device__ __forceinline__ CutIndex frag_index(const FragWorkspace& w)
{
    CutIndex x;
    x.req = w.req, x.R = (uint32_t)w.head[WS_REQUESTS], x.end = w.head[WS_END];
    return x;
}

// ---- 2. the next state of every state ----

// One lane per content dword q in [0, end / 4]: the state at 4 q, if it is one (the first unit of a
// request, or a later one; for a request without items the offset behind its header).
__global__ __launch_bounds__(256) void frag_next_kernel(NackFragmentArgs a)
{
    const FragWorkspace w = frag_workspace(a.workspace, a.content_capacity, a.nblocks);
    const CutIndex x = frag_index(w);
    const uint64_t q = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (q > x.end / 4u || q >= w.states) return;
    uint32_t nx = kCutNoState, info = 0;
    const uint64_t pos = q * 4u;
    if (x.R && pos >= 4u) {
        const DeviceContent load{a.content, content_length(a.content_capacity, a.content_bytes_dev)};
        const uint32_t r = cut_owner(x, pos);
        const uint64_t off_r = x.off(r);
        if (pos >= off_r + 4u) {
            CutRequest rq;
            cut_request(load(off_r), ~(uint64_t)0, a.cut.L, rq);
            const uint64_t d = pos - off_r - 4u;
            if (rq.len ? d < rq.len && d % rq.unit == 0 : d == 0) {
                const CutMessage m = cut_message(a.cut, x, r, pos, load);
                nx = m.next == kCutDone || m.next > x.end ? kCutEnd : (uint32_t)(m.next >> 2);
                info = (m.length & 0xffffu) | (m.split << 16);
            }
        }
    }
    w.next[q] = nx;
    w.info[q] = info;
}

// ---- 3. next^2 of a table ----
__global__ __launch_bounds__(256) void frag_double_kernel(NackFragmentArgs a, int from, int to)
{
    const FragWorkspace w = frag_workspace(a.workspace, a.content_capacity, a.nblocks);
    const uint32_t* __restrict__ src = from == 0 ? w.next : from == 1 ? w.ja : w.jb;
    uint32_t* __restrict__ dst = to == 1 ? w.ja : w.jb;
    const uint64_t last = w.head[WS_END] / 4u;
    const uint64_t q = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (q > last || q >= w.states) return;
    const uint32_t v = src[q];
    dst[q] = v >= kCutNoState ? v : v <= last ? src[v] : kCutEnd;
}

// ---- 4. the messages' numbers ----

// One workgroup.  Lane 0 walks next^64 from the first state: anchor[a] is the state of message 64 a.
// Then one lane per anchor walks next over its 64 messages: the state of message i into msg[i], the
// messages, their content bytes and the splits into the totals.
__global__ __launch_bounds__(1024) void frag_chain_kernel(NackFragmentArgs a)
{
    __shared__ uint32_t n_anchor;
    __shared__ unsigned long long sums[3];
    const FragWorkspace w = frag_workspace(a.workspace, a.content_capacity, a.nblocks);
    const uint64_t last = w.head[WS_END] / 4u;
    const uint64_t R = w.head[WS_REQUESTS];
    if (threadIdx.x == 0) {
        uint32_t n = 0;
        uint32_t q = R ? 1u : kCutEnd;
        while (q < kCutNoState && q <= last && n < w.anchor_cap) {
            w.anchor[n++] = q;
            q = w.jb[q];
        }
        n_anchor = n;
        sums[0] = sums[1] = sums[2] = 0;
    }
    __syncthreads();
    const uint64_t cap = a.capacity < w.msg_cap ? a.capacity : w.msg_cap;
    unsigned long long count = 0, bytes = 0, splits = 0;
    for (uint32_t an = threadIdx.x; an < n_anchor; an += 1024u) {
        uint32_t q = w.anchor[an];
        for (uint32_t s = 0; s < 64u && q < kCutNoState && q <= last; ++s) {
            const uint64_t i = (uint64_t)an * 64u + s;
            if (i < cap) w.msg[i] = q;
            const uint32_t info = w.info[q];
            ++count, bytes += info & 0xffffu, splits += info >> 16;
            q = w.next[q];
        }
    }
    if (count) atomicAdd(&sums[0], count), atomicAdd(&sums[1], bytes), atomicAdd(&sums[2], splits);
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint64_t C = content_length(a.content_capacity, a.content_bytes_dev);
        const uint64_t given = a.content_bytes_dev ? *a.content_bytes_dev : a.content_capacity;
        w.head[WS_MESSAGES] = sums[0];
        a.totals[0] = sums[0], a.totals[1] = sums[1], a.totals[2] = R, a.totals[3] = sums[2];
        a.totals[4] = w.head[WS_END];
        a.totals[5] = w.head[WS_END] != C || given > a.content_capacity;
    }
}

// ---- 5. the messages ----

__device__ __forceinline__ uint32_t header_word(const CtlHeaderFixed& f, uint32_t j)
{
    uint32_t v = 0;
#pragma unroll
    for (uint32_t t = 0; t < kCtlHeaderWords; ++t) v = j == t ? f.w[t] : v;
    return v;
}

// the content of message m behind a header of hw words at dst: dword copies, the head and the tail
// word replaced; no load at or past C
__device__ __forceinline__ void write_content(uint32_t* __restrict__ dst, const CutMessage& m, uint32_t length,
                                              const uint32_t* __restrict__ content, uint64_t C, uint32_t lane)
{
    for (uint32_t d = lane; d < length / 4u; d += 64u) {
        const uint64_t off = m.src + 4u * (uint64_t)d;
        uint32_t v = off + 4u <= C ? content[off >> 2] : 0u;
        if (d == 0) v = m.head;
        if (m.tail_at && 4u * d == m.tail_at) v = m.tail;
        dst[d] = v;
    }
}

// One wave per message, four waves a workgroup.  The message is recomputed from its state (every lane
// the same loads: one request each), then written by dword stores.
__global__ __launch_bounds__(256) void frag_write_kernel(NackFragmentArgs a)
{
    const FragWorkspace w = frag_workspace(a.workspace, a.content_capacity, a.nblocks);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = uniform(blockIdx.x * 4u + (threadIdx.x >> 6));
    const uint32_t nwaves = gridDim.x * 4u;
    const CutIndex x = frag_index(w);
    const uint64_t C = content_length(a.content_capacity, a.content_bytes_dev);
    uint64_t count = w.head[WS_MESSAGES];
    if (count > a.capacity) count = a.capacity;
    if (count > w.msg_cap) count = w.msg_cap;
    const DeviceContent load{a.content, C};
    const uint32_t H = a.header.hdr_bytes;
    for (uint64_t i = wave; i < count; i += nwaves) {
        const uint64_t pos = (uint64_t)uniform(w.msg[i]) * 4u;
        const uint32_t r = cut_owner(x, pos);
        const CutMessage m = cut_message(a.cut, x, r, pos, load);
        const uint32_t length = m.length < a.cut.S ? m.length & ~3u : a.cut.S;
        uint32_t* __restrict__ dst = reinterpret_cast<uint32_t*>(a.wire + i * a.pitch);
        if (lane < H / 4u)
            dst[lane] = lane == 0 ? ctl_header_word0(kNackVersionType, H, nack_sequence(a.header, i)) : header_word(a.header, lane);
        write_content(dst + H / 4u, m, length, a.content, C, lane);
        if (lane == 0) {
            if (a.msg_offsets_out) a.msg_offsets_out[i] = i * a.pitch;
            if (a.msg_length_out) a.msg_length_out[i] = (uint16_t)(H + length);
        }
    }
}

// ---- the advertisement ----

// One wave: the walk over the first message's request headers (every lane the same), then the copy.
__global__ __launch_bounds__(64) void adv_message_kernel(AdvMessageArgs a)
{
    const uint32_t lane = threadIdx.x;
    const uint64_t C = content_length(a.content_capacity, a.content_bytes_dev);
    const DeviceContent load{a.content, C};
    const CutMessage m = cut_first_message(a.cut, C, load);
    const uint32_t H = a.header.hdr_bytes;
    const uint32_t limit = m.used != C;
    if (m.length) {
        if (lane < H / 4u) a.wire[lane] = lane == 3 ? adv_flags_word(limit) : header_word(a.header, lane);
        write_content(a.wire + H / 4u, m, m.length, a.content, C, lane);
    }
    if (lane == 0) {
        a.msg_length_out[0] = (uint16_t)(m.length ? H + m.length : 0u);
        a.totals[0] = m.length, a.totals[1] = C - m.used, a.totals[2] = m.length ? limit : C != 0;
    }
}

// ---- the intake ----

// The datagram's first kCtlParseWords words out of its aligned chunks (ctl_msg.hpp: the only place
// their addresses are computed).  A word past the loaded bytes may hold anything; ctl_parse does not
// read it.
__device__ __forceinline__ void ctl_head_words(const uint8_t* __restrict__ dgram, uint32_t length, uint32_t (&h)[kCtlParseWords])
{
    // (the pointer is stepped back, not rebuilt from an integer: it stays a global-memory pointer)
    const uint64_t at = reinterpret_cast<uintptr_t>(dgram);
    const u32x4* __restrict__ chunk = reinterpret_cast<const u32x4*>(dgram - (at - ctl_chunk_offset(at)));
    const uint32_t n = ctl_chunk_count(at, length);
    u32x4 c[3];
#pragma unroll
    for (uint32_t j = 0; j < 3; ++j) {
        c[j] = u32x4{0u, 0u, 0u, 0u};
        if (j < n) c[j] = chunk[j];
    }
    const uint32_t res = (uint32_t)(at & 15u), dsh = res >> 2, bsh = (res & 3u) * 8u;
    uint32_t e[kCtlParseWords + 1];
    switch (dsh) {
    case 0:
#pragma unroll
        for (uint32_t j = 0; j <= kCtlParseWords; ++j) e[j] = c[j >> 2][j & 3u];
        break;
    case 1:
#pragma unroll
        for (uint32_t j = 0; j <= kCtlParseWords; ++j) e[j] = c[(j + 1u) >> 2][(j + 1u) & 3u];
        break;
    case 2:
#pragma unroll
        for (uint32_t j = 0; j <= kCtlParseWords; ++j) e[j] = c[(j + 2u) >> 2][(j + 2u) & 3u];
        break;
    default:
#pragma unroll
        for (uint32_t j = 0; j <= kCtlParseWords; ++j) e[j] = c[(j + 3u) >> 2][(j + 3u) & 3u];
        break;
    }
#pragma unroll
    for (uint32_t j = 0; j < kCtlParseWords; ++j) h[j] = bsh ? (e[j] >> bsh) | (e[j + 1] << (32u - bsh)) : e[j];
}

// One lane per datagram; a wave counts its datagrams per class by ballots and adds them to stats
// once, at its end.
__global__ __launch_bounds__(256) void ctl_ingest_kernel(CtlIngestArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t count = message_count(a.count, a.count_dev);
    const uint64_t step = (uint64_t)gridDim.x * 256u;
    uint32_t n_class[CTL_CLASSES] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    // (whole waves stay in the loop: the ballots count the lanes that hold a datagram)
    for (uint64_t base = (uint64_t)blockIdx.x * 256u + (threadIdx.x & ~63u); base < count; base += step) {
        const uint64_t i = base + lane;
        uint32_t cls = CTL_CLASSES;
        if (i < count) {
            const uint64_t off = a.offsets[i];
            const uint32_t len = a.length[i];
            CtlParse p;
            p.cls = CTL_UNREADABLE, p.extended = 0, p.hdr_bytes = 0, p.source_id = 0, p.sec = p.usec = 0;
            if (ctl_readable(off, len, a.payload_bytes)) {
                uint32_t h[kCtlParseWords];
                ctl_head_words(a.payloads + off, len, h);
                p = ctl_parse(h, len, a.filter);
            }
            cls = p.cls;
            if (a.class_out) a.class_out[i] = (uint8_t)(p.cls | (p.extended ? CTL_EXTENDED : 0u));
            a.content_offset_out[i] = p.hdr_bytes ? off + p.hdr_bytes : 0u;
            a.content_length_out[i] = (uint16_t)(p.hdr_bytes ? len - p.hdr_bytes : 0u);
            if (a.source_id_out) a.source_id_out[i] = p.source_id;
            if (a.grtt_response_out) a.grtt_response_out[2 * i] = p.sec, a.grtt_response_out[2 * i + 1] = p.usec;
        }
#pragma unroll
        for (uint32_t c = 0; c < CTL_CLASSES; ++c) n_class[c] += (uint32_t)__popcll(__ballot(cls == c));
    }
    if (a.stats && lane == 0) {
#pragma unroll
        for (uint32_t c = 0; c < CTL_CLASSES; ++c)
            if (n_class[c]) atomicAdd(a.stats + c, n_class[c]);
    }
}

}  // namespace

uint64_t nack_fragment_workspace(uint64_t content_capacity, uint32_t nblocks)
{
    return frag_workspace(nullptr, content_capacity, nblocks).bytes;
}

// (all three: the ABI entry has checked the arguments)
int launch_nack_fragment(const NackFragmentArgs& a, hipStream_t s)
{
    const FragWorkspace w = frag_workspace(a.workspace, a.content_capacity, a.nblocks);
    hipError_t e = hipMemsetAsync(w.head, 0xff, 8, s);
    if (e != hipSuccess) return hip_fail(e, "nack_fragment workspace");
    const uint32_t row_groups = (uint32_t)((w.rows_n + 255u) / 256u);
    const uint32_t state_groups = (uint32_t)((w.states + 255u) / 256u);
    hipLaunchKernelGGL(frag_walk_kernel<0>, dim3(row_groups), dim3(256), 0, s, a);
    hipLaunchKernelGGL(frag_scan_kernel, dim3(1), dim3(1024), 0, s, a);
    hipLaunchKernelGGL(frag_walk_kernel<1>, dim3(row_groups), dim3(256), 0, s, a);
    hipLaunchKernelGGL(frag_next_kernel, dim3(state_groups), dim3(256), 0, s, a);
    // next -> ja = next^2 -> jb = ^4 -> ja = ^8 -> jb = ^16 -> ja = ^32 -> jb = ^64
    for (int round = 0; round < 6; ++round)
        hipLaunchKernelGGL(frag_double_kernel, dim3(state_groups), dim3(256), 0, s, a, round == 0 ? 0 : round & 1 ? 1 : 2,
                           round & 1 ? 2 : 1);
    hipLaunchKernelGGL(frag_chain_kernel, dim3(1), dim3(1024), 0, s, a);
    const uint64_t most = std::min<uint64_t>(a.capacity, w.msg_cap);
    if (most) {
        const uint32_t grid = (uint32_t)std::min<uint64_t>((most + 3u) / 4u, 2048u);
        hipLaunchKernelGGL(frag_write_kernel, dim3(grid), dim3(256), 0, s, a);
    }
    e = hipGetLastError();
    return e == hipSuccess ? NFEC_OK : hip_fail(e, "nack_fragment launch");
}

int launch_adv_message(const AdvMessageArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(adv_message_kernel, dim3(1), dim3(64), 0, s, a);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? NFEC_OK : hip_fail(e, "adv_message launch");
}

int launch_ctl_ingest(const CtlIngestArgs& a, hipStream_t s)
{
    const uint32_t grid = (uint32_t)std::min<uint64_t>(((uint64_t)a.count + 255u) / 256u, 1024u);
    hipLaunchKernelGGL(ctl_ingest_kernel, dim3(grid), dim3(256), 0, s, a);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? NFEC_OK : hip_fail(e, "ctl_ingest launch");
}

}  // namespace nfec
