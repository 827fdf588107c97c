// kernels_stream.hip -- stream objects on the device (nfec.h, "stream objects on the device").
//
// frame:  NormStreamObject::Write's loop (reference src/common/normObject.cpp:4166-4210) over a
//         table of writes, in the closed form of stream_layout.hpp: which bytes of the stream make
//         which segment, and each segment's header fields.
// pack:   the segments into the source slots of their blocks: the 8-byte stream payload header
//         (include/normMessage.h:1145-1196), the stream bytes from any alignment, the zero pad of
//         CalculateBlockParity (:2203-2229); Terminate's control segment (:3904-3995) on request.
// unpack: what NormStreamObject::ReadPrivate (:3700-3860) takes out of a segment, for every
//         selected source slot: the header decides where the slot's bytes go in the window.
//
// Pack and unpack are obj_read_kernel / obj_write_kernel (kernels_obj.hip) with the source and
// the length of a segment read from a table / from the slot's header instead of computed: a
// workgroup of 256 lanes takes a run of up to 64 consecutive slots of one block, its first wave
// fetches and checks the run's 64 descriptors into LDS, and all lanes stride over the run's
// (segment, 16-byte piece) pairs as one flat index.  The copies are segment_copy.hpp's two rules
// on the slot's bytes from 8 on: a slot is 8-byte aligned, so slot + 8 is, which is all either
// rule asks of it.
#include <algorithm>

#include "message_wave.hpp"
#include "segment_copy.hpp"
#include "stream_layout.hpp"

namespace nfec {

namespace {

constexpr uint32_t kRun = 64;         // slots per work item
constexpr uint32_t kMaxGroups = 8192; // as the object kernels cap their grid
constexpr uint32_t kSkip = ~0u;       // pack: a slot of the run the call does not fill

// the flat index's shape (kernels_obj.hip): runs per block, pieces per segment, the multiply that
// divides a lane's first index by them and the step of 256 indices
struct StreamShape {
    uint32_t runs = 0, pieces = 0, magic = 0, step_sl = 0, step_p = 0;
    uint32_t b0 = 0, nb = 0;  // the batch blocks the call can touch: [b0, b0 + nb)
};

// work items are (block, run) pairs, item = block * runs + run; workgroup g takes g, g + gridDim.x, ...
struct ItemWalk {
    uint32_t i, r, step_i, step_r, runs;
    __device__ __forceinline__ ItemWalk(uint32_t runs_) : runs(runs_)
    {
        i = blockIdx.x / runs, r = blockIdx.x % runs;
        step_i = gridDim.x / runs, step_r = gridDim.x % runs;
    }
    __device__ __forceinline__ void next()
    {
        i += step_i, r += step_r;
        if (r >= runs) r -= runs, ++i;
    }
};

// a lane's flat index tid, tid + 256, ... as (segment of the run, piece): one multiply, then additions
struct PieceWalk {
    uint32_t sl, p;
    __device__ __forceinline__ PieceWalk(uint32_t tid, const StreamShape& sh)
    {
        sl = div_by_magic32(tid, sh.magic), p = tid - sl * sh.pieces;
    }
    __device__ __forceinline__ void next(const StreamShape& sh)
    {
        sl += sh.step_sl, p += sh.step_p;
        if (p >= sh.pieces) p -= sh.pieces, ++sl;
    }
};

// ---- pack ----

__global__ __launch_bounds__(256) void stream_pack_kernel(StreamPackArgs a, StreamShape sh)
{
    __shared__ uint64_t s_src[kRun];  // the segment's first byte in the stream bytes
    __shared__ uint32_t s_len[kRun];  // its length, or kSkip
    const uint32_t tid = threadIdx.x;
    const uint64_t entries = message_count(a.count, a.count_dev);
    const uint64_t lo = a.first_slot, hi = lo + entries + a.end;  // the stream slots the call fills
    uint32_t n_ok = 0, n_rej = 0;
    for (ItemWalk it(sh.runs); it.i < sh.nb; it.next()) {
        const uint32_t b = sh.b0 + it.i, s0 = it.r * kRun;
        const uint64_t blk0 = (uint64_t)b * a.batch.k;
        if (hi <= blk0 || lo >= blk0 + a.batch.k) continue;  // (none of the block's slots: the same for every lane)
        if (a.num_data_out && it.r == 0 && tid == 0)
            a.num_data_out[b] = (uint16_t)min((uint64_t)a.batch.k, hi - blk0);
        const uint32_t nseg = min(kRun, a.batch.k - s0);
        const uint64_t q0 = blk0 + s0;
        if (hi <= q0 || lo >= q0 + nseg) continue;
        uint8_t* __restrict__ slot0 = a.batch.base + (uint64_t)b * a.batch.block_stride + (uint64_t)s0 * a.batch.seg_stride;
        __syncthreads();  // (the run before is copied)
        if (tid < kRun) {
            // the first wave: one descriptor per lane, checked; the header is the lane's one store
            const uint64_t q = q0 + tid;
            uint64_t start = 0;
            uint32_t len = kSkip;
            const bool mine = tid < nseg && q >= lo && q < hi;
            bool ok = false;
            if (mine) {
                const uint64_t i = q - lo;
                uint32_t ms = 0;
                if (i < entries) {
                    start = a.seg_start[i], len = a.seg_len[i], ms = a.seg_msg_start[i];
                    ok = stream_entry_ok(start, len, a.S, a.stream_bytes);
                } else {  // Terminate's segment: behind the last entry's last byte
                    start = entries ? a.seg_start[entries - 1u] + a.seg_len[entries - 1u] : 0u;
                    len = 0, ok = true;
                }
                if (ok) {
                    uint32_t w0, w1;
                    stream_header_encode(len, ms, a.write_offset + (uint32_t)start, &w0, &w1);
                    *reinterpret_cast<u32x2*>(slot0 + (uint64_t)tid * a.batch.seg_stride) = u32x2{w0, w1};
                    if (a.seg_length_out)
                        a.seg_length_out[(uint64_t)b * a.length_stride + s0 + tid] = (uint16_t)(kStreamHeader + len);
                    if (len == 0) start = 0;  // (nothing of the stream is read)
                } else {
                    start = 0, len = kSkip;
                }
            }
            n_ok += __popcll(__ballot(mine && ok));
            n_rej += __popcll(__ballot(mine && !ok));
            s_src[tid] = start, s_len[tid] = len;
        }
        __syncthreads();
        for (PieceWalk w(tid, sh); w.sl < nseg; w.next(sh)) {
            const uint32_t len = s_len[w.sl];
            const bool skip = len == kSkip;
            const uint8_t* __restrict__ src = a.bytes + s_src[w.sl];
            // the piece's second chunk is the next lane's first where that lane holds the segment's
            // next piece (kernels_obj.hip, read_piece): every lane in the loop takes part
            const u32x4 c0 = gather_first_chunk(src, skip ? 0u : len, w.p);
            const u32x4 next_c0 = {(uint32_t)__shfl_down(c0[0], 1, 64), (uint32_t)__shfl_down(c0[1], 1, 64),
                                   (uint32_t)__shfl_down(c0[2], 1, 64), (uint32_t)__shfl_down(c0[3], 1, 64)};
            if (skip) continue;
            gather_store_piece(slot0 + (uint64_t)w.sl * a.batch.seg_stride + kStreamHeader, src, len,
                               a.batch.vec - kStreamHeader, w.p, c0, next_c0,
                               gather_second_from_next(tid & 63u, w.p, sh.pieces, len), PickPerLane());
        }
    }
    // the entries whose block the batch does not have: counted by the first workgroup
    if (blockIdx.x == 0 && tid == 0) {
        const uint64_t room = (uint64_t)a.batch.nblocks * a.batch.k;
        if (hi > max(lo, room)) n_rej += (uint32_t)(hi - max(lo, room));
    }
    if (a.stats && tid == 0) {
        if (n_ok) atomicAdd(a.stats + 0, n_ok);
        if (n_rej) atomicAdd(a.stats + 1, n_rej);
    }
}

// ---- unpack ----

__global__ __launch_bounds__(256) void stream_unpack_kernel(StreamUnpackArgs a, StreamShape sh)
{
    __shared__ uint32_t s_dst[kRun];  // where the segment goes in the window
    __shared__ uint32_t s_len[kRun];  // its length, 0: nothing to copy
    const uint32_t tid = threadIdx.x;
    uint32_t n[4] = {0u, 0u, 0u, 0u};  // delivered, not selected, control, invalid
    for (ItemWalk it(sh.runs); it.i < a.batch.nblocks; it.next()) {
        const uint32_t s0 = it.r * kRun;
        const uint32_t nseg = min(kRun, a.batch.k - s0);
        const uint8_t* __restrict__ slot0 = a.batch.base + (uint64_t)it.i * a.batch.block_stride + (uint64_t)s0 * a.batch.seg_stride;
        __syncthreads();  // (the run before is copied)
        if (tid < kRun) {
            // the run's selection (kernels_obj.hip): the two mask words of its 64 slots, or every
            // slot without a mask or in a repaired block
            uint64_t sel = ~0ull;
            if (a.received && !(a.status && a.status[it.i] > 0)) {
                const uint32_t* __restrict__ mw = a.received + (uint64_t)it.i * a.mask_stride + (s0 >> 5);
                sel = mw[0];
                if (nseg > 32) sel |= (uint64_t)mw[1] << 32;
            }
            // (a block the sender closed early has nd < k source slots: the rest are not its segments)
            const uint32_t nd = a.batch.num_data ? a.batch.num_data[it.i] : a.batch.k;
            const bool in_run = tid < nseg, picked = in_run && s0 + tid < nd && ((sel >> tid) & 1ull);
            uint32_t len = 0, ms = 0, off = 0, d = 0, verdict = 1u;
            if (picked) {
                // the header: network data, so it is judged before anything is done on its word
                const u32x2 h = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(slot0 + (uint64_t)tid * a.batch.seg_stride));
                stream_header_decode(h[0], h[1], &len, &ms, &off);
                verdict = stream_header_verdict(len, off, a.base_offset, a.S, a.window_bytes, &d);
            }
            if (in_run) {
                const uint64_t o = (uint64_t)it.i * a.out_stride + s0 + tid;
                if (a.len_out) a.len_out[o] = picked ? (uint16_t)len : (uint16_t)0xffffu;
                if (picked && a.offset_out) a.offset_out[o] = off;
                if (picked && a.msg_start_out) a.msg_start_out[o] = (uint16_t)ms;
            }
            s_dst[tid] = d, s_len[tid] = picked && verdict == STREAM_DELIVER ? len : 0u;
            n[0] += __popcll(__ballot(picked && verdict == STREAM_DELIVER));
            n[1] += __popcll(__ballot(in_run && !picked));
            n[2] += __popcll(__ballot(picked && verdict == STREAM_CONTROL));
            n[3] += __popcll(__ballot(picked && verdict == STREAM_INVALID));
        }
        __syncthreads();
        for (PieceWalk w(tid, sh); w.sl < nseg; w.next(sh)) {
            const uint32_t len = s_len[w.sl];
            if (!len) continue;
            // the aligned 16-byte piece w.p of the segment's window bytes (segment_copy.hpp, the
            // scatter rule without a payload ID; nothing where the segment has no such piece)
            scatter_piece(a.window + s_dst[w.sl], slot0 + (uint64_t)w.sl * a.batch.seg_stride + kStreamHeader, len, 0, 0, w.p);
        }
    }
    if (a.stats && tid == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (n[j]) atomicAdd(a.stats + j, n[j]);
    }
}

// ---- frame ----
//
// The six scans of stream_layout.hpp over the n + 1 elements (the carry, then the writes) by one
// workgroup of 1024 threads, in tiles of 1024 with a running carry as tx_scan_kernel walks its
// rows: a forward pass (B, LN, LE, then G, which needs the ends), a backward pass (NF, NM and the
// new carry's message start, then each element's segment count) and the exclusive scan of the
// counts.  The workspace holds five words per element, ws[j * (n + 2) + e]:
//   0  B, then the count, then the element's first segment number (row n + 1: the total)
//   1  the first segment start x0        2  NF
//   3  the own message start P, then the first segment's (m_first)        4  NM
constexpr uint32_t kFrameThreads = 1024;
constexpr uint32_t kFrameWaves = kFrameThreads / 64;

struct FwdScan {  // sums and "last index" maxima
    uint64_t sum;
    uint32_t ln, le;
    __device__ __forceinline__ static FwdScan identity() { return {0ull, 0u, 0u}; }
    __device__ __forceinline__ static FwdScan combine(const FwdScan& a, const FwdScan& b)
    {
        return {a.sum + b.sum, max(a.ln, b.ln), max(a.le, b.le)};
    }
    __device__ __forceinline__ FwdScan up(uint32_t d) const { return {lane_up(sum, d), lane_up(ln, d), lane_up(le, d)}; }
};
struct MaxScan {
    uint64_t v;
    __device__ __forceinline__ static MaxScan identity() { return {0ull}; }
    __device__ __forceinline__ static MaxScan combine(const MaxScan& a, const MaxScan& b) { return {max(a.v, b.v)}; }
    __device__ __forceinline__ MaxScan up(uint32_t d) const { return {lane_up(v, d)}; }
};
struct SumScan {
    uint64_t v;
    __device__ __forceinline__ static SumScan identity() { return {0ull}; }
    __device__ __forceinline__ static SumScan combine(const SumScan& a, const SumScan& b) { return {a.v + b.v}; }
    __device__ __forceinline__ SumScan up(uint32_t d) const { return {lane_up(v, d)}; }
};
struct BackScan {  // minima of positions
    uint64_t nf, nm, cp;
    __device__ __forceinline__ static BackScan identity() { return {kStreamNone, kStreamNone, kStreamNone}; }
    __device__ __forceinline__ static BackScan combine(const BackScan& a, const BackScan& b)
    {
        return {min(a.nf, b.nf), min(a.nm, b.nm), min(a.cp, b.cp)};
    }
    __device__ __forceinline__ BackScan up(uint32_t d) const { return {lane_up(nf, d), lane_up(nm, d), lane_up(cp, d)}; }
};

// One tile of a scan: `carry` is the combination of everything before the tile and is advanced
// over it; the results cover everything before the thread's value, without it (excl) and with it
// (incl).  Every thread of the workgroup calls it; `part` is LDS for one value per wave.
template <typename T>
__device__ __forceinline__ void tile_scan(T v, T& carry, T* part, T& excl, T& incl)
{
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const T u = v.up(d);
        if (lane >= d) v = T::combine(u, v);
    }
    const T before = v.up(1);
    if (lane == 63) part[wv] = v;
    __syncthreads();
    T base = carry;
    for (uint32_t w = 0; w < kFrameWaves; ++w) {
        const T p = part[w];
        if (w < wv) base = T::combine(base, p);
        carry = T::combine(carry, p);
    }
    __syncthreads();  // (part is free for the next scan)
    excl = lane ? T::combine(base, before) : base;
    incl = T::combine(base, v);
}

__global__ __launch_bounds__(kFrameThreads) void stream_frame_scan_kernel(StreamFrameArgs a)
{
    __shared__ FwdScan part_f[kFrameWaves];
    __shared__ MaxScan part_m[kFrameWaves];
    __shared__ BackScan part_b[kFrameWaves];
    __shared__ SumScan part_s[kFrameWaves];
    const uint32_t tid = threadIdx.x, S = a.S;
    const uint64_t ne = (uint64_t)a.n + 1u, row = (uint64_t)a.n + 2u;
    uint64_t* __restrict__ w_at = a.ws;
    uint64_t* __restrict__ w_x0 = a.ws + row;
    uint64_t* __restrict__ w_nf = a.ws + 2u * row;
    uint64_t* __restrict__ w_mf = a.ws + 3u * row;
    uint64_t* __restrict__ w_nm = a.ws + 4u * row;
    const bool pending0 = a.state.msg_start_pending != 0;

    // the scans over the elements before
    FwdScan cf = FwdScan::identity();
    MaxScan cg = MaxScan::identity();
    for (uint64_t t0 = 0; t0 < ne; t0 += kFrameThreads) {
        const uint64_t e = t0 + tid;
        uint32_t len = 0, fl = 0;
        if (e == 0) len = a.state.carry_bytes;
        else if (e < ne) len = a.write_len[e - 1u], fl = a.write_flags[e - 1u];
        FwdScan fx, fi;
        tile_scan(FwdScan{len, e && len ? (uint32_t)e : 0u, fl & NFEC_STREAM_EOM ? (uint32_t)e : 0u}, cf, part_f, fx, fi);
        MaxScan gx, gi;
        tile_scan(MaxScan{fl & NFEC_STREAM_FLUSH ? fi.sum : 0ull}, cg, part_m, gx, gi);
        if (e < ne) {
            uint64_t P;
            if (e == 0) P = a.state.carry_msg_start ? a.state.carry_msg_start - 1u : kStreamNone;
            else P = stream_is_message_start(len, fx.ln, fx.le, pending0) ? fx.sum : kStreamNone;
            w_at[e] = fx.sum;
            w_x0[e] = stream_first_start(fx.sum, gx.v, S);
            w_mf[e] = P;
        }
    }
    const uint64_t end = cf.sum, consumed = stream_consumed(cg.v, end, S);
    __syncthreads();  // (the last tile's rows are written: the next pass reads them from other threads)

    // the scans over the elements behind (element n first), and the counts
    BackScan cb = BackScan::identity();
    for (uint64_t t0 = 0; t0 < ne; t0 += kFrameThreads) {
        const uint64_t r = t0 + tid;
        const bool in = r < ne;
        const uint64_t e = in ? ne - 1u - r : 0u;
        uint32_t len = 0, fl = 0;
        uint64_t B = 0, P = kStreamNone;
        if (in) {
            if (e == 0) len = a.state.carry_bytes;
            else len = a.write_len[e - 1u], fl = a.write_flags[e - 1u];
            B = w_at[e], P = w_mf[e];
        }
        BackScan bx, bi;
        tile_scan(BackScan{fl & NFEC_STREAM_FLUSH ? B + len : kStreamNone, P, P != kStreamNone && P >= consumed ? P : kStreamNone},
                  cb, part_b, bx, bi);
        if (in) {
            const uint64_t x0 = w_x0[e];
            w_nf[e] = bi.nf;
            w_nm[e] = bx.nm;
            w_mf[e] = P != kStreamNone && P >= x0 ? P : bx.nm;
            w_at[e] = stream_closed_count(x0, B + len, bi.nf, consumed, S);
        }
    }

    __syncthreads();  // (as above)
    // each element's first segment number; row n + 1: the total
    SumScan cs = SumScan::identity();
    for (uint64_t t0 = 0; t0 <= ne; t0 += kFrameThreads) {
        const uint64_t e = t0 + tid;
        SumScan sx, si;
        tile_scan(SumScan{e < ne ? w_at[e] : 0ull}, cs, part_s, sx, si);
        if (e <= ne) w_at[e] = sx.v;
    }

    if (tid == 0) {
        const uint32_t carry_ms = stream_carry_msg_start(cb.cp, consumed);
        a.totals[0] = cs.v, a.totals[1] = consumed, a.totals[2] = end - consumed, a.totals[3] = carry_ms;
        nfec_stream_state st = a.state;
        st.write_offset += (uint32_t)consumed;
        st.msg_start_pending = stream_flag_raised(cf.ln, cf.le, pending0);
        st.carry_bytes = (uint32_t)(end - consumed);
        st.carry_msg_start = carry_ms;
        st.next_slot += cs.v;
        *a.state_out = st;
    }
}

// One lane per segment: its element is the last whose first segment number is not above it.
__global__ __launch_bounds__(256) void stream_frame_expand_kernel(StreamFrameArgs a)
{
    const uint64_t row = (uint64_t)a.n + 2u;
    const uint64_t* __restrict__ w_at = a.ws;
    const uint64_t count = min(w_at[row - 1u], (uint64_t)a.capacity);
    for (uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x; t < count; t += (uint64_t)gridDim.x * 256u) {
        uint64_t lo = 0, hi = row - 1u;  // w_at[lo] <= t < w_at[hi]
        while (hi - lo > 1u) {
            const uint64_t mid = lo + ((hi - lo) >> 1);
            if (w_at[mid] <= t) lo = mid;
            else hi = mid;
        }
        stream_segment_at(a.ws[row + lo], t - w_at[lo], a.S, a.ws[2u * row + lo], a.ws[3u * row + lo], a.ws[4u * row + lo],
                          a.seg_start + t, a.seg_len + t, a.seg_msg_start + t);
    }
}

StreamShape stream_shape(const BatchView& v, uint32_t pieces)
{
    StreamShape sh;
    sh.runs = (v.k + kRun - 1u) / kRun;
    sh.pieces = pieces;
    sh.magic = div_magic32(pieces);
    sh.step_sl = 256u / pieces, sh.step_p = 256u % pieces;
    return sh;
}

}  // namespace

// (all three: the ABI entry has checked the arguments and returned for a call with nothing to do)
int launch_stream_frame(const StreamFrameArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(stream_frame_scan_kernel, dim3(1), dim3(kFrameThreads), 0, s, a);
    if (a.capacity) {
        const uint32_t grid = (uint32_t)std::min<uint64_t>(((uint64_t)a.capacity + 255u) / 256u, kMaxGroups);
        hipLaunchKernelGGL(stream_frame_expand_kernel, dim3(grid), dim3(256), 0, s, a);
    }
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? NFEC_OK : hip_fail(e, "stream_frame launch");
}

int launch_stream_pack(const StreamPackArgs& a, hipStream_t s)
{
    StreamShape sh = stream_shape(a.batch, gather_pieces(a.batch.vec - kStreamHeader));
    // the blocks that hold the slots [first_slot, first_slot + count + end), inside the batch
    const uint64_t first = a.first_slot / a.batch.k, last = (a.first_slot + a.count + a.end - 1u) / a.batch.k;
    if (first < a.batch.nblocks) {
        sh.b0 = (uint32_t)first;
        sh.nb = (uint32_t)(std::min<uint64_t>(last, a.batch.nblocks - 1u) - first + 1u);
    }
    const uint32_t grid = (uint32_t)std::min<uint64_t>(std::max<uint64_t>((uint64_t)sh.nb * sh.runs, 1u), kMaxGroups);
    hipLaunchKernelGGL(stream_pack_kernel, dim3(grid), dim3(256), 0, s, a, sh);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? NFEC_OK : hip_fail(e, "stream_pack launch");
}

int launch_stream_unpack(const StreamUnpackArgs& a, hipStream_t s)
{
    // the most aligned 16-byte pieces a segment of S bytes can touch (15 bytes into one)
    const StreamShape sh = stream_shape(a.batch, (a.S + 30u) / 16u);
    const uint32_t grid = (uint32_t)std::min<uint64_t>((uint64_t)a.batch.nblocks * sh.runs, kMaxGroups);
    hipLaunchKernelGGL(stream_unpack_kernel, dim3(grid), dim3(256), 0, s, a, sh);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? NFEC_OK : hip_fail(e, "stream_unpack launch");
}

}  // namespace nfec
