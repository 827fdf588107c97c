// kernels_obj.hip -- object segmentation on the device (nfec.h, "object segmentation on the device").
//
// read:  NormDataObject::ReadSegment (reference src/common/normObject.cpp:2673-2718) with the zero
//        pad of CalculateBlockParity (:2203-2229) for every source slot of a batch: the object's
//        bytes, at any alignment, go into the 8-byte aligned slots of their blocks.
// write: NormDataObject::WriteSegment (:2628-2670) for every selected source slot: received ones
//        (:1529) and, in a block Decode repaired, all of them (:1616).
//
// Both are 2-D copies.  A workgroup of 256 lanes takes a run of up to 64 consecutive segments of
// one block, and its lanes stride over the run's (segment, 16-byte piece) pairs as one flat index:
// a 1,400-byte vector's 88 pieces leave no lane idle in a second round, as one wave per segment
// (rx_place, tx_emit) does.  Lanes of a wave then sit in different segments, so the byte shift
// between the object and the slot is per lane: the dword pick is a select (v_cndmask_b32), the
// byte funnel v_alignbyte_b32.  There is no descriptor to fetch and no atomic but the stats, two
// per workgroup.  At 16 bytes per lane and step the index and address arithmetic is not free
// beside the copy: the flat index is split once per run and stepped
// by additions, and the segment rule (object_layout.hpp) is evaluated once per run.
#include <algorithm>
#include <string>

#include "nfec_internal.hpp"
#include "object_layout.hpp"

namespace nfec {

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

constexpr uint32_t kRun = 64;         // segments per work item
constexpr uint32_t kMaxGroups = 8192; // as rx_place caps its grid; workgroups stride over the items

// the low n bytes of a dword (n <= 0: none, n >= 4: all)
__device__ __forceinline__ uint32_t low_bytes(int32_t n) { return n >= 4 ? ~0u : n <= 0 ? 0u : (1u << (8 * n)) - 1u; }

// Piece p of a source slot: its bytes [16p, 16p + 16) from the object bytes src[16p ...], src at
// any alignment.  place_segment's rule (kernels_rx.hip) with a per-lane shift sh = 4 dsh + bsh:
// the two aligned 16-byte chunks that hold the piece, a chunk loaded only when it holds a byte of
// the segment the piece needs, so every load stays on a page the object touches.  The second
// chunk is the first chunk of the segment's next piece, which the next lane holds when that piece
// is in the same wave: it comes from there (one cross-lane move per dword) and is loaded only at
// the wave's last lane and where the next piece loads nothing -- a misaligned object costs one
// load per piece, not two.  All lanes of a wave that are in the loop call this together.  Bytes
// from `len` to `vec` are zeros; the piece that holds byte `vec` is stored by bytes, whole pieces
// as one 16-byte store where the slot's address allows it and as two 8-byte stores elsewhere.
__device__ __forceinline__ void read_piece(uint8_t* __restrict__ slot, const uint8_t* __restrict__ src, uint32_t len,
                                           uint32_t vec, uint32_t p, uint32_t pieces, uint32_t lane)
{
    const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(src) & 15u);
    const uint32_t dsh = sh >> 2, bsh = sh & 3u;
    const u32x4* __restrict__ chunk0 = reinterpret_cast<const u32x4*>(src - sh);
    const uint32_t d0 = p * 16u;
    const int32_t nvalid = (int32_t)len - (int32_t)d0;  // segment bytes from d0 on (may be <= 0 or > 16)
    u32x4 q0 = {0u, 0u, 0u, 0u};
    if (nvalid > 0) q0 = __builtin_nontemporal_load(chunk0 + p);
    u32x4 q1;
    q1.x = __shfl_down(q0.x, 1, 64), q1.y = __shfl_down(q0.y, 1, 64);
    q1.z = __shfl_down(q0.z, 1, 64), q1.w = __shfl_down(q0.w, 1, 64);
    // the next lane holds piece p + 1 of this segment (flat indices are consecutive) and loaded its
    // first chunk when the segment reaches past this piece
    const bool from_lane = lane != 63u && p + 1u < pieces && nvalid > 16;
    if (nvalid > 0 && sh != 0 && (int32_t)sh + nvalid > 16 && !from_lane) q1 = __builtin_nontemporal_load(chunk0 + p + 1);
    // dwords dsh .. dsh + 4 of the eight: by two dwords, then by one.  (Where no second chunk was
    // needed q1 is arbitrary: with sh == 0 none of it is picked, otherwise the segment ends inside
    // q0 and the mask below clears what follows.)
    const bool by2 = dsh & 2u, by1 = dsh & 1u;
    const uint32_t t0 = by2 ? q0.z : q0.x, t1 = by2 ? q0.w : q0.y, t2 = by2 ? q1.x : q0.z, t3 = by2 ? q1.y : q0.w,
                   t4 = by2 ? q1.z : q1.x, t5 = by2 ? q1.w : q1.y;
    const uint32_t e0 = by1 ? t1 : t0, e1 = by1 ? t2 : t1, e2 = by1 ? t3 : t2, e3 = by1 ? t4 : t3, e4 = by1 ? t5 : t4;
    uint32_t o[4];
    o[0] = __builtin_amdgcn_alignbyte(e1, e0, bsh);
    o[1] = __builtin_amdgcn_alignbyte(e2, e1, bsh);
    o[2] = __builtin_amdgcn_alignbyte(e3, e2, bsh);
    o[3] = __builtin_amdgcn_alignbyte(e4, e3, bsh);
    if (nvalid < 16) {  // the segment ends inside or before the piece: zeros from there on
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] &= low_bytes(nvalid - 4 * j);
    }
    const uint32_t nw = vec - d0;  // bytes of this piece inside the vector (> 0; >= 16: all)
    uint8_t* d = slot + d0;
    if (nw >= 16) {
        if ((reinterpret_cast<uintptr_t>(d) & 15u) == 0) {
            *reinterpret_cast<u32x4*>(d) = u32x4{o[0], o[1], o[2], o[3]};
        } else {
            *reinterpret_cast<u32x2*>(d) = u32x2{o[0], o[1]};
            *reinterpret_cast<u32x2*>(d + 8) = u32x2{o[2], o[3]};
        }
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

// Piece p of a written segment: the aligned 16-byte piece p of the object bytes [dst, dst + len),
// dst at any alignment, counted from the piece that holds dst[0].  emit_message's rule
// (kernels_tx.hip) without a payload ID and with a per-lane shift: the piece's slot bytes start
// `sh` bytes into a 16-byte step of the slot; three 8-byte chunks of the slot cover them at any
// shift, and a chunk is loaded only when it holds a byte the piece stores, which keeps every load
// inside [slot, slot + len rounded up to 8) and so inside seg_stride.  A piece wholly inside the
// segment is one 16-byte store; the first and the last piece store their own bytes only, as dwords
// where a whole dword is theirs and as bytes elsewhere, so no byte of a neighbouring segment is
// stored or read.  Returns without a store when the segment has no piece p.
__device__ __forceinline__ void write_piece(uint8_t* __restrict__ dst, const uint8_t* __restrict__ slot, uint32_t len,
                                            uint32_t p)
{
    const uint32_t dres = (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u);
    const uint32_t pieces = (dres + len + 15u) >> 4;
    if (p >= pieces) return;
    uint8_t* __restrict__ piece0 = dst - dres;
    // slot byte 0 lies dres bytes into piece 0: piece p holds slot bytes [16 (p - pb) + sh, + 16)
    const int32_t pb = (int32_t)((dres + 15u) >> 4);
    const uint32_t sh = (0u - dres) & 15u;
    const uint32_t dsh = (sh >> 2) & 1u, bsh = sh & 3u;
    const u32x2* __restrict__ chunk = reinterpret_cast<const u32x2*>(slot);
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
    for (int j = 0; j < 4; ++j) o[j] = __builtin_amdgcn_alignbyte(dsh ? e[j + 2] : e[j + 1], dsh ? e[j + 1] : e[j], bsh);
    const uint32_t first = p * 16u;  // the piece's first byte, counted from piece 0
    // the piece's own bytes [lo, hi)
    const uint32_t lo = p == 0 ? dres : 0u;
    const uint32_t hi = min(16u, dres + len - first);
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

// What the launch prepares for the flat index: runs per block, pieces per segment, the multiply
// that divides a lane's first index by them (object_layout.hpp) and the step of 256 indices.
struct ObjShape {
    uint32_t runs = 0;    // runs of kRun segments that cover the largest block
    uint32_t pieces = 0;  // 16-byte pieces per segment (write: the most a segment can have)
    uint32_t magic = 0;   // div_magic32(pieces)
    uint32_t step_sl = 0, step_p = 0;  // 256 / pieces, 256 % pieces
};

// Work items are (block, run) pairs, item = block * runs + run; workgroup g takes items g, g +
// gridDim.x, ...  The pair is stepped, not divided out of a 64-bit item number.
struct ItemWalk {
    uint64_t i;  // block of the batch
    uint32_t r;  // run of the block
    uint32_t step_i, step_r, runs;
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

// A lane's flat index tid, tid + 256, ... over a run as the pair (segment of the run, piece): one
// multiply at the start, additions from there on.  At 16 bytes per lane and step the address
// arithmetic is not free beside the copy, so nothing in the loop divides or multiplies in 64 bits.
struct PieceWalk {
    uint32_t sl, p;
    __device__ __forceinline__ PieceWalk(uint32_t tid, const ObjShape& sh)
    {
        sl = div_by_magic32(tid, sh.magic), p = tid - sl * sh.pieces;
    }
    __device__ __forceinline__ void next(const ObjShape& sh)
    {
        sl += sh.step_sl, p += sh.step_p;
        if (p >= sh.pieces) p -= sh.pieces, ++sl;
    }
};

// One run: segments [s0, s0 + nseg) of object block b.  Its first segment's offset comes from the
// segment rule; segment s0 + sl lies sl * segment_size bytes past it (object_layout.hpp), and only
// the block's last segment can be the short one.
struct Run {
    uint32_t nd, s0, nseg, short_at;  // short_at: the run's segment of final_segment_size bytes (or none)
    uint64_t off0;
    __device__ __forceinline__ bool init(const ObjArgs& a, uint32_t b, uint32_t r)
    {
        nd = object_block_size(a.lay, b);
        s0 = r * kRun;
        if (s0 >= nd) return false;
        nseg = min(kRun, nd - s0);
        uint32_t len0;
        object_segment_at(a.lay, b, s0, &off0, &len0);
        short_at = object_segment_length(a.lay, b, nd - 1u) != a.lay.segment_size ? nd - 1u - s0 : ~0u;
        return true;
    }
    __device__ __forceinline__ uint32_t length(const ObjArgs& a, uint32_t sl) const
    {
        return sl == short_at ? a.lay.final_segment_size : a.lay.segment_size;
    }
};

__global__ __launch_bounds__(256) void obj_read_kernel(ObjArgs a, ObjShape sh)
{
    const uint32_t tid = threadIdx.x;
    for (ItemWalk it(sh.runs); it.i < a.nblocks; it.next()) {
        Run run;
        if (!run.init(a, a.first_block + (uint32_t)it.i, it.r)) continue;
        uint8_t* __restrict__ slot0 = a.base + it.i * a.block_stride + (uint64_t)run.s0 * a.seg_stride;
        const uint8_t* __restrict__ src0 = a.object + run.off0;
        if (a.num_data_out && it.r == 0 && tid == 0) a.num_data_out[it.i] = (uint16_t)run.nd;
        if (a.seg_length_out && tid < run.nseg)
            a.seg_length_out[it.i * a.length_stride + run.s0 + tid] = (uint16_t)run.length(a, tid);
        for (PieceWalk w(tid, sh); w.sl < run.nseg; w.next(sh))
            read_piece(slot0 + (uint64_t)w.sl * a.seg_stride, src0 + __umul24(w.sl, a.lay.segment_size),
                       run.length(a, w.sl), a.vec, w.p, sh.pieces, tid & 63u);
    }
}

__global__ __launch_bounds__(256) void obj_write_kernel(ObjArgs a, ObjShape sh)
{
    const uint32_t tid = threadIdx.x;
    uint32_t n_sel = 0, n_not = 0;
    for (ItemWalk it(sh.runs); it.i < a.nblocks; it.next()) {
        Run run;
        if (!run.init(a, a.first_block + (uint32_t)it.i, it.r)) continue;
        // the run's selection: the two mask words of its 64 segments (s0 is a multiple of 64),
        // or every segment without a mask or in a repaired block
        uint64_t sel = ~0ull;
        if (a.received && !(a.status && a.status[it.i] > 0)) {
            const uint32_t* __restrict__ mw = a.received + it.i * a.mask_stride + (run.s0 >> 5);
            sel = mw[0];
            if (run.nseg > 32) sel |= (uint64_t)mw[1] << 32;  // (slot s0 + 32 < nd <= k: inside the mask)
        }
        if (run.nseg < 64) sel &= (1ull << run.nseg) - 1ull;
        const uint32_t picked = (uint32_t)__popcll(sel);
        n_sel += picked, n_not += run.nseg - picked;
        // WriteSegment's clamp at data_max, relative to the run's first byte
        if (run.off0 >= a.object_bytes) continue;
        const uint64_t room = a.object_bytes - run.off0;
        const uint8_t* __restrict__ slot0 = a.base + it.i * a.block_stride + (uint64_t)run.s0 * a.seg_stride;
        uint8_t* __restrict__ dst0 = a.object + run.off0;
        for (PieceWalk w(tid, sh); w.sl < run.nseg; w.next(sh)) {
            if (!((sel >> w.sl) & 1ull)) continue;
            const uint32_t rel = __umul24(w.sl, a.lay.segment_size);  // (below 64 * 65,535)
            if (rel >= room) continue;
            const uint32_t len = (uint32_t)min((uint64_t)run.length(a, w.sl), room - rel);
            write_piece(dst0 + rel, slot0 + (uint64_t)w.sl * a.seg_stride, len, w.p);
        }
    }
    // the workgroup's counts are its first wave's: one vector atomic per counter from lane 0
    if (a.stats && tid == 0) {
        if (n_sel) atomicAdd(a.stats + 0, n_sel);
        if (n_not) atomicAdd(a.stats + 1, n_not);
    }
}

int check_obj(const ObjArgs& a, const char* what, ObjShape& sh, uint32_t pieces, uint32_t& grid)
{
    if (!a.base) return fail(NFEC_EINVAL, std::string(what) + ": null blocks pointer");
    if (!a.object) return fail(NFEC_EINVAL, std::string(what) + ": null object");
    if ((reinterpret_cast<uintptr_t>(a.base) | a.block_stride | a.seg_stride) & 7)
        return fail(NFEC_EINVAL, std::string(what) + ": blocks, seg_stride and block_stride must be multiples of 8 bytes");
    if (a.seg_stride < a.vec) return fail(NFEC_EINVAL, std::string(what) + ": seg_stride < vector_size");
    if (a.lay.segment_size > a.vec) return fail(NFEC_EINVAL, std::string(what) + ": segment_size > vector_size");
    if ((uint64_t)a.first_block + a.nblocks > a.lay.num_blocks)
        return fail(NFEC_EINVAL, std::string(what) + ": first_block + nblocks > num_blocks");
    sh.runs = (a.lay.large_block_size + kRun - 1u) / kRun;
    sh.pieces = pieces;
    sh.magic = div_magic32(pieces);
    sh.step_sl = 256u / pieces, sh.step_p = 256u % pieces;
    grid = (uint32_t)std::min<uint64_t>((uint64_t)a.nblocks * sh.runs, kMaxGroups);
    return NFEC_OK;
}

}  // namespace

int launch_obj_read(const ObjArgs& a, hipStream_t s)
{
    if (a.nblocks == 0) return NFEC_OK;
    ObjShape sh;
    uint32_t grid = 0;
    // a slot's pieces: its vec bytes from the slot's start
    int rc = check_obj(a, "object_read", sh, (a.vec + 15u) / 16u, grid);
    if (rc) return rc;
    if (a.object_bytes < a.lay.object_size) return fail(NFEC_EINVAL, "object_read: object_bytes < object_size");
    if (a.seg_length_out && a.length_stride < a.lay.num_data) return fail(NFEC_EINVAL, "object_read: length_stride < k");
    hipLaunchKernelGGL(obj_read_kernel, dim3(grid), dim3(256), 0, s, a, sh);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? NFEC_OK : hip_fail(e, "object_read launch");
}

int launch_obj_write(const ObjArgs& a, hipStream_t s)
{
    if (a.nblocks == 0) return NFEC_OK;
    ObjShape sh;
    uint32_t grid = 0;
    // the most aligned 16-byte pieces a segment of segment_size bytes can touch (15 bytes into one)
    int rc = check_obj(a, "object_write", sh, (a.lay.segment_size + 30u) / 16u, grid);
    if (rc) return rc;
    if (a.received && (uint64_t)a.mask_stride * 32u < (uint64_t)a.lay.num_data)
        return fail(NFEC_EINVAL, "object_write: mask_stride smaller than the source slots");
    hipLaunchKernelGGL(obj_write_kernel, dim3(grid), dim3(256), 0, s, a, sh);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? NFEC_OK : hip_fail(e, "object_write launch");
}

}  // namespace nfec
