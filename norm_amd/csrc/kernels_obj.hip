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

#include "nfec_internal.hpp"
#include "object_layout.hpp"
#include "segment_copy.hpp"

namespace nfec {

namespace {

constexpr uint32_t kRun = 64;         // segments per work item
constexpr uint32_t kMaxGroups = 8192; // as rx_place caps its grid; workgroups stride over the items

// Piece p of a source slot from the object bytes src[16p ...] (segment_copy.hpp, the gather rule),
// with the shift between the object and the slot per lane.  The piece's second chunk is the first
// chunk of the segment's next piece, which the next lane holds when that piece is in the same
// wave (flat indices are consecutive): it comes from there, one cross-lane move per dword, and is
// loaded only at the wave's last lane and where the next piece loads nothing -- a misaligned object
// costs one load per piece, not two.  All lanes of a wave that are in the loop call this together.
__device__ __forceinline__ void read_piece(uint8_t* __restrict__ slot, const uint8_t* __restrict__ src, uint32_t len,
                                           uint32_t vec, uint32_t p, uint32_t pieces, uint32_t lane)
{
    const u32x4 q0 = gather_first_chunk(src, len, p);
    const u32x4 next_q0 = {(uint32_t)__shfl_down(q0[0], 1, 64), (uint32_t)__shfl_down(q0[1], 1, 64),
                           (uint32_t)__shfl_down(q0[2], 1, 64), (uint32_t)__shfl_down(q0[3], 1, 64)};
    gather_store_piece(slot, src, len, vec, p, q0, next_q0, gather_second_from_next(lane, p, pieces, len),
                       PickPerLane());
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
    for (ItemWalk it(sh.runs); it.i < a.batch.nblocks; it.next()) {
        Run run;
        if (!run.init(a, a.first_block + (uint32_t)it.i, it.r)) continue;
        uint8_t* __restrict__ slot0 = a.batch.base + it.i * a.batch.block_stride + (uint64_t)run.s0 * a.batch.seg_stride;
        const uint8_t* __restrict__ src0 = a.object + run.off0;
        if (a.num_data_out && it.r == 0 && tid == 0) a.num_data_out[it.i] = (uint16_t)run.nd;
        if (a.seg_length_out && tid < run.nseg)
            a.seg_length_out[it.i * a.length_stride + run.s0 + tid] = (uint16_t)run.length(a, tid);
        for (PieceWalk w(tid, sh); w.sl < run.nseg; w.next(sh))
            read_piece(slot0 + (uint64_t)w.sl * a.batch.seg_stride, src0 + __umul24(w.sl, a.lay.segment_size),
                       run.length(a, w.sl), a.batch.vec, w.p, sh.pieces, tid & 63u);
    }
}

__global__ __launch_bounds__(256) void obj_write_kernel(ObjArgs a, ObjShape sh)
{
    const uint32_t tid = threadIdx.x;
    uint32_t n_sel = 0, n_not = 0;
    for (ItemWalk it(sh.runs); it.i < a.batch.nblocks; it.next()) {
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
        const uint8_t* __restrict__ slot0 = a.batch.base + it.i * a.batch.block_stride + (uint64_t)run.s0 * a.batch.seg_stride;
        uint8_t* __restrict__ dst0 = a.object + run.off0;
        for (PieceWalk w(tid, sh); w.sl < run.nseg; w.next(sh)) {
            if (!((sel >> w.sl) & 1ull)) continue;
            const uint32_t rel = __umul24(w.sl, a.lay.segment_size);  // (below 64 * 65,535)
            if (rel >= room) continue;
            const uint32_t len = (uint32_t)min((uint64_t)run.length(a, w.sl), room - rel);
            // the aligned 16-byte piece w.p of the segment's object bytes (segment_copy.hpp, the scatter
            // rule without a payload ID; nothing where the segment has no such piece): no byte of a
            // neighbouring segment is stored or read
            scatter_piece(dst0 + rel, slot0 + (uint64_t)w.sl * a.batch.seg_stride, len, 0, 0, w.p);
        }
    }
    // the workgroup's counts are its first wave's: one vector atomic per counter from lane 0
    if (a.stats && tid == 0) {
        if (n_sel) atomicAdd(a.stats + 0, n_sel);
        if (n_not) atomicAdd(a.stats + 1, n_not);
    }
}

// the flat index's shape for segments of `pieces` pieces, and the grid
ObjShape obj_shape(const ObjArgs& a, uint32_t pieces, uint32_t& grid)
{
    ObjShape sh;
    sh.runs = (a.lay.large_block_size + kRun - 1u) / kRun;
    sh.pieces = pieces;
    sh.magic = div_magic32(pieces);
    sh.step_sl = 256u / pieces, sh.step_p = 256u % pieces;
    grid = (uint32_t)std::min<uint64_t>((uint64_t)a.batch.nblocks * sh.runs, kMaxGroups);
    return sh;
}

}  // namespace

// (both: the ABI entry has checked the arguments and returned for an empty batch)
int launch_obj_read(const ObjArgs& a, hipStream_t s)
{
    uint32_t grid = 0;
    const ObjShape sh = obj_shape(a, gather_pieces(a.batch.vec), grid);
    hipLaunchKernelGGL(obj_read_kernel, dim3(grid), dim3(256), 0, s, a, sh);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? NFEC_OK : hip_fail(e, "object_read launch");
}

int launch_obj_write(const ObjArgs& a, hipStream_t s)
{
    uint32_t grid = 0;
    // the most aligned 16-byte pieces a segment of segment_size bytes can touch (15 bytes into one)
    const ObjShape sh = obj_shape(a, (a.lay.segment_size + 30u) / 16u, grid);
    hipLaunchKernelGGL(obj_write_kernel, dim3(grid), dim3(256), 0, s, a, sh);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? NFEC_OK : hip_fail(e, "object_write launch");
}

}  // namespace nfec
