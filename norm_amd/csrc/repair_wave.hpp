// repair_wave.hpp -- what the kernels of the repair cycle share (kernels_nack.hip,
// kernels_txrepair.hip, kernels_suppress.hip; device code only): the loads of repair-request
// content at any byte alignment, a block's class and cut from one pass over its mask words, and
// the counters of a workgroup added once.
#pragma once

#include "nack_layout.hpp"
#include "wave.hpp"

namespace nfec {

// ---- bytes of a message ----

// The four bytes at p, which lie in the message, at any alignment: the aligned dword that holds
// the first and, when they straddle it, the one behind it; both hold a byte of the message.
__device__ __forceinline__ uint32_t load32(const uint8_t* __restrict__ p)
{
    const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 3u);
    const uint32_t* __restrict__ q = reinterpret_cast<const uint32_t*>(p - sh);
    const uint32_t lo = q[0];
    if (sh == 0) return lo;
    const uint32_t hi = q[1];
    return (lo >> (8u * sh)) | (hi << (32u - 8u * sh));
}

struct WireItem {
    uint32_t fec_id, object_id, block, symbol;
};
// an item of L bytes at p: fec_id, reserved, object id, then the payload ID (nack_layout.hpp)
__device__ __forceinline__ WireItem load_item(uint32_t id_kind, uint32_t first_block_id, const uint8_t* __restrict__ p, uint32_t L)
{
    const uint32_t w = load32(p), w0 = load32(p + 4), w1 = L == 12u ? load32(p + 8) : 0u;
    const RxId id = rx_id_decode(id_kind, w0, w1, first_block_id);
    return WireItem{w & 0xffu, bswap16(w >> 16), id.block, id.symbol};
}

// ---- counters ----

__device__ __forceinline__ void add64(uint64_t* p, uint64_t v)
{
    if (v) atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);
}

// The workgroup's counters into totals[0 .. N): one atomic per counter and workgroup.  (One per
// block on one address costs more than the blocks' work: 65,536 blocks took 1.4 ms that way.)
// Every wave of a workgroup of four calls it once, with its lane 0 holding the wave's counts.
template <int N>
__device__ __forceinline__ void group_add(uint64_t* totals, const uint64_t (&v)[N], uint32_t lane)
{
    __shared__ unsigned long long sums[4][N];
    if (lane == 0)
        for (int j = 0; j < N; ++j) sums[threadIdx.x >> 6][j] = v[j];
    __syncthreads();
    if (threadIdx.x < (uint32_t)N) add64(totals + threadIdx.x, sums[0][threadIdx.x] + sums[1][threadIdx.x] + sums[2][threadIdx.x] + sums[3][threadIdx.x]);
}

// ---- one block of a reception mask ----

struct BlockShape {
    uint32_t cls;
    NackCut cut;
};

// e, p, whether anything arrived, and the m-th pending slot: one pass over the block's words, 64 a
// round, the pending count carried between rounds.  The lane whose word holds the m-th pending slot
// steps to it through its own 32 bits.  word0 (may be null): the lane's word of the first round,
// that is mask[lane] (0 past the block's words), for a caller that goes on with the words.
__device__ __forceinline__ BlockShape block_shape(uint32_t k, uint32_t m, const uint32_t* __restrict__ mask, uint32_t nd,
                                                  uint32_t lane, uint32_t* word0 = nullptr)
{
    BlockShape r = {NACK_SILENT, {0u, 0u}};
    if (word0) *word0 = 0u;
    if (nd < 1 || nd > k) return r;
    const uint32_t n = nd + m, w_end = (n + 31u) >> 5;
    uint32_t e = 0, p = 0, any = 0, before = 0, mth = 0;
    for (uint32_t w0 = 0; w0 < w_end; w0 += 64) {
        const uint32_t w = w0 + lane;
        const uint32_t word = w < w_end ? mask[w] : 0u;
        if (word0 && w0 == 0) *word0 = word;
        const uint32_t valid = nack_range_bits(w, 0, n), src = nack_range_bits(w, 0, nd);
        const uint32_t pend = ~word & valid;
        e += __popc(pend & src);
        p += __popc(word & valid & ~src);
        any |= word & valid;
        const uint32_t cnt = __popc(pend), inc = wave_scan(cnt, lane), exc = before + inc - cnt;
        const bool hit = exc < m && m <= exc + cnt;
        uint32_t slot = 0;
        if (hit) {
            uint32_t t = pend;
            for (uint32_t i = m - exc; i > 1; --i) t &= t - 1u;
            slot = (w << 5) + (__ffs(t) - 1u);
        }
        const uint64_t owner = __ballot(hit);
        if (owner) mth = __shfl(slot, __ffsll((unsigned long long)owner) - 1, 64);
        before += __shfl(inc, 63, 64);
    }
    e = __shfl(wave_scan(e, lane), 63, 64);
    p = __shfl(wave_scan(p, lane), 63, 64);
    any = __any(any != 0);
    r.cls = uniform(nack_class(nd, k, e, p, any));
    r.cut = nack_cut(nd, m, e, mth);
    r.cut.lo = uniform(r.cut.lo), r.cut.hi = uniform(r.cut.hi);
    return r;
}

}  // namespace nfec
