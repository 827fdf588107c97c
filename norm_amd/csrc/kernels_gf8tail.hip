// kernels_gf8tail.hip -- the segment tails of the RS8 / MDP fast kernels.
//
// The bit-sliced GF(2^8) kernels (q4, the runtime-coefficient kernel, the fused and unfused
// fixed-shape repair) work in 8-byte lane pieces, so they cover the first vec & ~7 bytes of each
// segment.  NORM's vectors are segmentSize + 8 bytes (normSession.cpp:883): a 1452-byte segment
// gives 1460-byte vectors, 4 bytes past the last piece.  The product is the same at every byte
// position, so the callers run the fast kernels over vec & ~7 and one of the two kernels here over
// the last 1..7 bytes, writing disjoint bytes:
//   gf8_rt_tail_kernel         the runtime-coefficient kernel's products (gen_rs8_rt.hip), from its
//                              own arguments and snippet-offset tables: every encode, the
//                              closed-form RS8 repair, the MDP repair
//   rs8_fixed_dec_tail_kernel  the fixed-shape RS8 repair, from the closed-form plan's outputs
// Both multiply through log / exp lookups in the field 0x11d, read a column's tail as one 8-byte
// load at slot + off (strides are multiples of 8 and at least vec, nfec.h: the 8 bytes stay inside
// the slot) and store exactly nbytes bytes per output row, so the callers' bytes [vec, seg_stride)
// keep their contents.
#include "nfec_internal.hpp"

namespace nfec {

namespace {

__constant__ Gf8Tables kGf8Tables = make_gf8_tables();

constexpr uint32_t kTailThreads = 64;
constexpr uint32_t kTailMaxBytes = 7;
constexpr uint32_t kNoLog = 0xffffu;

__device__ __forceinline__ uint32_t tail_byte(const uint2& v, uint32_t j)
{
    return ((j < 4u ? v.x : v.y) >> (8u * (j & 3u))) & 255u;
}

// acc[j] ^= c * x_j for the tail bytes j < nbytes (lc = log c, c != 0)
// (one compiled form per tail length measured the same on encode and 3 % faster on repair: not kept)
__device__ __forceinline__ void tail_addmul(uint32_t (&acc)[kTailMaxBytes], uint32_t lc, const uint2& x, uint32_t nbytes,
                                            const uint8_t* ex, const uint16_t* lg)
{
#pragma unroll
    for (uint32_t j = 0; j < kTailMaxBytes; ++j) {
        const uint32_t lx = lg[tail_byte(x, j)];
        if (j < nbytes && lx != kNoLog) acc[j] ^= ex[lc + lx];
    }
}

__device__ __forceinline__ void tail_store(uint8_t* out, const uint32_t (&acc)[kTailMaxBytes], uint32_t nbytes, bool xor_in)
{
#pragma unroll
    for (uint32_t j = 0; j < kTailMaxBytes; ++j)
        if (j < nbytes) out[j] = (uint8_t)(xor_in ? acc[j] ^ out[j] : acc[j]);
}

// One thread per (block, output row): rpg rows per block in a workgroup (a power of two up to 64;
// 64 / rpg blocks share a workgroup, blocks of more than 64 rows take `chunks` workgroups).
// Blocks, columns, rows, slots and table entries are enumerated exactly as rs8_rt_kernel does.
__global__ __launch_bounds__(kTailThreads) void gf8_rt_tail_kernel(Rs8RtArgs a, uint32_t off, uint32_t nbytes,
                                                                   uint32_t rpg, uint32_t chunks)
{
    __shared__ uint8_t ex[512];
    __shared__ uint16_t lg[256];
    const uint32_t t = threadIdx.x;
    for (uint32_t i = t; i < 512; i += kTailThreads) ex[i] = kGf8Tables.exp[i];
    for (uint32_t i = t; i < 256; i += kTailThreads) lg[i] = i ? kGf8Tables.log[i] : (uint16_t)kNoLog;
    __syncthreads();  // the only barrier: every thread reaches it
    const uint64_t blk64 = (uint64_t)(blockIdx.x / chunks) * (kTailThreads / rpg) + t / rpg;
    const uint32_t r = (blockIdx.x % chunks) * rpg + t % rpg;
    if (blk64 >= a.nblocks) return;
    const uint32_t blk = (uint32_t)blk64;
    const bool pb = a.per_block != 0u;
    uint32_t kk = a.k, rows = a.m, nd = a.k;
    if (a.num_data) nd = a.num_data[blk];
    if (nd == 0u || nd > a.k) return;  // left alone, as the fast kernel does
    if (pb) {
        kk = a.blk_cols ? (uint32_t)a.blk_cols[blk] : (a.num_data ? nd : a.k);
        if (a.blk_rows) {
            const int32_t e = a.blk_rows[blk];
            rows = e > 0 ? min((uint32_t)e, a.m) : 0u;
        }
        // a plan writes no slot list or table for a block it rejected or that has no erasure
        if (rows == 0u || kk == 0u || kk > a.k) return;
    } else if (a.num_data) {
        kk = nd;  // flat shortened: the block stops at its own numData
    }
    if (r >= rows) return;
    // this row's table entries: (c, r) at tb + c * tab_col_stride
    const uint8_t* tb = reinterpret_cast<const uint8_t*>(a.tab) +
                        (pb && a.tab_block_stride ? (uint64_t)(a.tab_by_count ? nd - 1u : blk) * a.tab_block_stride : 0u);
    if (a.tab_pass_stride) {
        uint32_t p = 0, row0 = 0, row1 = 0;
        const uint32_t np = rs8_rt_passes(rows);
        for (; p < np; ++p) {
            rs8_rt_pass_rows(rows, p, row0, row1);
            if (r < row1) break;
        }
        if (p >= np || r < row0) return;  // (the passes cover [0, rows): not reached)
        tb += (uint64_t)p * a.tab_pass_stride + 2u * (r - row0);
    } else {
        tb += 2u * r;
    }
    const uint32_t bound = a.slot_bound ? a.slot_bound : 65536u;
    const uint16_t* isl = pb && a.in_slots ? a.in_slots + (uint64_t)blk * a.in_slots_stride : nullptr;
    const uint8_t* in = a.in_base + (uint64_t)blk * a.in_block_stride + off;
    uint32_t acc[kTailMaxBytes] = {0, 0, 0, 0, 0, 0, 0};
#pragma unroll 4
    for (uint32_t c = 0; c < kk; ++c) {
        const uint32_t coef = ((uint32_t)*reinterpret_cast<const uint16_t*>(tb + (uint64_t)c * a.tab_col_stride) >> 7) & 255u;
        const uint32_t slot = isl ? (uint32_t)isl[c] : a.in_slot0 + c;
        if (coef == 0u || slot >= bound) continue;
        const uint2 x = *reinterpret_cast<const uint2*>(in + (uint64_t)slot * a.in_seg_stride);
        tail_addmul(acc, lg[coef], x, nbytes, ex, lg);
    }
    uint32_t oslot;
    if (pb) {
        oslot = a.out_slots ? (uint32_t)a.out_slots[(uint64_t)blk * a.out_slots_stride + r]
                            : a.out_slot0 + (a.out_after_data ? nd : 0u) + r;
    } else {
        oslot = a.out_slot0 + (a.num_data ? nd : 0u) + r;  // flat shortened: parity at slot numData + r
    }
    if (oslot >= bound) return;
    uint8_t* out = a.out_base + (uint64_t)blk * a.out_block_stride + (uint64_t)oslot * a.out_seg_stride + off;
    tail_store(out, acc, nbytes, a.accumulate != 0u);
}

constexpr uint32_t kFixWaves = 4;  // blocks per workgroup, one wave each: they share the tables

__global__ __launch_bounds__(64 * kFixWaves) void rs8_fixed_dec_tail_kernel(Rs8FixedDecTailArgs a, uint32_t off,
                                                                            uint32_t nbytes)
{
    __shared__ uint8_t ex[512];
    __shared__ uint16_t lg[256];
    __shared__ uint2 dcol[kFixWaves][64];  // the block's received source tails (erased columns: 0)
    __shared__ uint2 zrow[kFixWaves][64];  // z_p of the parity rows used
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    for (uint32_t i = threadIdx.x; i < 512; i += 64 * kFixWaves) ex[i] = kGf8Tables.exp[i];
    for (uint32_t i = threadIdx.x; i < 256; i += 64 * kFixWaves) lg[i] = i ? kGf8Tables.log[i] : (uint16_t)kNoLog;
    const uint64_t b = (uint64_t)blockIdx.x * kFixWaves + w;
    // the plan's outputs for this block; a block with nothing to repair (undecodable, invalid
    // numData, no source erased: rows = 0) only keeps the workgroup's barriers
    uint32_t e = 0, nd = a.k;
    uint64_t em = ~0ull, pused = 0;
    if (b < a.nblocks) {
        const int32_t ev = a.rows[b];
        e = ev > 0 ? (uint32_t)ev : 0u;
        if (a.num_data) nd = a.num_data[b];
        em = (uint64_t)a.emask[b * 2] | ((uint64_t)a.emask[b * 2 + 1] << 32);
        pused = ((uint64_t)a.psel[b * 2] | ((uint64_t)a.psel[b * 2 + 1] << 32)) & ((1ull << a.m) - 1ull);
    }
    const bool act = e > 0u && e <= a.k && e <= a.m && nd >= 1u && nd <= a.k;
    uint8_t* base = a.base + b * a.block_stride + off;
    uint2 v = make_uint2(0u, 0u);
    if (act && lane < nd && !((em >> lane) & 1ull)) v = *reinterpret_cast<const uint2*>(base + (uint64_t)lane * a.seg_stride);
    dcol[w][lane] = v;
    __syncthreads();
    // z_p = parity p ^ sum_{j received} G[p][j] d_j, lane p
    if (act && lane < a.m && ((pused >> lane) & 1ull)) {
        const uint2 pv = *reinterpret_cast<const uint2*>(base + (uint64_t)(nd + lane) * a.seg_stride);
        uint32_t z[kTailMaxBytes];
#pragma unroll
        for (uint32_t j = 0; j < kTailMaxBytes; ++j) z[j] = tail_byte(pv, j);
        const uint8_t* g = a.gen + (uint64_t)lane * a.k;
        for (uint32_t j = 0; j < nd; ++j) {
            const uint32_t gc = g[j];
            if (((em >> j) & 1ull) || gc == 0u) continue;
            tail_addmul(z, lg[gc], dcol[w][j], nbytes, ex, lg);
        }
        zrow[w][lane] = make_uint2(z[0] | (z[1] << 8) | (z[2] << 16) | (z[3] << 24), z[4] | (z[5] << 8) | (z[6] << 16));
    }
    __syncthreads();
    // d_s = sum_p coef2[row(p)][s] z_p, lane s
    if (!act || lane >= e) return;
    const uint32_t cs = a.coef_stride;
    const uint8_t* coef = a.coef2 + b * cs * cs;
    // the plan's rule (rs_plan2_kernel): blocks the fused kernel takes have the inverse by parity
    // row as snippet offsets (u16, c << 7), the others by rank as bytes
    const bool fused = a.fused_rows && e <= 16u && (pused >> a.fused_rows) == 0ull;
    uint32_t acc[kTailMaxBytes] = {0, 0, 0, 0, 0, 0, 0};
    for (uint32_t p = 0; p < a.m; ++p) {
        if (!((pused >> p) & 1ull)) continue;
        uint32_t cv;
        if (fused) {
            cv = ((uint32_t)reinterpret_cast<const uint16_t*>(coef)[(uint64_t)p * (cs / 2u) + lane] >> 7) & 255u;
        } else {
            const uint32_t t = a.pmap[b * a.m + p];
            if (t >= e) continue;  // (a used row's rank is below e: not reached)
            cv = coef[(uint64_t)t * cs + lane];
        }
        if (cv == 0u) continue;
        tail_addmul(acc, lg[cv], zrow[w][p], nbytes, ex, lg);
    }
    const uint32_t slot = a.out_slots[b * a.slots_stride + lane];
    if (slot >= nd) return;  // (erased source slots are below numData: not reached)
    tail_store(base + (uint64_t)slot * a.seg_stride, acc, nbytes, a.accumulate != 0u);
}

bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

}  // namespace

bool rs8_rt_tail_covers(const Rs8RtArgs& a, uint32_t off, uint32_t nbytes)
{
    if (nbytes == 0u || nbytes > kTailMaxBytes || (off & 7u) || !a.tab || !a.in_base || !a.out_base || a.k == 0u) return false;
    // the 8-byte loads: aligned, and inside the slot they start in
    if (!aligned8(a.in_base) || (a.in_block_stride & 7u) || (a.in_seg_stride & 7u) || (uint64_t)off + 8u > a.in_seg_stride)
        return false;
    if ((uint64_t)off + nbytes > a.out_seg_stride) return false;
    if ((reinterpret_cast<uintptr_t>(a.tab) & 1u) || (a.tab_col_stride & 1u) || (a.tab_block_stride & 1u) ||
        (a.tab_pass_stride & 1u))
        return false;
    return true;
}

int launch_rs8_rt_tail(const Rs8RtArgs& a, uint32_t off, uint32_t nbytes, hipStream_t s)
{
    if (a.nblocks == 0 || a.m == 0) return NFEC_OK;
    if (!rs8_rt_tail_covers(a, off, nbytes)) return NFEC_ENOTSUP;
    uint32_t rpg = 1;
    while (rpg < a.m && rpg < kTailThreads) rpg <<= 1;
    const uint32_t chunks = (a.m + rpg - 1u) / rpg;  // 1 below 64 rows
    const uint32_t bpw = kTailThreads / rpg;
    const uint64_t wgs = ((uint64_t)a.nblocks + bpw - 1u) / bpw * chunks;
    if (wgs >= (1ull << 31)) return NFEC_ENOTSUP;
    hipLaunchKernelGGL(gf8_rt_tail_kernel, dim3((uint32_t)wgs), dim3(kTailThreads), 0, s, a, off, nbytes, rpg, chunks);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? NFEC_OK : hip_fail(e, "rs8 runtime-coefficient tail launch");
}

bool rs8_fixed_dec_tail_covers(const Rs8FixedDecTailArgs& a, uint32_t off, uint32_t nbytes)
{
    if (nbytes == 0u || nbytes > kTailMaxBytes || (off & 7u) || a.k == 0u || a.k > 64u || a.m == 0u || a.m > 32u) return false;
    if (!a.base || !a.rows || !a.emask || !a.psel || !a.pmap || !a.out_slots || !a.coef2 || !a.gen) return false;
    if (!aligned8(a.base) || (a.block_stride & 7u) || (a.seg_stride & 7u) || (uint64_t)off + 8u > a.seg_stride) return false;
    // the inverse's two layouts: e bytes per rank row, or 16 u16 per parity row (fused)
    if (a.coef_stride < std::min(a.k, a.m) || (a.fused_rows && ((a.coef_stride & 1u) || a.coef_stride < 32u || a.fused_rows > 16u)))
        return false;
    return a.slots_stride >= std::min(a.k, a.m);
}

int launch_rs8_fixed_dec_tail(const Rs8FixedDecTailArgs& a, uint32_t off, uint32_t nbytes, hipStream_t s)
{
    if (a.nblocks == 0) return NFEC_OK;
    if (!rs8_fixed_dec_tail_covers(a, off, nbytes)) return NFEC_ENOTSUP;
    hipLaunchKernelGGL(rs8_fixed_dec_tail_kernel, dim3((a.nblocks + kFixWaves - 1u) / kFixWaves), dim3(64 * kFixWaves), 0, s,
                       a, off, nbytes);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? NFEC_OK : hip_fail(e, "rs8 fixed-shape repair tail launch");
}

}  // namespace nfec
