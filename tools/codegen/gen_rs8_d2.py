#!/usr/bin/env python3
"""Generate norm_amd/csrc/rs8_enc_d2.hip: bit-sliced RS8(64,32) encode in which TWO role waves of 16
parity rows each share every source column's bit transpose through LDS, at 3 waves per SIMD.

Same arithmetic as gen_rs8_q4.py (8x8 bit transpose per source column, method of four Russians
over the constant generator of NormEncoderRS8, one v_bitop3 per parity bit-plane and column) and
the same sharing of the transposes, but a wave owns 16 rows instead of 8, so the 22 M4RM
combinations of a column are built twice per column instead of four times: 48 + 2 x 22 + 256 =
348 VALU per column against q4's 392.  128 accumulators per wave fit 3 waves per SIMD (168 VGPRs)
the way rs8_fdec3's stage 1 does (gen_fdec_asm.py, whose register map this kernel uses): the
source columns arrive by LDS-DMA in a ring of raw 2 KiB slots and take no registers.

  * a workgroup is 2 waves over the same 64 lanes x 32 bytes: lane L holds pairs g0 + L and
    g0 + 64 + L of the batch's flat list of 16-byte pairs (ceil(vec / 16) per segment; the last
    pair of a segment with vec % 16 = 8 is half valid: its second item's loaded bytes are whatever
    follows the segment and its stores are dropped);
  * in step s wave w owns column 2s + w: it reads the column from its ring slot (4 x ds_read_b64),
    transposes it (48 VALU), writes the 8 planes to its half of a double-buffered exchange slot,
    applies the column to its 16 rows, and after one s_barrier reads the partner's planes and
    applies them too;
  * ring: NSLOT slots of 2 KiB per wave, private to it (no barrier): two buffer_load_dwordx4 ...
    offen lds pieces per column (pair p of every lane at slot + 1024 p + 16 L), counted vmcnt.  A
    slot is read after the vmcnt that retires its DMA and re-armed after the lgkmcnt(0) that
    returned its reads (rs8_fdec3's rules);
  * registers: v0/v1 are left to the compiler (the lane's two LDS addresses), 22 combinations,
    column sets X (own column) and Y (partner's planes), 128 accumulators.  The lane's two DMA
    offsets and four store offsets do not fit: the C++ prologue parks them in the wave's LDS
    region, a step reads the DMA offsets back into a dead combination pair ahead of its DMA, the
    epilogue reads all four;
  * epilogue: per parity row the planes go back to bytes (optional accumulate, as q4's) and every
    whole 16-byte pair leaves by one buffer_store_dwordx4 (role_asm's epilogue comment).

Usage: gen_rs8_d2.py OUT.hip           (norm_amd/csrc/rs8_enc_d2.hip: the kernel, compact form)
       gen_rs8_d2.py OUT.hip --diag    (the diagnostic library's gen_rs8_d2.hip: the timing probes)
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_fdec_asm as F3  # noqa: E402
from gen_fdec_asm import f3_acc, f3_blk, f3_combo, f3_set, f3_temps  # noqa: E402
from gen_rs8_asm import MASKS, MULTI, S_MASK, bank, split, table_code, transpose  # noqa: E402
from gen_rs8_bitsliced import bitmatrix_rows, generator  # noqa: E402
from gen_rs8_q4 import update  # noqa: E402

K, M = 64, 32
NW = 2                        # role waves per workgroup
ROWS = M // NW
VGPRS = 168
IN = [0, 1]                   # left to the compiler
NSLOT = 4                     # ring slots per wave
SLOT = 2048                   # one column of the item group: 2 pieces x 64 lanes x 16 bytes
RING0 = 0                     # ring of wave w: RING0 + w * NSLOT * SLOT
EX0 = NW * NSLOT * SLOT       # exchange: buffer b, wave w at EX0 + (2 b + w) * SLOT
PARK0 = EX0 + 2 * NW * SLOT   # parked offsets of wave w: (d0, d1) then (h0, h1), 8 bytes per lane each
PARK = 1024
LDS_BYTES = PARK0 + NW * PARK
S_LRS, S_SRS = 64, 68         # DMA / store buffer descriptors (masks: s72..s77, gen_rs8_asm)
S_COL, S_ROW = 78, 79
S_IB = 80                     # the item group's first block (the DMA descriptor's base moves by column)
# 6 workgroups per CU (3 waves per SIMD) in 160 KiB at either allocation granule
assert all(6 * (-(-LDS_BYTES // g) * g) <= 160 * 1024 for g in (512, 1280)), LDS_BYTES

X, Y = f3_set(0), f3_set(1)
TR_TEMPS = [f3_combo(g, a) for a in MULTI[:4] for g in (0, 1)]
DP = (f3_combo(0, MULTI[4]), f3_combo(1, MULTI[4]))       # a step's DMA offsets (d0, d1)
SO_D = (f3_combo(0, MULTI[9]), f3_combo(1, MULTI[9]))     # epilogue: (d0, d1)
SO_H = (f3_combo(0, MULTI[10]), f3_combo(1, MULTI[10]))   # epilogue: (h0, h1)
SO_F = (f3_combo(0, MULTI[7]), f3_combo(1, MULTI[7]))     # epilogue: whole pairs' store offsets
SO_E = (f3_combo(0, MULTI[8]), f3_combo(1, MULTI[8]))     # epilogue: half pairs' store offsets
# epilogue staging quads v[4P:4P+3], P = 1, 2: a combination pair and, in banks 2/3, registers of row 8
QUADS = [[f3_combo(0, MULTI[p]), f3_combo(1, MULTI[p]), f3_combo(0, MULTI[p]) + 2, f3_combo(0, MULTI[p]) + 3] for p in range(2)]
EPI_ROWS = [8] + [r for r in range(ROWS) if r != 8]
EPI_FREE = [f3_combo(g, a) for a in MULTI[2:7] for g in (0, 1)]
S_HALF = 82                   # lanes that hold a half-valid pair (64-bit mask)
assert DP[1] == DP[0] + 1 and SO_D[1] == SO_D[0] + 1 and SO_H[1] == SO_H[0] + 1
assert all(q[0] % 4 == 0 and q == list(range(q[0], q[0] + 4)) for q in QUADS)

# timing probes (diagnostic library, NFEC_D2_VARIANT=<id>; wrong parity on purpose): VALU + LDS
# only (no DMA), memory only (DMA and stores, no arithmetic, no ring reads), no exchange (each
# wave reuses its own column's planes: the cost of the exchange and its barrier)
PROBES = {1: "noload", 2: "nocompute", 3: "noexch"}


def ring(w, s):
    return RING0 + (w * NSLOT + s % NSLOT) * SLOT


def ex(buf, w):
    return EX0 + (2 * buf + w) * SLOT


def park(w, part):
    return PARK0 + w * PARK + 512 * part


def epi_pool():
    avail = list(EPI_FREE)

    def pick(avoid):
        for i, r in enumerate(avail):
            if bank(r) != avoid:
                return avail.pop(i)
        return avail.pop(0)
    return pick


def column(G, r0, j, w, first):
    """(combination code, updates) of rows [r0, r0 + ROWS) by column j whose planes are in w"""
    need, todo = [set(), set()], []
    for r in range(ROWS):
        mat = bitmatrix_rows(G[r0 + r][j])
        for i in range(8):
            a, b = split(mat[i])
            todo.append((f3_acc(r, i), a, b))
            if a:
                need[0].add(a)
            if b:
                need[1].add(b)
    pre = f3_blk(table_code(w, need, f3_combo))
    A, B = need
    ups = [u for u in (update(acc, A, B, a, b, first) for acc, a, b in todo) if u]
    return pre, ups


def setup():
    """the DMA and store descriptors and the transpose masks"""
    L = [f"s_mov_b64 s[{S_IB}:{S_IB + 1}], %[ib]",
         f"s_mov_b32 s{S_LRS + 2}, 0x80000000",   # offsets with bit 31 set (pairs past the batch) read nothing
         f"s_mov_b32 s{S_LRS + 3}, 0x00020000",
         f"s_mov_b64 s[{S_SRS}:{S_SRS + 1}], %[ob]",
         f"s_mov_b32 s{S_SRS + 2}, 0x80000000",   # ... and stores there are dropped
         f"s_mov_b32 s{S_SRS + 3}, 0x00020000"]
    for i, mk in enumerate(MASKS):
        L.append(f"s_mov_b32 s{S_MASK + i}, 0x{mk:08x}")
    return L


def epilogue(r0, w, before_row=None, park=park, spol=""):
    """rows [r0, r0 + ROWS) out of the accumulators; w: whose parked offsets (park: where they lie).
    spol: cache-policy suffix of the parity stores (gen_rs8_t3.py's "nts" variant; after offen).
    before_row(n, r): code ahead of the n-th stored row r (gen_rs8_t3.py merges another wave's
    share there)"""
    L = []
    # epilogue as q4's: per row, planes back to bytes, optional accumulate, stores.  A lane's pair is
    # 16 contiguous bytes, so a whole pair goes out as one buffer_store_dwordx4 (a wave's store is
    # then 1 KiB of whole lines; two dwordx2 stores at a 16-byte lane stride would each half-fill
    # them), staged through a 4-aligned register quad: the first row stored (row 8, by dwordx2)
    # frees banks 2/3 of the quads QUADS.  The first item of a half-valid pair goes out by dwordx2,
    # behind a branch that is not taken when no lane of the wave holds one.
    so = [SO_D[0], SO_H[0], SO_D[1], SO_H[1]]   # items in X's dword-pair order: (pair 0, half 0), (0, 1), (1, 0), (1, 1)
    L += [f"ds_read_b64 v[{SO_D[0]}:{SO_D[1]}], %[la] offset:{park(w, 0)}",
          f"ds_read_b64 v[{SO_H[0]}:{SO_H[1]}], %[la] offset:{park(w, 1)}",
          "s_waitcnt lgkmcnt(0)"]
    for p in range(2):
        # whole pair: d, dropped (bit 31) unless h is valid; half pair: d, dropped unless h is not
        L += [f"v_and_or_b32 v{SO_F[p]}, v{SO_H[p]}, s{S_SRS + 2}, v{SO_D[p]}",
              f"v_not_b32 v{SO_E[p]}, v{SO_H[p]}",
              f"v_and_or_b32 v{SO_E[p]}, v{SO_E[p]}, s{S_SRS + 2}, v{SO_D[p]}",
              f"v_cmp_le_i32 vcc, 0, v{SO_E[p]}",
              f"s_mov_b64 s[{S_HALF}:{S_HALF + 1}], vcc" if p == 0 else f"s_or_b64 s[{S_HALF}:{S_HALF + 1}], s[{S_HALF}:{S_HALF + 1}], vcc"]
    for n, r in enumerate(EPI_ROWS):
        acc = [f3_acc(r, i) for i in range(8)]
        if before_row:
            L += before_row(n, r)
        L += f3_blk(transpose(acc, epi_pool))
        L += [f"s_mul_i32 s{S_ROW}, %[ss], {K + r0 + r}", "s_cmp_eq_u32 %[acc], 0", f"s_cbranch_scc1 Lnoacc{r}_%="]
        for q in range(4):
            L.append(f"buffer_load_dwordx2 v[{X[2 * q]}:{X[2 * q + 1]}], v{so[q]}, s[{S_SRS}:{S_SRS + 3}], s{S_ROW} offen")
        L.append("s_waitcnt vmcnt(0)")
        for q in range(4):
            L.append(f"v_xor_b32 v{acc[2 * q]}, v{X[2 * q]}, v{acc[2 * q]}")
            L.append(f"v_xor_b32 v{acc[2 * q + 1]}, v{X[2 * q + 1]}, v{acc[2 * q + 1]}")
        L.append(f"Lnoacc{r}_%=:")
        if n == 0:
            assert set(acc) >= {x for q in QUADS for x in q[2:]}
            for q in range(4):
                L.append(f"buffer_store_dwordx2 v[{acc[2 * q]}:{acc[2 * q + 1]}], v{so[q]}, s[{S_SRS}:{S_SRS + 3}], s{S_ROW} offen{spol}")
            continue
        for p in range(2):
            Q = QUADS[p]
            L += [f"v_mov_b32 v{Q[i]}, v{acc[4 * p + i]}" for i in range(4)]
            # (a store of more than 8 bytes needs a wait state before its data registers change)
            L += [f"buffer_store_dwordx4 v[{Q[0]}:{Q[3]}], v{SO_F[p]}, s[{S_SRS}:{S_SRS + 3}], s{S_ROW} offen{spol}", "s_nop 1"]
        L += [f"s_cmp_lg_u64 s[{S_HALF}:{S_HALF + 1}], 0", f"s_cbranch_scc0 Lnohalf{r}_%="]
        for p in range(2):
            L.append(f"buffer_store_dwordx2 v[{acc[4 * p]}:{acc[4 * p + 1]}], v{SO_E[p]}, s[{S_SRS}:{S_SRS + 3}], s{S_ROW} offen{spol}")
        L.append(f"Lnohalf{r}_%=:")
    return L


def role_asm(G, w, probe=None):
    noload, nocompute, noexch = probe == "noload", probe == "nocompute", probe == "noexch"
    r0 = w * ROWS
    steps = K // NW
    L = setup()

    def read_dp():
        return [] if noload else [f"ds_read_b64 v[{DP[0]}:{DP[1]}], %[la] offset:{park(w, 0)}"]

    def dma(s):
        """column 2s + w into ring slot s % NSLOT; DP holds the lane's pair offsets (an M0 write
        needs one wait state before the LDS-DMA that reads it)"""
        if noload:
            return []
        out = [f"s_mul_i32 s{S_COL}, %[ss], {NW * s + w}",
               f"s_add_u32 s{S_LRS}, s{S_IB}, s{S_COL}", f"s_addc_u32 s{S_LRS + 1}, s{S_IB + 1}, 0"]
        for p in range(2):
            out += [f"s_add_u32 m0, %[lb], {ring(w, s) + 1024 * p}", "s_nop 0",
                    f"buffer_load_dwordx4 v{DP[p]}, s[{S_LRS}:{S_LRS + 3}], 0 offen lds"]
        return out

    def raw_read(s):
        return [f"ds_read_b64 v[{X[2 * q]}:{X[2 * q + 1]}], %[la2] offset:{ring(w, s) + 1024 * (q // 2) + 8 * (q % 2)}"
                for q in range(4)]

    def vm_wait(s):
        """column s's DMA has retired: the later steps' pieces may still be in flight"""
        return [] if noload else [f"s_waitcnt vmcnt({2 * (min(s + NSLOT - 1, steps - 1) - s)})"]

    if nocompute:
        L += [f"v_mov_b32 v{f3_acc(r, i)}, 0" for r in range(ROWS) for i in range(8)]
    L += read_dp()
    L.append("s_waitcnt lgkmcnt(0)")
    for s in range(min(NSLOT, steps)):
        L += dma(s)
    for s in range(steps):
        if nocompute:
            L += vm_wait(s)
            if s + NSLOT < steps:
                L += read_dp() + ["s_waitcnt lgkmcnt(0)"] + dma(s + NSLOT)
            continue
        if s == 0:
            L += vm_wait(0) + raw_read(0)
        L.append("s_waitcnt lgkmcnt(0)")      # column s is in X, ring slot s % NSLOT is free
        rearm = s + NSLOT < steps
        if rearm:
            L += read_dp()
        L += f3_blk(transpose(X, f3_temps(TR_TEMPS)))
        if rearm:
            L += (["s_waitcnt lgkmcnt(0)"] if not noload else []) + dma(s + NSLOT)
        if not noexch:
            for i in range(4):
                L.append(f"ds_write_b64 %[la], v[{X[2 * i]}:{X[2 * i + 1]}] offset:{ex(s % 2, w) + 512 * i}")
        pre, ups = column(G, r0, NW * s + w, X, first=(s == 0))
        L += pre + ups
        if noexch:
            pre, ups = column(G, r0, NW * s + 1 - w, X, first=False)
            L += pre + ups
            if s + 1 < steps:
                L += vm_wait(s + 1) + raw_read(s + 1)
            continue
        L += ["s_waitcnt lgkmcnt(0)", "s_barrier"]
        for i in range(4):
            L.append(f"ds_read_b64 v[{Y[2 * i]}:{Y[2 * i + 1]}], %[la] offset:{ex(s % 2, 1 - w) + 512 * i}")
        # X is dead: it takes the next own column during the partner's updates
        if s + 1 < steps:
            L += vm_wait(s + 1) + raw_read(s + 1)
            L.append("s_waitcnt lgkmcnt(4)")
        else:
            L.append("s_waitcnt lgkmcnt(0)")
        pre, ups = column(G, r0, NW * s + 1 - w, Y, first=False)
        L += pre + ups
    return L + epilogue(r0, w)


# the committed source's compact form (gen_fdec_asm.py f3_compact): one macro per instruction shape
FORMS = [f for f in F3.F3_FORMS if f[0] in ("B", "S", "X", "R", "L", "M", "Z", "WL", "WV")] + [
    ("DL", "ds_read_b64 v[{0}:{1}], %[la] offset:{2}"),
    ("DR", "ds_read_b64 v[{0}:{1}], %[la2] offset:{2}"),
    ("DW", "ds_write_b64 %[la], v[{0}:{1}] offset:{2}"),
    ("MO", "s_add_u32 m0, %[lb], {0}"),
    ("DM", f"buffer_load_dwordx4 v{{0}}, s[{S_LRS}:{S_LRS + 3}], 0 offen lds"),
    ("BL", f"buffer_load_dwordx2 v[{{0}}:{{1}}], v{{2}}, s[{S_SRS}:{S_SRS + 3}], s{S_ROW} offen"),
    ("BS", f"buffer_store_dwordx2 v[{{0}}:{{1}}], v{{2}}, s[{S_SRS}:{S_SRS + 3}], s{S_ROW} offen"),
]


def clobbers():
    v = [f'"v{i}"' for i in range(VGPRS) if i not in IN]
    s = [f'"s{i}"' for i in range(S_LRS, S_HALF + 2)]
    return ", ".join(v + s + ['"m0"', '"vcc"', '"scc"', '"memory"'])


def gen_kernel(probe=None, compact=False):
    G = generator(K, M)
    name = f"rs8_d2_enc_k{K}_m{M}" + (f"_probe_{probe}" if probe else "")
    out, defs = [], []
    bodies = []
    for w in range(NW):
        asm = role_asm(G, w, probe)
        if compact:
            d, packed = F3.f3_compact(asm, forms=FORMS)
            bodies.append((d, "\n        ".join(packed)))
        else:
            bodies.append(([], '"' + "\\n\"\n        \"".join(asm) + '\\n"'))
    if compact:
        # the recurring runs (transposes, combination builds) are the same in both roles
        assert bodies[0][0] == bodies[1][0]
        defs = bodies[0][0]
    for w in range(NW):
        out.append(f"""__device__ __forceinline__ void {name}_role{w}(const uint8_t* ib, uint8_t* ob, uint32_t ss, uint32_t acc, uint32_t lb, uint32_t la, uint32_t la2)
{{
    asm volatile(
        {bodies[w][1]}
        :
        : [ib] "s"(ib), [ob] "s"(ob), [ss] "s"(ss), [acc] "s"(acc), [lb] "s"(lb), [la] "v"(la), [la2] "v"(la2)
        : {clobbers()});
}}""")
    out.append(f"""__global__ __launch_bounds__({64 * NW}, 3) void {name}(bs::EncArgs a)
{{
    __shared__ __attribute__((aligned(16))) uint32_t lds[{LDS_BYTES} / 4];
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // the item group: pairs g0 + p * 64 + lane (p = 0, 1) of the flat list of 16-byte pairs,
    // pps = ceil(vec / 16) per segment; both waves hold the same pairs
    const uint32_t pps = (a.vec + 15u) >> 4, total = a.nblocks * pps;
    const uint32_t g0 = bs::wg_index(a.xcd_remap) * {64 * NW}u;
    const uint32_t b0 = __builtin_amdgcn_readfirstlane(min(g0, total - 1u) / pps);
    const uint8_t* ib = a.base + (uint64_t)b0 * a.block_stride;
    uint8_t* ob = a.out + (uint64_t)b0 * a.block_stride;
    // d: the pair's byte offset from the first block's slot 0 (DMA offset and first item's store
    // offset); h: the second item's store offset.  Bit 31 (past the descriptors' records): nothing
    // is read, the store is dropped -- pairs past the batch, and the second item of a segment's
    // last pair when vec % 16 = 8
    // parked in the wave's own LDS region (LDS operations of one wave complete in order, so the
    // statement's reads need no wait)
    const uint32_t pk = {PARK0 // 4}u + wave * {PARK // 4}u + lane * 2u;
#pragma unroll
    for (int p = 0; p < 2; ++p) {{
        const uint32_t g = g0 + (uint32_t)p * 64u + lane, gg = g < total ? g : g0;
        const uint32_t b = gg / pps, o = (gg - b * pps) * 16u;
        const uint32_t off = (b - b0) * (uint32_t)a.block_stride + o;
        lds[pk + p] = g < total ? off : 0x80000000u;
        lds[pk + 128 + p] = g < total && o + 16u <= a.vec ? off + 8u : 0x80000000u;
    }}
    const uint32_t lb = bs::lds_addr(lds);
    const uint32_t la = lb + lane * 8u;    // plane pairs and parked offsets: 8 bytes per lane
    const uint32_t la2 = lb + lane * 16u;  // raw pairs in a ring slot: 16 bytes per lane
    if (wave == 0) {name}_role0(ib, ob, a.seg_stride, a.accumulate, lb, la, la2);
    else {name}_role1(ib, ob, a.seg_stride, a.accumulate, lb, la, la2);
}}""")
    return defs, "\n\n".join(out)


LAUNCH_DOC = """// NFEC_ENOTSUP for every batch that is not this kernel's (the caller then runs q4): only (64, 32),
// whole 8-byte pieces (the caller passes vec8 and runs the tail kernel), no shortened batches, no
// nontemporal stores.  Layout: a DMA piece reads 16 bytes per pair, so a half-valid last pair
// (vec % 16 = 8) reads the 8 bytes after its segment: with seg_stride >= vec they are the segment's
// padding or the start of the block's next slot, which exists for every source slot (k < k + m) --
// inside the batch as long as a block holds its k + m slots.  Offsets: an item group's 128 pairs
// span at most 128 / pps + 2 blocks; the farthest byte a descriptor addresses stays below 2^31."""


def launcher(name, fn):
    return f"""static int {fn}(const bs::EncArgs& a, hipStream_t s)
{{
    const uint64_t pps = ((uint64_t)a.vec + 15) / 16, pairs = (uint64_t)a.nblocks * pps;
    if (a.num_data || a.nt_store || a.vec == 0 || (a.vec & 7u) || a.nblocks == 0 || pairs >= (1ull << 31) ||
        a.seg_stride < a.vec || a.block_stride < (uint64_t){K + M - 1} * a.seg_stride + a.vec)
        return NFEC_ENOTSUP;
    const uint64_t span = std::min<uint64_t>(a.nblocks, {64 * NW} / pps + 2);
    if (span * a.block_stride + (uint64_t){K + M} * a.seg_stride + 16 >= (1ull << 31)) return NFEC_ENOTSUP;
    const uint64_t wgs = (pairs + {64 * NW - 1}) / {64 * NW};
    hipLaunchKernelGGL({name}, dim3((uint32_t)wgs), dim3({64 * NW}), 0, s, a);
    return hipGetLastError() == hipSuccess ? NFEC_OK : NFEC_EDEVICE;
}}"""


def main():
    diag = "--diag" in sys.argv
    path = [a for a in sys.argv if a != "--diag"][1]
    name = f"rs8_d2_enc_k{K}_m{M}"
    if not diag:
        defs, kernel = gen_kernel(compact=True)
        parts = [
            "// GENERATED by tools/codegen/gen_rs8_d2.py -- do not edit by hand.",
            "// Bit-sliced RS8(64,32) encode at 3 waves per SIMD: 2 role waves of 16 parity rows share each",
            "// column's transpose through LDS, source columns by LDS-DMA into a ring (DESIGN.md section 4).  The",
            "// assembly is written with one macro per instruction shape; each expands to the instruction's text.",
            "#include <algorithm>",
            '#include "bitslice.hpp"',
            "",
            "namespace nfec {",
            "namespace {",
        ] + F3.f3_defines(FORMS) + defs + [kernel] + [f"#undef {n}" for n, _ in FORMS] + [f"#undef U{r}" for r in range(16)] + [
            "",
            launcher(name, f"launch_{name}"),
            "}  // namespace",
            "",
            LAUNCH_DOC,
            "int launch_rs8_d2_encode(uint32_t k, uint32_t m, const bs::EncArgs& a, hipStream_t s)",
            "{",
            f"    if (k != {K} || m != {M}) return NFEC_ENOTSUP;",
            f"    return launch_{name}(a, s);",
            "}",
            "",
            "}  // namespace nfec",
        ]
    else:
        parts = [
            "// GENERATED by tools/codegen/gen_rs8_d2.py --diag -- do not edit by hand.",
            "// Diagnostic library only: the timing probes of rs8_d2_enc_k64_m32 (wrong parity on purpose).",
            "#include <algorithm>",
            "#include <cstdlib>",
            '#include "bitslice.hpp"',
            "",
            "namespace nfec {",
            "namespace {",
        ]
        for probe in PROBES.values():
            parts.append(gen_kernel(probe)[1])
            parts.append(launcher(f"{name}_probe_{probe}", f"launch_{name}_probe_{probe}"))
        parts += [
            "}  // namespace",
            "",
            "// NFEC_D2_VARIANT=<id>: a timing probe instead of the kernel (0 or unset: NFEC_ENOTSUP, the kernel runs)",
            "int launch_rs8_d2_probe(uint32_t k, uint32_t m, const bs::EncArgs& a, hipStream_t s)",
            "{",
            '    static const int v = [] { const char* e = std::getenv("NFEC_D2_VARIANT"); return e ? std::atoi(e) : 0; }();',
            f"    if (k != {K} || m != {M}) return NFEC_ENOTSUP;",
        ]
        for v, probe in PROBES.items():
            parts.append(f"    if (v == {v}) return launch_{name}_probe_{probe}(a, s);")
        parts += ["    return NFEC_ENOTSUP;", "}", "", "}  // namespace nfec"]
    open(path, "w").write("\n".join(parts) + "\n")


if __name__ == "__main__":
    main()
