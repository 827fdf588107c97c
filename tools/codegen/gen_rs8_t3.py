#!/usr/bin/env python3
"""Generate norm_amd/csrc/rs8_enc_t3.hip: bit-sliced RS8(64,32) encode with one Karatsuba step over
the Toeplitz core of the generator, as THREE role waves at 3 waves per SIMD.

For j >= 1 the generator of NormEncoderRS8 factors as  G[p][j] = W(y_p) * tau(k + p - j) * c_j
(x_0 = 0, x_j = a^(j-1), y_p = a^(k-1+p), W(z) = prod (z + x_l), c_j = a^-(j-1) / W'(x_j),
tau(d) = 1 / (1 + a^d)): a row scaling times a Toeplitz matrix times a column scaling.  In 16 x 16
blocks (row half P, column group g holding columns 1 + 16 g + j') the block of tau is B_(P-g), so
the two row halves by a pair of groups (h, h + 1) are the 2 x 2 block Toeplitz  [[B_-h, B_-h-1],
[B_1-h, B_-h]]  and need three block products instead of four (j0 = 1 + 16 h + j', j1 = j0 + 16):

  S1            += (B_-h[.][j'] c_j0) * u,   u = d_j0 + (c_j1 / c_j0) d_j1
  S2 (rows  0..15) += W(y_p)    (B_-h-1 + B_-h)[p][j'] c_j1 * d_j1     and G[p][0] * d_0
  S3 (rows 16..31) += W(y_16+p) (B_1-h  + B_-h)[p][j'] c_j0 * d_j0     and G[16+p][0] * d_0
  parity_p = W(y_p) S1_p + S2_p,   parity_16+p = W(y_16+p) S1_p + S3_p

Column 64 does not exist (a zero input) and column 0 lies outside the Toeplitz part: the one step
whose j1 is 64 carries column 0 in its place.  Every coefficient is a constant of the generated
code; what remains at run time is the constant multiply inside u (once per step) and the two row
scalings of S1 (once per item group).

  * roles B and C are gen_rs8_d2.py's role waves (its register map, LDS-DMA ring, parked offsets
    and epilogue): in step t role C owns column j0 and role B column j1 (column 0 in the last
    step).  Each reads its column from its ring, transposes it, writes the planes to its half of
    the double-buffered exchange, passes the step's one s_barrier and applies the column to its
    own 128 accumulators (S2 in B, S3 in C).  Own columns alternate between the two plane sets, so
    the next column's ring reads land during the updates.  In the last step role C also reads
    column 0's planes from the exchange;
  * role A loads and transposes nothing: after the step's barrier it reads both columns' planes,
    forms u in place, builds u's combinations and updates S1.  It so runs one step behind B and C:
    a buffer of the exchange written in step t is read between barriers t and t + 1 and written
    again after barrier t + 1;
  * epilogue: in rounds of two rows role A scales S1 by W(y_p) for B and by W(y_16+p) for C and
    writes both to a double-buffered hand-over area in the (dead) rings; after the round's barrier
    B and C XOR their share in and run gen_rs8_d2.py's epilogue for the rows.

Usage: gen_rs8_t3.py OUT.hip           (norm_amd/csrc/rs8_enc_t3.hip: the kernel, compact form)
       gen_rs8_t3.py OUT.hip --diag    (the diagnostic library's gen_rs8_t3.hip: the timing probes)
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_fdec_asm as F3  # noqa: E402
import gen_rs8_d2 as D2  # noqa: E402
from gen_fdec_asm import f3_acc, f3_blk, f3_combo, f3_temps  # noqa: E402
from gen_rs8_asm import split, table_code, transpose  # noqa: E402
from gen_rs8_bitsliced import EXP, bitmatrix_rows, generator, inv, mul, point  # noqa: E402
from gen_rs8_d2 import DP, EPI_ROWS, FORMS, K, M, PARK, ROWS, S_COL, S_IB, S_LRS, SLOT, TR_TEMPS, X, Y  # noqa: E402
from gen_rs8_q4 import update  # noqa: E402

NW = 3                        # role waves per workgroup: A (wave 0), B (wave 1), C (wave 2)
PAIRS = 128                   # 16-byte pairs per item group, as gen_rs8_d2.py's
STEPS = K // 2
SETS = (X, Y)
ROUND = 2                     # rows per hand-over round
# LDS as gen_rs8_d2.py's, with deeper rings: 4 workgroups of 2 loading waves keep as many column
# slots in flight per CU (56 against 48) as its 6 workgroups of 2 waves with 4 slots each
NSLOT = 7                     # ring slots per loading wave
RING0 = 0                     # ring of loading wave w: RING0 + w * NSLOT * SLOT
EX0 = 2 * NSLOT * SLOT        # exchange: buffer b, loading wave w at EX0 + (2 b + w) * SLOT
PARK0 = EX0 + 2 * 2 * SLOT    # parked offsets of loading wave w
LDS_BYTES = PARK0 + 2 * PARK
assert ROWS == 16 and len(EPI_ROWS) % ROUND == 0
# 4 workgroups per CU (3 waves per SIMD) in 160 KiB at either allocation granule
assert LDS_BYTES <= 40960 and all(4 * (-(-LDS_BYTES // g) * g) <= 160 * 1024 for g in (512, 1280)), LDS_BYTES
# the hand-over area (2 buffers x 2 targets x ROUND rows of 8 planes) lies in the rings
assert 2 * 2 * ROUND * SLOT <= EX0

# timing probes (diagnostic library, NFEC_T3_VARIANT=<id>; wrong parity on purpose): VALU + LDS
# only (no DMA), memory only (DMA and stores: no arithmetic, no ring reads, no role A)
PROBES = {1: "noload", 2: "nocompute"}
# stream variants (diagnostic library, the ids after the probes'): a cache policy on the parity stores
# ("nts") or on the column DMA ("ntl"), each as the whole kernel and as its memory-only probe.  The
# assembler takes the DMA's policy only between offen and lds, a spelling the committed codegen
# tests' interpreter refuses, so "ntl" can be measured but not adopted.
POLICY = {"nts": {"spol": " nt"}, "ntl": {"lpol": " nt"}}
VARIANTS = {3: ("nts", None), 4: ("nts", "nocompute"), 5: ("ntl", None), 6: ("ntl", "nocompute")}


def ring(w, s):
    return RING0 + (w * NSLOT + s % NSLOT) * SLOT


def ex(buf, w):
    return EX0 + (2 * buf + w) * SLOT


def park(w, part):
    return PARK0 + w * PARK + 512 * part


def hand(buf, target, n):
    return RING0 + ((2 * buf + target) * ROUND + n) * SLOT


def algebra():
    """(W(y_p), c_j, tau) of the factorisation  G[p][j] = W(y_p) tau(k + p - j) c_j,  j >= 1"""
    x = [point(j) for j in range(K)]

    def prod(z, skip=None):
        out = 1
        for l in range(K):
            if l != skip:
                out = mul(out, z ^ x[l])
        return out
    Wy = [prod(point(K + p)) for p in range(M)]
    c = [None] + [mul(inv(EXP[j - 1]), inv(prod(x[j], skip=j))) for j in range(1, K)]
    return Wy, c, lambda d: inv(1 ^ EXP[d])


def plan(G):
    """-> (steps, Wy): per step its columns and the three roles' 16 coefficients.  j1 is None in
    the last step, where column 0 stands in: role B applies s2 = G[0..15][0] and role C s3x =
    G[16..31][0] to it, role A's u is d_j0 alone"""
    Wy, c, tau = algebra()
    steps = []
    for h in (0, 2):
        for jp in range(ROWS):
            j0 = 1 + ROWS * h + jp
            j1 = j0 + ROWS if j0 + ROWS < K else None
            t = [[tau(K + ROWS * d + p - 1 - jp) if K + ROWS * d + p - 1 - jp > 0 else None for p in range(ROWS)]
                 for d in (-h - 1, -h, 1 - h)]
            st = {"j0": j0, "j1": j1,
                  "s1": [mul(t[1][p], c[j0]) for p in range(ROWS)],
                  "s3": [mul(mul(Wy[ROWS + p], t[2][p] ^ t[1][p]), c[j0]) for p in range(ROWS)]}
            if j1 is None:
                st["s2"] = [G[p][0] for p in range(ROWS)]
                st["s3x"] = [G[ROWS + p][0] for p in range(ROWS)]
            else:
                st["gamma"] = mul(c[j1], inv(c[j0]))
                st["s2"] = [mul(mul(Wy[p], t[0][p] ^ t[1][p]), c[j1]) for p in range(ROWS)]
            steps.append(st)
    assert [st["j1"] for st in steps].index(None) == STEPS - 1
    return steps, Wy


def accs(r):
    return [f3_acc(r, i) for i in range(8)]


def times(coefs, w, dst, first):
    """dst[r] (8 planes each) = or ^= coefs[r] times the column whose planes are in w:
    (combination code, updates), as gen_rs8_d2.py's column()"""
    need, todo = [set(), set()], []
    for r, cf in enumerate(coefs):
        mat = bitmatrix_rows(cf)
        for i in range(8):
            a, b = split(mat[i])
            todo.append((dst[r][i], a, b))
            if a:
                need[0].add(a)
            if b:
                need[1].add(b)
    pre = f3_blk(table_code(w, need, f3_combo))
    A, B = need
    return pre, [u for u in (update(acc, A, B, a, b, first) for acc, a, b in todo) if u]


ALL = [accs(r) for r in range(ROWS)]


def role_a(G, probe=None):
    """role A: S1, one step behind the loading roles"""
    if probe == "nocompute":
        return ["s_nop 0"]
    steps, Wy = plan(G)
    L = []
    for s, st in enumerate(steps):
        L.append("s_barrier")                 # the step's planes are in exchange buffer s % 2
        both = st["j1"] is not None
        for z, w in ((X, 1), (Y, 0)) if both else ((X, 1),):
            for i in range(4):
                L.append(f"ds_read_b64 v[{z[2 * i]}:{z[2 * i + 1]}], %[la] offset:{ex(s % 2, w) + 512 * i}")
        L.append("s_waitcnt lgkmcnt(0)")
        if both:                              # u = d_j0 + gamma d_j1, in X
            pre, ups = times([st["gamma"]], Y, [X], first=False)
            L += pre + ups
        pre, ups = times(st["s1"], X, ALL, first=(s == 0))
        L += pre + ups
    # epilogue: W(y_p) S1_p for role B (through X) and W(y_16+p) S1_p for role C (through Y)
    for q in range(ROWS // ROUND):
        for n, r in enumerate(EPI_ROWS[ROUND * q:ROUND * (q + 1)]):
            for target, z in enumerate(SETS):
                pre, ups = times([Wy[ROWS * target + r]], ALL[r], [z], first=True)
                L += pre + ups
                for i in range(4):
                    L.append(f"ds_write_b64 %[la], v[{z[2 * i]}:{z[2 * i + 1]}] offset:{hand(q % 2, target, n) + 512 * i}")
        L += ["s_waitcnt lgkmcnt(0)", "s_barrier"]
    return L


def role_bc(G, w, probe=None, lpol="", spol=""):
    """role B (w = 0: rows 0..15, S2) or C (w = 1: rows 16..31, S3): ring w, exchange half w"""
    noload, nocompute = probe == "noload", probe == "nocompute"
    steps, _ = plan(G)
    cols = [(st["j1"] if st["j1"] is not None else 0) if w == 0 else st["j0"] for st in steps]
    L = D2.setup()

    def read_dp():
        return [] if noload else [f"ds_read_b64 v[{DP[0]}:{DP[1]}], %[la] offset:{park(w, 0)}"]

    def dma(s):
        """the role's column of step s into ring slot s % NSLOT (gen_rs8_d2.py's dma)"""
        if noload:
            return []
        out = [f"s_mul_i32 s{S_COL}, %[ss], {cols[s]}",
               f"s_add_u32 s{S_LRS}, s{S_IB}, s{S_COL}", f"s_addc_u32 s{S_LRS + 1}, s{S_IB + 1}, 0"]
        for p in range(2):
            out += [f"s_add_u32 m0, %[lb], {ring(w, s) + 1024 * p}", "s_nop 0",
                    f"buffer_load_dwordx4 v{DP[p]}, s[{S_LRS}:{S_LRS + 3}], 0 offen{lpol} lds"]
        return out

    def raw_read(s):
        z = SETS[s % 2]
        return [f"ds_read_b64 v[{z[2 * q]}:{z[2 * q + 1]}], %[la2] offset:{ring(w, s) + 1024 * (q // 2) + 8 * (q % 2)}"
                for q in range(4)]

    def vm_wait(s):
        return [] if noload else [f"s_waitcnt vmcnt({2 * (min(s + NSLOT - 1, STEPS - 1) - s)})"]

    if nocompute:
        L += [f"v_mov_b32 v{f3_acc(r, i)}, 0" for r in range(ROWS) for i in range(8)]
    L += read_dp()
    L.append("s_waitcnt lgkmcnt(0)")
    for s in range(NSLOT):
        L += dma(s)
    for s, st in enumerate(steps):
        if nocompute:
            L += vm_wait(s)
            if s + NSLOT < STEPS:
                L += read_dp() + ["s_waitcnt lgkmcnt(0)"] + dma(s + NSLOT)
            continue
        Z = SETS[s % 2]
        if s == 0:
            L += vm_wait(0) + raw_read(0)
        L.append("s_waitcnt lgkmcnt(0)")      # column s is in Z, ring slot s % NSLOT is free
        rearm = s + NSLOT < STEPS
        if rearm:
            L += read_dp()
        L += f3_blk(transpose(Z, f3_temps(TR_TEMPS)))
        if rearm:
            L += (["s_waitcnt lgkmcnt(0)"] if not noload else []) + dma(s + NSLOT)
        for i in range(4):
            L.append(f"ds_write_b64 %[la], v[{Z[2 * i]}:{Z[2 * i + 1]}] offset:{ex(s % 2, w) + 512 * i}")
        pre, ups = times(st["s2"] if w == 0 else st["s3"], Z, ALL, first=(s == 0))
        L += pre + ["s_waitcnt lgkmcnt(0)", "s_barrier"]
        # the other set takes the next own column (or, role C's last step, column 0) during the updates
        if s + 1 < STEPS:
            L += vm_wait(s + 1) + raw_read(s + 1)
        elif w == 1:
            O = SETS[(s + 1) % 2]
            for i in range(4):
                L.append(f"ds_read_b64 v[{O[2 * i]}:{O[2 * i + 1]}], %[la] offset:{ex(s % 2, 0) + 512 * i}")
        L += ups
        if s + 1 == STEPS and w == 1:
            pre, ups = times(st["s3x"], O, ALL, first=False)
            L += ["s_waitcnt lgkmcnt(0)"] + pre + ups
    if nocompute:
        return L + D2.epilogue(ROWS * w, w, park=park, spol=spol)

    def merge(n, r):
        """role A's share of row r: hand-over round n // ROUND"""
        out = ["s_barrier"] if n % ROUND == 0 else []
        for i in range(4):
            out.append(f"ds_read_b64 v[{Y[2 * i]}:{Y[2 * i + 1]}], %[la] offset:{hand(n // ROUND % 2, w, n % ROUND) + 512 * i}")
        out.append("s_waitcnt lgkmcnt(0)")
        return out + [f"v_xor_b32 v{a}, v{Y[i]}, v{a}" for i, a in enumerate(accs(r))]
    return L + D2.epilogue(ROWS * w, w, merge, park, spol)


def role_asm(G, role, probe=None, policy=None):
    return role_a(G, probe) if role == 0 else role_bc(G, role - 1, probe, **POLICY.get(policy, {}))


def compact_roles(roles, width=200):
    """gen_fdec_asm.py's f3_compact over several bodies that share the recurring runs' macros"""
    roles = [list(r) for r in roles]
    defs = []
    for blk in sorted(F3.F3_BLOCKS, key=len, reverse=True):
        n = len(blk)
        if n < 8:
            continue
        hits = [[i for i in range(len(ls) - n + 1) if ls[i] == blk[0] and tuple(ls[i:i + n]) == blk] for ls in roles]
        if sum(len(h) for h in hits) < 2:
            continue
        name = f"K{len(defs)}"
        defs.append(f"#define {name} \\\n    " + " \\\n    ".join(F3.f3_compact_lines(blk, width, FORMS)))
        for ls, h in zip(roles, hits):
            for i in reversed(h):
                ls[i:i + n] = [f"\0{name}"]
    return defs, [F3.f3_compact_lines(ls, width, FORMS) for ls in roles]


def gen_kernel(probe=None, compact=False, policy=None):
    G = generator(K, M)
    name = f"rs8_t3_enc_k{K}_m{M}" + (f"_{policy}" if policy else "") + (f"_probe_{probe}" if probe else "")
    asm = [role_asm(G, r, probe, policy) for r in range(NW)]
    if compact:
        defs, packed = compact_roles(asm)
        bodies = ["\n        ".join(p) for p in packed]
    else:
        defs, bodies = [], ['"' + "\\n\"\n        \"".join(a) + '\\n"' for a in asm]
    out = []
    for r in range(NW):
        out.append(f"""__device__ __forceinline__ void {name}_role{r}(const uint8_t* ib, uint8_t* ob, uint32_t ss, uint32_t acc, uint32_t lb, uint32_t la, uint32_t la2)
{{
    asm volatile(
        {bodies[r]}
        :
        : [ib] "s"(ib), [ob] "s"(ob), [ss] "s"(ss), [acc] "s"(acc), [lb] "s"(lb), [la] "v"(la), [la2] "v"(la2)
        : {D2.clobbers()});
}}""")
    out.append(f"""__global__ __launch_bounds__({64 * NW}, 3) void {name}(bs::EncArgs a)
{{
    __shared__ __attribute__((aligned(16))) uint32_t lds[{LDS_BYTES} / 4];
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // the item group: pairs g0 + p * 64 + lane (p = 0, 1) of the flat list of 16-byte pairs,
    // pps = ceil(vec / 16) per segment; all three waves work on the same pairs
    const uint32_t pps = (a.vec + 15u) >> 4, total = a.nblocks * pps;
    const uint32_t g0 = bs::wg_index(a.xcd_remap) * {PAIRS}u;
    const uint32_t b0 = __builtin_amdgcn_readfirstlane(min(g0, total - 1u) / pps);
    const uint8_t* ib = a.base + (uint64_t)b0 * a.block_stride;
    uint8_t* ob = a.out + (uint64_t)b0 * a.block_stride;
    // d: the pair's byte offset from the first block's slot 0 (DMA offset and first item's store
    // offset); h: the second item's store offset.  Bit 31 (past the descriptors' records): nothing
    // is read, the store is dropped -- pairs past the batch, and the second item of a segment's
    // last pair when vec % 16 = 8
    // parked in the loading wave's own LDS region (LDS operations of one wave complete in order,
    // so the statement's reads need no wait); wave 0 loads and stores nothing
    if (wave != 0) {{
        const uint32_t pk = {PARK0 // 4}u + (wave - 1u) * {PARK // 4}u + lane * 2u;
#pragma unroll
        for (int p = 0; p < 2; ++p) {{
            const uint32_t g = g0 + (uint32_t)p * 64u + lane, gg = g < total ? g : g0;
            const uint32_t b = gg / pps, o = (gg - b * pps) * 16u;
            const uint32_t off = (b - b0) * (uint32_t)a.block_stride + o;
            lds[pk + p] = g < total ? off : 0x80000000u;
            lds[pk + 128 + p] = g < total && o + 16u <= a.vec ? off + 8u : 0x80000000u;
        }}
    }}
    const uint32_t lb = bs::lds_addr(lds);
    const uint32_t la = lb + lane * 8u;    // plane pairs and parked offsets: 8 bytes per lane
    const uint32_t la2 = lb + lane * 16u;  // raw pairs in a ring slot: 16 bytes per lane
    if (wave == 0) {name}_role0(ib, ob, a.seg_stride, a.accumulate, lb, la, la2);
    else if (wave == 1) {name}_role1(ib, ob, a.seg_stride, a.accumulate, lb, la, la2);
    else {name}_role2(ib, ob, a.seg_stride, a.accumulate, lb, la, la2);
}}""")
    return defs, "\n\n".join(out)


def launcher(name, fn):
    return D2.launcher(name, fn).replace(f"dim3({64 * D2.NW}), 0, s, a)", f"dim3({64 * NW}), 0, s, a)")


def main():
    diag = "--diag" in sys.argv
    path = [a for a in sys.argv if a != "--diag"][1]
    name = f"rs8_t3_enc_k{K}_m{M}"
    if not diag:
        defs, kernel = gen_kernel(compact=True)
        parts = [
            "// GENERATED by tools/codegen/gen_rs8_t3.py -- do not edit by hand.",
            "// Bit-sliced RS8(64,32) encode at 3 waves per SIMD with one Karatsuba step over the generator's",
            "// Toeplitz core: role waves B and C load, transpose and share the columns (rs8_enc_d2.hip's ring",
            "// and exchange) and keep 16 rows each, role wave A keeps the 16 rows both halves have in common",
            "// (DESIGN.md section 4).  One macro per instruction shape; each expands to the instruction's text.",
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
            D2.LAUNCH_DOC.replace("the caller then runs q4", "the caller then runs d2 or q4"),
            "int launch_rs8_t3_encode(uint32_t k, uint32_t m, const bs::EncArgs& a, hipStream_t s)",
            "{",
            f"    if (k != {K} || m != {M}) return NFEC_ENOTSUP;",
            f"    return launch_{name}(a, s);",
            "}",
            "",
            "}  // namespace nfec",
        ]
    else:
        parts = [
            "// GENERATED by tools/codegen/gen_rs8_t3.py --diag -- do not edit by hand.",
            "// Diagnostic library only: the timing probes of rs8_t3_enc_k64_m32 (wrong parity on purpose).",
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
        vname = {v: f"{name}_{pol}" + (f"_probe_{probe}" if probe else "") for v, (pol, probe) in VARIANTS.items()}
        for v, (pol, probe) in VARIANTS.items():
            parts.append(gen_kernel(probe, policy=pol)[1])
            parts.append(launcher(vname[v], f"launch_{vname[v]}"))
        parts += [
            "}  // namespace",
            "",
            "// NFEC_T3_VARIANT=<id>: a timing probe instead of the kernel (0 or unset: NFEC_ENOTSUP, the kernel runs)",
            "int launch_rs8_t3_probe(uint32_t k, uint32_t m, const bs::EncArgs& a, hipStream_t s)",
            "{",
            '    static const int v = [] { const char* e = std::getenv("NFEC_T3_VARIANT"); return e ? std::atoi(e) : 0; }();',
            f"    if (k != {K} || m != {M}) return NFEC_ENOTSUP;",
        ]
        for v, probe in PROBES.items():
            parts.append(f"    if (v == {v}) return launch_{name}_probe_{probe}(a, s);")
        for v in VARIANTS:
            parts.append(f"    if (v == {v}) return launch_{vname[v]}(a, s);")
        parts += ["    return NFEC_ENOTSUP;", "}", "", "}  // namespace nfec"]
    open(path, "w").write("\n".join(parts) + "\n")


if __name__ == "__main__":
    main()
