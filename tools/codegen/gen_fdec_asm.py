#!/usr/bin/env python3
"""Generate norm_amd/csrc/gen_fdec_asm.hip: fused RS8 erasure repair, one wavefront per block.

The closed-form RS8 decode (same bytes as the reference's k x k inverse,
src/common/normEncoderRS8.cpp:652-757) has two linear stages:
    z_t = parity(P_t) ^ sum_{c present} G[P_t][c] * d_c         (constant generator rows)
    d_E = A^-1 z                                                (per-block e x e matrix)
The unfused path writes z to HBM between the two (gen_rs8_bitsliced.hip stage 1, then
gen_solve_asm.hip).  Here one wave owns one block, so the block's erasure pattern and its
coefficients are wave-uniform and both stages run back to back in registers:

  * stage 1 = the bit-sliced re-encode of gen_rs8_asm.py (bank-separated VGPR layout, 11-column
    load ring) over the 64 source columns plus the e used parity rows as 16 extra "columns"
    (identity coefficient on their own row).  Erased columns are neither read (their loads go
    through a descriptor with 0 records) nor computed (uniform branch).
  * stage 2 = the snippet-table solve of gen_solve_asm.py: for each row t, z_t's planes are
    copied into a fixed window and expanded into M4RM tables; for each output s the wave jumps
    into the 128-byte snippet of c[s][t], whose accumulator operands are relative to M0.
    Outputs are produced in two halves of 8 (64 accumulators in the freed load ring).
  * z never leaves the register file: the block's HBM traffic is the 48 + 16 segments read and
    the e repaired segments written.

Two kernels do this.  rs8_fdec_* (gen_fdec_asm.hip) is the layout above at 256 VGPRs (2 waves per
SIMD).  rs8_fdec3 (the fdec3 section below, written to rs8_fdec3.hip by --fdec3) runs 3 waves per
SIMD at 168 VGPRs: the load ring lives in LDS, filled by LDS-DMA, and half of z is parked there
during the solve; it takes the lane-major (64, 32) and (64, 16) batches whose segment is at most
F3_MAX_VEC bytes, the first family every other batch.

A block qualifies when e <= 16 and the used parity rows are exactly rows 0..e-1 (no parity
erasures among them: NORM's usual case); the kernel marks the blocks it repaired (rows = 0,
psel = 0) so the unfused kernels that run after it on the same stream skip them.

Usage: gen_fdec_asm.py OUT.hip [k,m ...]          (norm_amd/csrc/gen_fdec_asm.hip)
       gen_fdec_asm.py --fdec3 OUT.hip           (norm_amd/csrc/rs8_fdec3.hip)
"""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_rs8_asm import (MASKS, MULTI, NSLOT, S_MASK, TEMP, acc_reg, bank, combo_reg, ring_temps,  # noqa: E402
                         slot_regs, split, table_code, transpose)
from gen_rs8_bitsliced import bitmatrix_rows, generator  # noqa: E402

DEFAULT_SHAPES = [(64, 32), (64, 16), (64, 8)]
IN_REGS = [0, 1, 4, 5, 8, 9, 12, 13]      # compiler-placed inputs: load / store offsets
S_RET, S_EM = 56, 58                       # return address; erased-column mask (64 bit)
S_COEF2 = 60
S_LRS, S_SRS = 64, 68
S_COL, S_T = 78, 79
S_COEF1 = 80
S_SLOT = 84
S_TAB = 92                                 # s92:93 snippet table, s94:95 jump target
GPR_MODE = 0x9000                          # M0[15:12]: index SRC0 and DST
SNIP_ALIGN = 7
D_P0 = 19                                  # solve accumulators d[sl][i]: pairs 19..50 (ring)
WIN_P0 = 51                                # solve window: pairs 51..54
NCOLS_PAR = 16                             # parity rows handled as extra columns


def d_reg(sl, i):
    return 4 * (D_P0 + 4 * sl + i // 2) + (i & 1)


def win_regs():
    w = []
    for q in range(4):
        w += [4 * (WIN_P0 + q), 4 * (WIN_P0 + q) + 1]
    return w


def solve_pool():
    """transpose temporaries for the outputs (d in banks 0/1; banks 2/3 still hold z)"""
    free = list(TEMP[0]) + list(TEMP[1]) + [combo_reg(g, a) for a in MULTI for g in (0, 1)]

    def make():
        avail = list(free)

        def pick(avoid):
            for i, r in enumerate(avail):
                if bank(r) != avoid:
                    return avail.pop(i)
            return avail.pop(0)
        return pick
    return make


def all_tables(w, combo_reg=combo_reg):
    code, regs = [], [{}, {}]
    for g in (0, 1):
        single = [w[2 * t + g] for t in range(4)]
        built = {1 << t: single[t] for t in range(4)}
        for a in sorted(MULTI, key=lambda a: bin(a).count("1")):
            top = a.bit_length() - 1
            dst = combo_reg(g, a)
            code.append(f"v_xor_b32 v{dst}, v{built[a & ~(1 << top)]}, v{single[top]}")
            built[a] = dst
        regs[g] = built
    return code, regs


def snippets(regs, d_reg=d_reg):
    A, B = regs
    # 64 KiB-aligned table start: in the e = 16 solve a snippet address's low word is the table
    # address's high half packed with the u16 offset (s_pack_*_b32_b16), no extract, no add
    out = [".p2align 16"]
    for c in range(256):
        out.append(f".p2align {SNIP_ALIGN}")
        if c == 0:
            out.append("Lsnip0_%=:")
        rows = bitmatrix_rows(c) if c else [0] * 8
        for i in range(8):
            a, b = split(rows[i])
            d = d_reg(0, i)
            if a and b:
                out.append(f"v_bitop3_b32 v{d}, v{d}, v{A[a]}, v{B[b]} bitop3:0x96")
            elif a:
                out.append(f"v_xor_b32 v{d}, v{d}, v{A[a]}")
            elif b:
                out.append(f"v_xor_b32 v{d}, v{d}, v{B[b]}")
        out.append(f"s_setpc_b64 s[{S_RET}:{S_RET + 1}]")
    return out


def fdec_asm(k, m, probe=None, e16=False):
    G = generator(k, m)
    nr = min(NCOLS_PAR, m)  # z rows that can be in use (e <= m)
    L = []
    offs = ["%[o0]", "%[o1]", "%[o2]", "%[o3]"]
    soffs = ["%[s0]", "%[s1]", "%[s2]", "%[s3]"]
    ncol = k + nr
    # load records 2^31: item offsets with bit 31 set (items past the segment) read as zero
    # without a memory access; erased columns switch the records to 0
    L += [f"s_mov_b64 s[{S_LRS}:{S_LRS + 1}], %[base]", f"s_mov_b32 s{S_LRS + 2}, 0x80000000",
          f"s_mov_b32 s{S_LRS + 3}, 0x00020000",
          f"s_mov_b64 s[{S_SRS}:{S_SRS + 1}], %[base]", f"s_mov_b32 s{S_SRS + 2}, 0x80000000",
          f"s_mov_b32 s{S_SRS + 3}, 0x00020000",
          f"s_mov_b64 s[{S_EM}:{S_EM + 1}], %[em]"]
    for i, mk in enumerate(MASKS):
        L.append(f"s_mov_b32 s{S_MASK + i}, 0x{mk:08x}")
    L += [f"s_load_dwordx8 s[{S_SLOT}:{S_SLOT + 7}], %[sp], 0x0",
          f"s_load_dwordx4 s[{S_COEF1}:{S_COEF1 + 3}], %[cp], 0x0",
          f"s_getpc_b64 s[{S_TAB}:{S_TAB + 1}]",
          "Lpc_%=:",
          f"s_add_u32 s{S_TAB}, s{S_TAB}, Lsnip0_%=-Lpc_%=",
          f"s_addc_u32 s{S_TAB + 1}, s{S_TAB + 1}, 0"]

    def loads(c):
        """column c: source slot c (c < k) or parity row c - k (slot c); unused ones read nothing"""
        if probe == "noload":
            return []
        w = slot_regs(c % NSLOT)
        if c < k:
            out = [f"s_bitcmp1_b64 s[{S_EM}:{S_EM + 1}], {c}", f"s_cselect_b32 s{S_LRS + 2}, 0, 0x80000000"]
        else:  # parity row c - k: read when the block uses it (bit of the parity-row mask)
            out = [f"s_bitcmp1_b32 %[ps], {c - k}", f"s_cselect_b32 s{S_LRS + 2}, 0x80000000, 0"]
        if c < k:
            out.append(f"s_mul_i32 s{S_COL}, %[ss], {c}")
        else:  # (slot numData + t: a shortened block's parity follows its numData sources)
            out += [f"s_add_u32 s{S_COL}, %[pk], {c - k}", f"s_mul_i32 s{S_COL}, s{S_COL}, %[ss]"]
        for q in range(4):
            out.append(f"buffer_load_dwordx2 v[{w[2 * q]}:{w[2 * q + 1]}], {offs[q]}, s[{S_LRS}:{S_LRS + 3}], s{S_COL} offen{LPOL}")
        return out

    for r in range(16):
        for i in range(8):
            L.append(f"v_mov_b32 v{acc_reg(r, i)}, 0")
    issued = -1
    for c in range(min(NSLOT, ncol)):
        L += loads(c)
        issued = c
    # ---- stage 1: z_t for rows 0..15 (rows >= e are computed but unused) ----
    if probe == "prio1":
        L.append("s_setprio 2")  # A/B: the loading stage ahead of the other wave's solve
    for c in range(ncol):
        w = slot_regs(c % NSLOT)
        if probe != "noload":
            L.append(f"s_waitcnt vmcnt({4 * (issued - c)})")
        if probe == "nos1":
            for i in range(8):  # keep the loaded data live
                L.append(f"v_xor_b32 v{acc_reg(0, i)}, v{w[i]}, v{acc_reg(0, i)}")
        elif c < k:
            L += [f"s_bitcmp1_b64 s[{S_EM}:{S_EM + 1}], {c}", f"s_cbranch_scc1 Lskip{c}_%="]
            L += transpose(w, ring_temps())
            ups, need = [], [set(), set()]
            for r in range(nr):
                mat = bitmatrix_rows(G[r][c])
                for i in range(8):
                    a, b = split(mat[i])
                    ups.append((acc_reg(r, i), a, b))
                    if a:
                        need[0].add(a)
                    if b:
                        need[1].add(b)
            L += table_code(w, need)
            A, B = need
            for acc, a, b in ups:
                if a and b:
                    L.append(f"v_bitop3_b32 v{acc}, v{acc}, v{A[a]}, v{B[b]} bitop3:0x96")
                elif a:
                    L.append(f"v_xor_b32 v{acc}, v{A[a]}, v{acc}")
                elif b:
                    L.append(f"v_xor_b32 v{acc}, v{B[b]}, v{acc}")
        else:
            t = c - k
            L += [f"s_bitcmp0_b32 %[ps], {t}", f"s_cbranch_scc1 Lskip{c}_%="]
            L += transpose(w, ring_temps())
            for i in range(8):
                L.append(f"v_xor_b32 v{acc_reg(t, i)}, v{w[i]}, v{acc_reg(t, i)}")
        L.append(f"Lskip{c}_%=:")
        if probe and probe.startswith("sync") and ((c + 1) % int(probe[4:]) == 0 or c + 1 == ncol):
            # A/B: keep the workgroup's four waves (four blocks) within N columns of each other,
            # so they stream the same stage-1 code through the instruction cache
            L.append("s_barrier")
        if c + NSLOT < ncol:
            L += loads(c + NSLOT)
            issued = c + NSLOT
    # ---- stage 2: d_s = sum_t c[s][t] z_t, outputs in two halves of 8 ----
    if probe == "prio1":
        L.append("s_setprio 0")
    if probe == "prio2":
        L.append("s_setprio 2")  # A/B: the solve ahead of the other wave's loading stage
    win = win_regs()
    cbuf = [S_COEF1, S_COEF2]
    tmp = [4 * (WIN_P0 + p) + h for p in range(4) for h in (0, 1)]
    regs = all_tables(win)[1]

    def stage2(x, full):
        """x: label suffix; full: the block has e = 16 (then every output is live and the used
        parity rows are 0..15), so the per-output and per-row bound checks are left out, and the
        snippet addresses add only their low word (the wave checked that no offset carries).
        The plan writes each coefficient as its snippet's byte offset (u16, c << 7); row t holds
        16 of them (32 bytes), half h loads its 8 (16 bytes at 32 t + 16 h)."""
        S = []
        for h in range(2):
            if h == 1 and not full:
                S.extend(["s_cmp_le_u32 %[e], 8", "s_cbranch_scc1 Ldone_%="])
            for sl in range(8):
                for i in range(8):
                    S.append(f"v_mov_b32 v{d_reg(sl, i)}, 0")
            for t in range(0 if probe == "nos2" else 16):
                if not full:
                    S.extend([f"s_cmp_le_u32 %[tmax], {t}", f"s_cbranch_scc1 Lrows{h}{x}_%="])
                cur = cbuf[t % 2]
                S.append("s_waitcnt lgkmcnt(0)")
                # next coefficient row (after row 15: row 0 again, for the second half)
                nt = (t + 1) % 16
                S.append(f"s_load_dwordx4 s[{cbuf[nt % 2]}:{cbuf[nt % 2] + 3}], %[cp], 0x{32 * nt + 16 * h:x}")
                for i in range(8):
                    S.append(f"v_mov_b32 v{win[i]}, v{acc_reg(t, i)}")
                S.extend(all_tables(win)[0])
                S.extend([f"s_mov_b32 s{S_T}, 0", f"s_set_gpr_idx_on s{S_T}, gpr_idx(SRC0,DST)"])
                for sl in range(8):
                    s = 8 * h + sl
                    if not full:
                        S.extend([f"s_cmp_le_u32 %[e], {s}", f"s_cbranch_scc1 Lsend{h}_{t}{x}_%="])
                    if full:
                        op = "s_pack_lh_b32_b16" if sl % 2 == 0 else "s_pack_hh_b32_b16"
                        S.append(f"{op} s{S_TAB + 2}, s{cur + sl // 2}, s{S_TAB}")
                    else:
                        S.extend([f"s_bfe_u32 s{S_T}, s{cur + sl // 2}, 0x{(16 << 16) | (16 * (sl % 2)):x}",
                                  f"s_add_u32 s{S_TAB + 2}, s{S_TAB}, s{S_T}",
                                  f"s_addc_u32 s{S_TAB + 3}, s{S_TAB + 1}, 0"])
                    S.extend([f"s_movk_i32 m0, 0x{GPR_MODE | (16 * sl):x}",
                              f"s_swappc_b64 s[{S_RET}:{S_RET + 1}], s[{S_TAB + 2}:{S_TAB + 3}]"])
                S.extend([f"Lsend{h}_{t}{x}_%=:", "s_set_gpr_idx_off"])
            S.append(f"Lrows{h}{x}_%=:")
            # the coefficient row that leaving early left in flight must land before the next half
            S.append("s_waitcnt lgkmcnt(0)")
            if h == 0:
                # the next half starts at row 0, which must sit in buffer 0
                S.append(f"s_load_dwordx4 s[{S_COEF1}:{S_COEF1 + 3}], %[cp], 0x10")
            for sl in range(8):
                s = 8 * h + sl
                if not full:
                    S.extend([f"s_cmp_le_u32 %[e], {s}",
                              "s_cbranch_scc1 Ldone_%=" if h == 1 else f"s_cbranch_scc1 Lhalf{h}{x}_%="])
                w = [d_reg(sl, i) for i in range(8)]
                S.extend(transpose(w, solve_pool()))
                S.extend([f"s_bfe_u32 s{S_T}, s{S_SLOT + s // 2}, 0x{(16 << 16) | (16 * (s % 2)):x}",
                          f"s_mul_i32 s{S_T}, s{S_T}, %[ss]",
                          "s_cmp_eq_u32 %[acc], 0", f"s_cbranch_scc1 Lna{s}{x}_%="])
                for q in range(4):
                    S.append(f"buffer_load_dwordx2 v[{tmp[2 * q]}:{tmp[2 * q + 1]}], {soffs[q]}, s[{S_SRS}:{S_SRS + 3}], s{S_T} offen")
                S.append("s_waitcnt vmcnt(0)")
                for q in range(4):
                    S.append(f"v_xor_b32 v{w[2 * q]}, v{tmp[2 * q]}, v{w[2 * q]}")
                    S.append(f"v_xor_b32 v{w[2 * q + 1]}, v{tmp[2 * q + 1]}, v{w[2 * q + 1]}")
                S.append(f"Lna{s}{x}_%=:")
                for q in range(4):
                    S.append(f"buffer_store_dwordx2 v[{w[2 * q]}:{w[2 * q + 1]}], {soffs[q]}, s[{S_SRS}:{S_SRS + 3}], s{S_T} offen{SPOL}")
            if h == 0:
                S.append(f"Lhalf{h}{x}_%=:")
        return S

    if e16:
        # the e = 16 copy packs a snippet address from the table address's high half and the
        # offset: taken when the table starts at a 64 KiB boundary in memory
        L += ["s_cmp_eq_u32 %[e], 16", "s_cbranch_scc0 Lgen_%=",
              f"s_mov_b32 s{S_TAB + 3}, s{S_TAB + 1}", f"s_and_b32 s{S_T}, s{S_TAB}, 0xffff",
              f"s_cmp_lg_u32 s{S_T}, 0", "s_cbranch_scc1 Lgen_%="]
        L += stage2("f", True)
        L += ["s_branch Ldone_%=", "Lgen_%=:"]
    L += stage2("", False)
    L.append("Ldone_%=:")
    L.append("s_waitcnt lgkmcnt(0)")
    L.append("s_branch Lend_%=")
    L += snippets(regs)
    L.append("Lend_%=:")
    return L


def clobbers():
    v = [f'"v{i}"' for i in range(256) if i not in IN_REGS]
    s = [f'"s{i}"' for i in range(S_RET, 96)]
    return ", ".join(v + s + ['"m0"', '"scc"', '"memory"'])


# A/B probes of the (64, 32) kernel, NFEC_FDEC_VARIANT=<id> (never the default): no stage-2 solve,
# no stage-1 arithmetic (loads only), no stage-1 loads, no e = 16 specialisation of stage 2
# (measured: 1.992 ms without it, 1.981 with it, 64k blocks)
# Also generable (add to PROBES): "prio1" (stage 1 at issue priority 2: 2.12-2.14 ms, slower) and
# "prio2" (stage 2 at priority 2: 1.993-1.996 ms, no change against 1.989-1.992).
# "dephase" / "dephase2" (first-generation second workgroups start 30 / 17 us late, so the two
# waves of a SIMD do not ramp their loads in phase): 1.999-2.002 / 1.984-1.987 ms against
# 1.983-1.986, no gain; generable, not built.
PROBES = {1: "nos2", 2: "nos1", 3: "noload", 4: "gen", 5: "sync4", 6: "sync8", 7: "sync16", 8: "sync80",
          9: "persist"}
# "persist" (A/B): a grid of 1,024 workgroups whose waves loop over the blocks (no wave launch
# and prologue per block, no tail of partly filled workgroups)


def persist_kernel(K, nr, body, k):
    """the fused repair as a persistent loop: each wave walks blocks w, w + 4 * gridDim.x, ...;
    the item offsets are the same for every block (o doubles as the store offsets)"""
    return f"""__global__ __launch_bounds__(256, 2) void {K}(FdecArgs a)
{{
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t l4 = (a.ips + 3u) / 4u;
    if (lane >= l4) return;  // lane-major items (lane_major 2 only in this probe)
    uint32_t o[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {{
        const uint32_t item = (uint32_t)q * l4 + lane;
        o[q] = item < a.ips ? item * 8u : 0x80000000u;
    }}
    const uint32_t stride = gridDim.x * 4u;
    for (uint32_t blk = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)); blk < a.nblocks;
         blk += stride) {{
        const int32_t rows = (int32_t)__builtin_amdgcn_readfirstlane((uint32_t)a.rows[blk]);
        const uint32_t ps0 = __builtin_amdgcn_readfirstlane(a.psel[2 * (uint64_t)blk]);
        const uint32_t ps1 = __builtin_amdgcn_readfirstlane(a.psel[2 * (uint64_t)blk + 1]);
        if (rows <= 0 || rows > 16 || ps1 != 0 || (ps0 >> {nr}) != 0u) continue;
        const uint32_t e = (uint32_t)rows;
        const uint32_t tmax = 32u - (uint32_t)__builtin_clz(ps0);
        const uint64_t em = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane(a.emask[2 * (uint64_t)blk]) |
                            ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane(a.emask[2 * (uint64_t)blk + 1]) << 32);
        const uint32_t pk = a.num_data ? __builtin_amdgcn_readfirstlane((uint32_t)a.num_data[blk]) : {k}u;
        if (lane == 0) {{
            a.rows[blk] = 0;
            a.psel[2 * (uint64_t)blk] = 0;
        }}
        const uint8_t* base = a.base + (uint64_t)blk * a.block_stride;
        const uint8_t* cp = a.coef + (uint64_t)blk * a.coef_block_stride;
        const uint16_t* sp = a.out_slots + (uint64_t)blk * a.slots_stride;
        asm volatile(
            "{body}\\n"
            :
            : [base] "s"(base), [em] "s"(em), [cp] "s"(cp), [sp] "s"(sp), [e] "s"(e), [ss] "s"(a.seg_stride),
              [acc] "s"(a.accumulate), [ps] "s"(ps0), [tmax] "s"(tmax), [pk] "s"(pk),
              [o0] "v"(o[0]), [o1] "v"(o[1]), [o2] "v"(o[2]), [o3] "v"(o[3]),
              [s0] "v"(o[0]), [s1] "v"(o[1]), [s2] "v"(o[2]), [s3] "v"(o[3])
            : {clobbers()});
    }}
}}
"""


def gen_kernel(k, m, probe=None):
    K = f"rs8_fdec_k{k}_m{m}" + (f"_probe_{probe}" if probe else "")
    nr = min(NCOLS_PAR, m)
    # e = 16 blocks (every output live) get a copy of stage 2 without the bound checks; m < 16
    # codes never have them
    asm = fdec_asm(k, m, None if probe in ("gen", "dephase", "dephase2", "persist") else probe,
                   e16=((probe in (None, "prio1", "prio2", "dephase", "dephase2", "persist") or probe.startswith("sync"))
                        and nr == 16))
    # A/B probe: the first generation's second workgroup per CU (dispatch order 256..511) starts
    # ~half (dephase) / ~a quarter (dephase2) of a block later, so the two waves of a SIMD stop
    # ramping their loads in phase
    nsleep = {"dephase": 9, "dephase2": 5}.get(probe, 0)
    dephase = (f"    if (blockIdx.x >= 256u && blockIdx.x < 512u)\n"
               f"        for (int i = 0; i < {nsleep}; ++i) __builtin_amdgcn_s_sleep(127);\n") if nsleep else ""
    body = "\\n\"\n        \"".join(asm)
    if probe == "persist":
        return persist_kernel(K, nr, body, k)
    wg = "bs::wg_index(a.xcd_remap)" if F3_PRODUCT["xcd"] else "blockIdx.x"
    return f"""__global__ __launch_bounds__(256, 2) void {K}(FdecArgs a)
{{
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t blk = __builtin_amdgcn_readfirstlane({wg} * 4 + (threadIdx.x >> 6));
    if (blk >= a.nblocks) return;
{dephase}    const int32_t rows = (int32_t)__builtin_amdgcn_readfirstlane((uint32_t)a.rows[blk]);
    const uint32_t ps0 = __builtin_amdgcn_readfirstlane(a.psel[2 * (uint64_t)blk]);
    const uint32_t ps1 = __builtin_amdgcn_readfirstlane(a.psel[2 * (uint64_t)blk + 1]);
    // qualifies: 1..16 source erasures repaired from parity rows below {nr} (the z rows this
    // kernel computes); the plan then wrote the inverse by parity row, zero for unused rows
    if (rows <= 0 || rows > 16 || ps1 != 0 || (ps0 >> {nr}) != 0u) return;
    const uint32_t e = (uint32_t)rows;
    const uint32_t tmax = 32u - (uint32_t)__builtin_clz(ps0);  // highest used parity row + 1
    // (readfirstlane yields int: widen through uint32_t, or bit 31 would sign-extend into the
    // high word)
    const uint64_t em = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane(a.emask[2 * (uint64_t)blk]) |
                        ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane(a.emask[2 * (uint64_t)blk + 1]) << 32);
    // the block's parity slot 0: numData (a shortened block; the plan put its columns
    // [numData, k) into em, so they are neither read nor computed), else k
    const uint32_t pk = a.num_data ? __builtin_amdgcn_readfirstlane((uint32_t)a.num_data[blk]) : {k}u;
    // hand the block off: the unfused stage 1 and solve that follow on the stream skip it
    if (lane == 0) {{
        a.rows[blk] = 0;
        a.psel[2 * (uint64_t)blk] = 0;
    }}
    // lane-major items: a 1400-byte segment occupies lanes 0..43 and the lanes past it drop out
    // of every instruction (EXEC) instead of computing garbage bytes, a third of the lane work.
    // lane_major 1: lane L holds items 4L..4L+3 (strided loads; measured slower, off);
    // lane_major 2: item q*L4 + L with L4 = ceil(items / 4), so each load stays contiguous
    const uint32_t l4 = (a.ips + 3u) / 4u;
    if ((a.lane_major == 1u && lane * 4u >= a.ips) || (a.lane_major == 2u && lane >= l4)) return;
    uint32_t o[4], so[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {{
        const uint32_t item = a.lane_major == 1u   ? lane * 4u + (uint32_t)q
                              : a.lane_major == 2u ? (uint32_t)q * l4 + lane
                                                   : (uint32_t)q * 64u + lane;
        const bool ok = item < a.ips;
        o[q] = ok ? item * 8u : 0x80000000u;  // past the load records: zeros, no memory access
        so[q] = ok ? item * 8u : 0x80000000u;  // past the store descriptor's records: dropped
    }}
    const uint8_t* base = a.base + (uint64_t)blk * a.block_stride;
    const uint8_t* cp = a.coef + (uint64_t)blk * a.coef_block_stride;
    const uint16_t* sp = a.out_slots + (uint64_t)blk * a.slots_stride;
    asm volatile(
        "{body}\\n"
        :
        : [base] "s"(base), [em] "s"(em), [cp] "s"(cp), [sp] "s"(sp), [e] "s"(e), [ss] "s"(a.seg_stride),
          [acc] "s"(a.accumulate), [ps] "s"(ps0), [tmax] "s"(tmax), [pk] "s"(pk),
          [o0] "v"(o[0]), [o1] "v"(o[1]), [o2] "v"(o[2]), [o3] "v"(o[3]),
          [s0] "v"(so[0]), [s1] "v"(so[1]), [s2] "v"(so[2]), [s3] "v"(so[3])
        : {clobbers()});
}}
"""


# ---- fdec3: the same repair at 168 VGPRs (3 waves per SIMD), source columns through an LDS ring ----
# Register map, quads P = 0..41 (v4P..v4P+3; bank = index mod 4):
#   v0, v1            left to the compiler: the lane's DMA offset (16 * lane) and LDS address
#   P1..P11  b0/b1    M4RM combinations (A in bank 0, B in bank 1)
#   P12..P15 b0/b1    column set X, P16..P19 column set Y: one holds the column, the other serves as
#                     its transpose temporaries and then receives the next column from LDS
#   P0..P31  b2/b3    z rows 8..15 (the rows stage 2 parks in LDS; its d accumulators replace them)
#   P20..P41 b0/b1 and P32..P41 b2/b3: z rows 0..7 (stay in registers through the solve)
# LDS: a static region of F3_WAVE_LDS bytes per wave, private to it (no barriers): in stage 1 a ring
# of F3_NSLOT raw source columns filled by LDS-DMA, a slot being the segment as it lies in memory.
# 160 KiB per CU / 3 workgroups = 54,613 B; 4 * 13,312 = 53,248 B is the largest multiple of the
# allocation granule (512 B or 1,280 B) below it that splits four ways into 16-byte multiples.
# 13,312 B = 8 rows * 8 planes * 4 B * 52 lanes, so l4 <= 52: segments of up to 1,664 B.
F3_VGPRS = 168
F3_MAX_VEC = 1664
F3_SLOT = F3_MAX_VEC
F3_NSLOT = 8
F3_WAVE_LDS = F3_SLOT * F3_NSLOT
F3_LDS_BUDGET = (160 * 1024 // 3) // 1280 * 1280
F3_IN = [0, 1]
F3_COMBO_P0, F3_SET_P0, F3_ZLO_P0, F3_ZHI_P0 = 1, 12, 20, 32
S3_EX, S3_BASE = 52, 54                    # saved EXEC; the block's base address
F3_PARK = 8 * (F3_MAX_VEC // 32)           # bytes of one parked plane pair: 8 per lane, 52 lanes
# NFEC_FDEC_VARIANT ids (diagnostic library, with NFEC_FDEC3=0 so that the batch reaches
# launch_rs8_fused_decode): fdec3's own probes (no solve / DMA, waits and LDS reads only / no DMA)
F3_PROBES = {10: "nos2", 11: "nos1", 12: "noload"}
# ... and the stream variants (F3_FLAGS), each as the whole kernel and as its load-only probe
# ("dfs": the stores at the default policy, the stream before round 20 made them non-temporal)
F3_VARIANTS = {20: (("xcd",), None), 21: (("xcd",), "nos1"), 22: (("ntl",), None), 23: (("ntl",), "nos1"),
               24: (("dfs",), None), 25: (("dfs",), "nos1"), 26: (("pair",), None), 27: (("pair",), "nos1"),
               28: (("quad",), None), 29: (("quad",), "nos1"), 30: (("xcd", "pair"), None), 31: (("xcd", "pair"), "nos1"),
               34: (("sc1s",), None), 35: (("sc1s",), "nos1"), 36: (("sc1l",), None), 37: (("sc1l",), "nos1"),
               38: (("sysnts",), None), 39: (("sysnts",), "nos1")}
assert 4 * F3_WAVE_LDS <= F3_LDS_BUDGET and F3_WAVE_LDS % 16 == 0


def f3_combo(g, a):
    return 4 * (F3_COMBO_P0 + MULTI.index(a)) + g


def f3_set(x):
    return [4 * (F3_SET_P0 + 4 * x + q) + h for q in range(4) for h in (0, 1)]


def f3_d(sl, i):
    """solve accumulators: in the registers of z row 8 + sl, 16 apart (M0-relative in the snippets)"""
    return 4 * (4 * sl + i // 2) + 2 + (i & 1)


def f3_acc(r, i):
    if r >= 8:
        return 4 * (4 * (r - 8) + i // 2) + 2 + (i & 1)
    j = 8 * r + i
    if j < 44:
        return 4 * (F3_ZLO_P0 + j // 2) + (j & 1)
    j -= 44
    return 4 * (F3_ZHI_P0 + j // 2) + 2 + (j & 1)


F3_BLOCKS = []   # instruction runs that recur (transposes, table builds, ...): candidates for
#                  a macro of their own in the compact form


def f3_blk(lines):
    if tuple(lines) not in F3_BLOCKS:
        F3_BLOCKS.append(tuple(lines))
    return lines


def f3_temps(regs):
    """transpose temporaries out of regs (banks 0 and 1 only), per transpose stage"""
    def make():
        avail = {0: [r for r in regs if bank(r) == 0], 1: [r for r in regs if bank(r) == 1]}

        def pick(avoid):
            return avail[1 if avoid == 0 else 0].pop(0)
        return pick
    return make


# Generator options of the fdec3 stream (profiles/r20/dma_stream).  F3_PRODUCT
# is what rs8_fdec3.hip is generated with; the diagnostic library builds the others as variants:
#   xcd     workgroup -> block through bs::wg_index(a.xcd_remap): each XCD a contiguous block range
#   lpol    cache-policy suffix of the column DMA (" nt"), spol: of the repaired-row stores
#   refill  columns re-armed together: 1 = one slot per step; R = R adjacent columns (contiguous in
#           memory when seg_stride == vec) back to back at every R-th step, R slots at a time
F3_PRODUCT = {"xcd": False, "lpol": "", "spol": " nt", "refill": 1}
F3_FLAGS = {"xcd": {"xcd": True}, "ntl": {"lpol": " nt"}, "dfs": {"spol": ""},
            "pair": {"refill": 2}, "quad": {"refill": 4},
            "sc1l": {"lpol": " sc1"}, "sc1s": {"spol": " sc1"}, "sysnts": {"spol": " sc0 sc1 nt"}}


def f3_opt(flags=()):
    opt = dict(F3_PRODUCT)
    for f in flags:
        opt.update(F3_FLAGS[f])
    return opt


def fdec3_stage1(k, m, probe=None, opt=None):
    """z rows 0..15 into f3_acc.  The arithmetic is fdec_asm's; a column comes HBM -> LDS by two
    buffer_load_dwordx4 ... lds pieces (lanes 0..63 bytes 0..1023, the rest at offset 1024, EXEC
    widened to the piece's lanes) through a descriptor that starts at the segment and has vec
    records (0 for a column that is not read), so the range check is the hardware's, per dword:
    the last piece of a 1,400-byte segment is half inside it and reads nothing past it.  16-byte
    pieces from 8-byte aligned segments: buffer loads need dword alignment only.
    Ordering, all within the wave: a slot is read (ds_read_b64) after the counted vmcnt that
    retires its DMA, and re-armed after the lgkmcnt(0) that returned its reads.  With refill R > 1
    the slots of columns c - R + 1 .. c are re-armed together behind column c's lgkmcnt(0), c = R - 1
    (mod R); every vmcnt still follows from the last column issued."""
    opt = opt or F3_PRODUCT
    R, lpol = opt["refill"], opt["lpol"]
    G = generator(k, m)
    nr = min(NCOLS_PAR, m)
    ncol = k + nr
    assert F3_NSLOT % R == 0 and ncol % R == 0 and R < F3_NSLOT
    L = [f"s_mov_b64 s[{S3_EX}:{S3_EX + 1}], exec",
         f"s_mov_b64 s[{S3_BASE}:{S3_BASE + 1}], %[base]",
         f"s_mov_b32 s{S_LRS + 3}, 0x00020000", f"s_mov_b32 s{S_SRS + 3}, 0x00020000",
         f"s_mov_b64 s[{S_EM}:{S_EM + 1}], %[em]"]
    for i, mk in enumerate(MASKS):
        L.append(f"s_mov_b32 s{S_MASK + i}, 0x{mk:08x}")
    L += [f"s_load_dwordx8 s[{S_SLOT}:{S_SLOT + 7}], %[sp], 0x0",
          f"s_load_dwordx4 s[{S_COEF1}:{S_COEF1 + 3}], %[cp], 0x0"]
    qoff = [None, "%[q1]", "%[q2]", "%[q3]"]

    def dma(c):
        if probe == "noload":
            return []
        if c < k:
            out = [f"s_bitcmp1_b64 s[{S_EM}:{S_EM + 1}], {c}", f"s_cselect_b32 s{S_LRS + 2}, 0, %[vec]",
                   f"s_mul_i32 s{S_COL}, %[ss], {c}"]
        else:
            out = [f"s_bitcmp1_b32 %[ps], {c - k}", f"s_cselect_b32 s{S_LRS + 2}, %[vec], 0",
                   f"s_add_u32 s{S_COL}, %[pk], {c - k}", f"s_mul_i32 s{S_COL}, s{S_COL}, %[ss]"]
        # (an M0 write needs one wait state before the LDS-DMA that reads it: the EXEC write)
        out += [f"s_add_u32 s{S_LRS}, s{S3_BASE}, s{S_COL}", f"s_addc_u32 s{S_LRS + 1}, s{S3_BASE + 1}, 0",
                f"s_add_u32 m0, %[wb], {(c % F3_NSLOT) * F3_SLOT}",
                "s_mov_b64 exec, %[dm0]",
                f"buffer_load_dwordx4 %[dma], s[{S_LRS}:{S_LRS + 3}], 0 offen{lpol} lds",
                "s_mov_b64 exec, %[dm1]",
                f"buffer_load_dwordx4 %[dma], s[{S_LRS}:{S_LRS + 3}], 0 offen offset:1024{lpol} lds",
                "s_mov_b64 exec, %[live]"]
        return out

    def lds_read(c):
        w = f3_set(c % 2)
        out = []
        for q in range(4):
            if q:
                out.append(f"v_add_u32 v{w[2 * q]}, {qoff[q]}, %[lds]")
            addr = f"v{w[2 * q]}" if q else "%[lds]"
            out.append(f"ds_read_b64 v[{w[2 * q]}:{w[2 * q + 1]}], {addr} offset:{(c % F3_NSLOT) * F3_SLOT}")
        return out

    for r in range(16):
        for i in range(8):
            L.append(f"v_mov_b32 v{f3_acc(r, i)}, 0")
    issued = -1
    for c in range(min(F3_NSLOT, ncol)):
        L += dma(c)
        issued = c
    L.append("s_mov_b64 exec, %[live]")
    if probe != "noload":
        L.append(f"s_waitcnt vmcnt({2 * issued})")
    L += lds_read(0)
    for c in range(ncol):
        w, other = f3_set(c % 2), f3_set((c + 1) % 2)
        L.append("s_waitcnt lgkmcnt(0)")  # column c is in its set (and slot c % F3_NSLOT is free)
        if c % R == R - 1 and c + F3_NSLOT < ncol:
            for n in range(c + F3_NSLOT - R + 1, c + F3_NSLOT + 1):
                L += dma(n)
            issued = c + F3_NSLOT
        if probe != "noload" and c + 1 < ncol:
            L.append(f"s_waitcnt vmcnt({2 * (issued - c - 1)})")
        skip = ([f"s_bitcmp1_b64 s[{S_EM}:{S_EM + 1}], {c}"] if c < k else [f"s_bitcmp0_b32 %[ps], {c - k}"])
        ups, pre = [], []
        if probe == "nos1":
            ups = [f"v_xor_b32 v{f3_acc(8, i)}, v{w[i]}, v{f3_acc(8, i)}" for i in range(8)]
        elif c < k:
            pre = f3_blk(transpose(w, f3_temps(other)))
            need = [set(), set()]
            todo = []
            for r in range(nr):
                mat = bitmatrix_rows(G[r][c])
                for i in range(8):
                    a, b = split(mat[i])
                    todo.append((f3_acc(r, i), a, b))
                    if a:
                        need[0].add(a)
                    if b:
                        need[1].add(b)
            pre += f3_blk(table_code(w, need, f3_combo))
            A, B = need
            for acc, a, b in todo:
                if a and b:
                    ups.append(f"v_bitop3_b32 v{acc}, v{acc}, v{A[a]}, v{B[b]} bitop3:0x96")
                elif a:
                    ups.append(f"v_xor_b32 v{acc}, v{A[a]}, v{acc}")
                elif b:
                    ups.append(f"v_xor_b32 v{acc}, v{B[b]}, v{acc}")
        else:
            pre = f3_blk(transpose(w, f3_temps(other)))
            ups = [f"v_xor_b32 v{f3_acc(c - k, i)}, v{w[i]}, v{f3_acc(c - k, i)}" for i in range(8)]
        if probe != "nos1":
            L += skip + [f"s_cbranch_scc1 Lrd{c}_%="]
        L += pre
        L.append(f"Lrd{c}_%=:")
        # the other set's transpose temporaries are dead: it takes the next column during the updates
        if c + 1 < ncol:
            L += lds_read(c + 1)
        if probe != "nos1":
            L += skip + [f"s_cbranch_scc1 Lskip{c}_%="]
        L += ups
        L.append(f"Lskip{c}_%=:")
    return L


def fdec3_stage2(e16, probe=None, opt=None):
    """fdec_asm's solve with z rows 8..15 parked in the wave's LDS region (the ring is dead: every
    DMA retired, every read returned) and the d accumulators in their registers.  Row t's planes
    reach the window by v_mov, from the row's registers (t < 8) or from the staging set, which a
    parked row's four ds_read_b64 fill one row ahead, behind the previous row's calls.  The store
    offsets are recomputed per half; the store descriptor starts at the output's segment and has
    vec records, so items past the segment are dropped by the range check."""
    spol = (opt or F3_PRODUCT)["spol"] or SPOL
    win, stg = f3_set(0), f3_set(1)
    so = [f3_combo(0, a) for a in MULTI[:4]]
    free = [f3_combo(g, a) for a in MULTI for g in (0, 1) if f3_combo(g, a) not in so]
    regs = all_tables(win, f3_combo)[1]
    cbuf = [S_COEF1, S_COEF2]

    def pool():
        avail = list(free)
        return lambda avoid: avail.pop(0)

    S = ["s_cmp_le_u32 %[tmax], 8", "s_cbranch_scc1 Lnopark_%="]
    for r in range(8, 16):
        for j in range(4):
            S.append(f"ds_write_b64 %[lds], v[{f3_acc(r, 2 * j)}:{f3_acc(r, 2 * j + 1)}] offset:{(4 * (r - 8) + j) * F3_PARK}")
    S += ["s_waitcnt lgkmcnt(0)", "Lnopark_%=:", f"s_mov_b32 s{S_SRS + 2}, %[vec]",
          f"s_getpc_b64 s[{S_TAB}:{S_TAB + 1}]", "Lpc_%=:",
          f"s_add_u32 s{S_TAB}, s{S_TAB}, Lsnip0_%=-Lpc_%=", f"s_addc_u32 s{S_TAB + 1}, s{S_TAB + 1}, 0"]

    def solve(x, full):
        """as fdec_asm's stage2(x, full)"""
        S = []
        for h in range(2):
            if h == 1 and not full:
                S.extend(["s_cmp_le_u32 %[e], 8", "s_cbranch_scc1 Ldone_%="])
            S.extend(f3_blk([f"v_mov_b32 v{f3_d(sl, i)}, 0" for sl in range(8) for i in range(8)]))
            for t in range(0 if probe == "nos2" else 16):
                if not full:
                    S.extend([f"s_cmp_le_u32 %[tmax], {t}", f"s_cbranch_scc1 Lrows{h}{x}_%="])
                cur = cbuf[t % 2]
                S.append("s_waitcnt lgkmcnt(0)")
                nt = (t + 1) % 16
                S.append(f"s_load_dwordx4 s[{cbuf[nt % 2]}:{cbuf[nt % 2] + 3}], %[cp], 0x{32 * nt + 16 * h:x}")
                for i in range(8):
                    S.append(f"v_mov_b32 v{win[i]}, v{f3_acc(t, i) if t < 8 else stg[i]}")
                if 8 <= t + 1 < 16:
                    for q in range(4):
                        S.append(f"ds_read_b64 v[{stg[2 * q]}:{stg[2 * q + 1]}], %[lds] offset:{(4 * (t - 7) + q) * F3_PARK}")
                S.extend(f3_blk(all_tables(win, f3_combo)[0]))
                S.extend([f"s_mov_b32 s{S_T}, 0", f"s_set_gpr_idx_on s{S_T}, gpr_idx(SRC0,DST)"])
                for sl in range(8):
                    s = 8 * h + sl
                    if not full:
                        S.extend([f"s_cmp_le_u32 %[e], {s}", f"s_cbranch_scc1 Lsend{h}_{t}{x}_%="])
                    if full:
                        op = "s_pack_lh_b32_b16" if sl % 2 == 0 else "s_pack_hh_b32_b16"
                        S.append(f"{op} s{S_TAB + 2}, s{cur + sl // 2}, s{S_TAB}")
                    else:
                        S.extend([f"s_bfe_u32 s{S_T}, s{cur + sl // 2}, 0x{(16 << 16) | (16 * (sl % 2)):x}",
                                  f"s_add_u32 s{S_TAB + 2}, s{S_TAB}, s{S_T}",
                                  f"s_addc_u32 s{S_TAB + 3}, s{S_TAB + 1}, 0"])
                    S.extend([f"s_movk_i32 m0, 0x{GPR_MODE | (16 * sl):x}",
                              f"s_swappc_b64 s[{S_RET}:{S_RET + 1}], s[{S_TAB + 2}:{S_TAB + 3}]"])
                S.extend([f"Lsend{h}_{t}{x}_%=:", "s_set_gpr_idx_off"])
            S.append(f"Lrows{h}{x}_%=:")
            S.append("s_waitcnt lgkmcnt(0)")
            if h == 0:
                S.append(f"s_load_dwordx4 s[{S_COEF1}:{S_COEF1 + 3}], %[cp], 0x10")
            S.append(f"v_subrev_u32 v{so[0]}, %[wb], %[lds]")
            for q in range(1, 4):
                S.append(f"v_add_u32 v{so[q]}, %[q{q}], v{so[0]}")
            for sl in range(8):
                s = 8 * h + sl
                if not full:
                    S.extend([f"s_cmp_le_u32 %[e], {s}",
                              "s_cbranch_scc1 Ldone_%=" if h == 1 else f"s_cbranch_scc1 Lhalf{h}{x}_%="])
                w = [f3_d(sl, i) for i in range(8)]
                S.extend(f3_blk(transpose(w, pool)))
                S.extend([f"s_bfe_u32 s{S_T}, s{S_SLOT + s // 2}, 0x{(16 << 16) | (16 * (s % 2)):x}",
                          f"s_mul_i32 s{S_T}, s{S_T}, %[ss]",
                          f"s_add_u32 s{S_SRS}, s{S3_BASE}, s{S_T}", f"s_addc_u32 s{S_SRS + 1}, s{S3_BASE + 1}, 0",
                          "s_cmp_eq_u32 %[acc], 0", f"s_cbranch_scc1 Lna{s}{x}_%="])
                for q in range(4):
                    S.append(f"buffer_load_dwordx2 v[{win[2 * q]}:{win[2 * q + 1]}], v{so[q]}, s[{S_SRS}:{S_SRS + 3}], 0 offen")
                S.append("s_waitcnt vmcnt(0)")
                for q in range(4):
                    S.append(f"v_xor_b32 v{w[2 * q]}, v{win[2 * q]}, v{w[2 * q]}")
                    S.append(f"v_xor_b32 v{w[2 * q + 1]}, v{win[2 * q + 1]}, v{w[2 * q + 1]}")
                S.append(f"Lna{s}{x}_%=:")
                for q in range(4):
                    S.append(f"buffer_store_dwordx2 v[{w[2 * q]}:{w[2 * q + 1]}], v{so[q]}, s[{S_SRS}:{S_SRS + 3}], 0 offen{spol}")
            if h == 0:
                S.append(f"Lhalf{h}{x}_%=:")
        return S

    if e16:
        S += ["s_cmp_eq_u32 %[e], 16", "s_cbranch_scc0 Lgen_%=",
              f"s_mov_b32 s{S_TAB + 3}, s{S_TAB + 1}", f"s_and_b32 s{S_T}, s{S_TAB}, 0xffff",
              f"s_cmp_lg_u32 s{S_T}, 0", "s_cbranch_scc1 Lgen_%="]
        S += solve("f", True)
        S += ["s_branch Ldone_%=", "Lgen_%=:"]
    S += solve("", False)
    S += ["Ldone_%=:", "s_waitcnt lgkmcnt(0)", f"s_mov_b64 exec, s[{S3_EX}:{S3_EX + 1}]", "s_branch Lend_%="]
    S += snippets(regs, f3_d)
    S.append("Lend_%=:")
    return S


# The fdec3 source is committed in a compact form: an instruction of one of these shapes is
# written as a call of a preprocessor macro that expands to its text, several to a line (the
# straight-line body is 26k instructions; as plain strings it is 1.6 MB).  {i}: a number.
F3_FORMS = [
    ("B", "v_bitop3_b32 v{0}, v{0}, v{1}, v{2} bitop3:0x96"),
    ("S", "v_bitop3_b32 v{0}, s{1}, v{2}, v{0} bitop3:0xca"),
    ("X", "v_xor_b32 v{0}, v{1}, v{2}"),
    ("R", "v_lshrrev_b32 v{0}, {1}, v{2}"),
    ("L", "v_lshlrev_b32 v{0}, {1}, v{2}"),
    ("M", "v_mov_b32 v{0}, v{1}"),
    ("Z", "v_mov_b32 v{0}, 0"),
    ("MK", "s_movk_i32 m0, {0}"),
    ("SW", f"s_swappc_b64 s[{S_RET}:{S_RET + 1}], s[{S_TAB + 2}:{S_TAB + 3}]"),
    ("RT", f"s_setpc_b64 s[{S_RET}:{S_RET + 1}]"),
    ("AC", "s_addc_u32 s{0}, s{1}, 0"),
    ("AD", "s_add_u32 s{0}, s{1}, s{2}"),
    ("BF", "s_bfe_u32 s{0}, s{1}, {2}"),
    ("CE", "s_cmp_le_u32 %[e], {0}"),
    ("PA", ".p2align {0}"),
    ("PL", "s_pack_lh_b32_b16 s{0}, s{1}, s{2}"),
    ("PH", "s_pack_hh_b32_b16 s{0}, s{1}, s{2}"),
    ("DR", "ds_read_b64 v[{0}:{1}], v{2} offset:{3}"),
    ("DL", "ds_read_b64 v[{0}:{1}], %[lds] offset:{2}"),
    ("VA", "v_add_u32 v{0}, %[q{1}], %[lds]"),
    ("WL", "s_waitcnt lgkmcnt({0})"),
    ("WV", "s_waitcnt vmcnt({0})"),
    ("BL", f"buffer_load_dwordx2 v[{{0}}:{{1}}], v{{2}}, s[{S_SRS}:{S_SRS + 3}], 0 offen"),
    ("BS", f"buffer_store_dwordx2 v[{{0}}:{{1}}], v{{2}}, s[{S_SRS}:{S_SRS + 3}], 0 offen{F3_PRODUCT['spol']}"),
]


def f3_form_nargs(fmt):
    return 1 + max([int(x) for x in re.findall(r"\{(\d)\}", fmt)], default=-1)


def f3_defines(forms=None):
    """forms: another kernel's instruction shapes (gen_rs8_d2.py), default fdec3's"""
    out = []
    for name, fmt in forms or F3_FORMS:
        n = f3_form_nargs(fmt)
        text = '"' + re.sub(r"\{(\d)\}", lambda mt: '" #' + "abcd"[int(mt.group(1))] + ' "', fmt) + '\\n"'
        text = text.replace(' ""', "").replace('"" ', "")
        args = "(" + ", ".join("abcd"[:n]) + ")" if n else ""
        out.append(f"#define {name}{args} {text}")
    # U<r>: the eight updates of z row r (accumulators fixed), arguments: the A and B entry of each
    prm = "abcdefghijklmnop"
    for r in range(16):
        out.append(f"#define U{r}({', '.join(prm)}) " +
                   " ".join(f"B({f3_acc(r, i)}, {prm[2 * i]}, {prm[2 * i + 1]})" for i in range(8)))
    return out


def f3_compact(lines, width=200, forms=None):
    """-> (defines, body): the asm lines as macro calls and string literals, packed into source
    lines; a registered run of instructions that occurs more than once becomes a macro K<n>"""
    lines = list(lines)
    defs = []
    for blk in sorted(F3_BLOCKS, key=len, reverse=True):
        n = len(blk)
        hits = [i for i in range(len(lines) - n + 1) if lines[i] == blk[0] and tuple(lines[i:i + n]) == blk]
        if len(hits) < 2 or n < 8:
            continue
        name = f"K{len(defs)}"
        defs.append(f"#define {name} \\\n    " + " \\\n    ".join(f3_compact_lines(blk, width, forms)))
        for i in reversed(hits):
            lines[i:i + n] = [f"\0{name}"]
    return defs, f3_compact_lines(lines, width, forms)


def f3_compact_lines(lines, width, forms=None):
    pats = []
    for name, fmt in forms or F3_FORMS:
        seen, rx = set(), ""
        for part in re.split(r"(\{\d\})", fmt):
            if re.fullmatch(r"\{\d\}", part):
                rx += f"(?P=a{part[1]})" if part in seen else f"(?P<a{part[1]}>0x[0-9a-f]+|[0-9]+)"
                seen.add(part)
            else:
                rx += re.escape(part)
        pats.append((name, fmt, re.compile(rx)))
    toks = []
    for ln in lines:
        if ln.startswith("\0"):
            toks.append(ln[1:])
            continue
        for name, fmt, rx in pats:
            mt = rx.fullmatch(ln)
            if mt:
                n = f3_form_nargs(fmt)
                args = [mt.group(f"a{i}") for i in range(n)]
                assert fmt.format(*args) == ln
                toks.append(name + ("(" + ",".join(args) + ")" if n else ""))
                break
        else:
            assert '"' not in ln and "\\" not in ln
            toks.append(f'"{ln}\\n"')
    rows = {tuple(str(f3_acc(r, i)) for i in range(8)): r for r in range(16)}
    i = 0
    while i + 8 <= len(toks):
        run = [re.fullmatch(r"B\((\d+),(\d+),(\d+)\)", t) for t in toks[i:i + 8]]
        r = rows.get(tuple(mt.group(1) for mt in run)) if all(run) else None
        if r is None:
            i += 1
            continue
        toks[i:i + 8] = [f"U{r}(" + ",".join(f"{mt.group(2)},{mt.group(3)}" for mt in run) + ")"]
        i += 1
    out, cur = [], ""
    for t in toks:
        if cur and len(cur) + 1 + len(t) > width:
            out.append(cur)
            cur = ""
        cur += (" " if cur else "") + t
    out.append(cur)
    return out


def f3_clobbers():
    v = [f'"v{i}"' for i in range(F3_VGPRS) if i not in F3_IN]
    s = [f'"s{i}"' for i in range(S3_EX, 96)]
    return ", ".join(v + s + ['"m0"', '"scc"', '"memory"'])


def f3_name(k, m, flags=(), probe=None):
    """rs8_fdec3_*: the kernel and its probes; rs8_f3s_*: a stream variant (and its probe)"""
    return (f"rs8_f3s_k{k}_m{m}_" + "_".join(flags) if flags else f"rs8_fdec3_k{k}_m{m}") + (f"_probe_{probe}" if probe else "")


def gen_kernel3(k, m, probe=None, compact=False, flags=()):
    """the fdec3 kernel of (k, m), or one of its timing probes (diagnostic library; their
    outputs are wrong on purpose); flags: the F3_FLAGS of a stream variant (diagnostic library)"""
    K = f3_name(k, m, flags, probe)
    nr = min(NCOLS_PAR, m)
    opt = f3_opt(flags)
    asm = fdec3_stage1(k, m, None if probe == "nos2" else probe, opt) + fdec3_stage2(nr == 16, probe, opt)
    wg = "bs::wg_index(a.xcd_remap)" if opt["xcd"] else "blockIdx.x"
    if compact:
        defs, packed = f3_compact(asm)
        body = "\n        ".join(packed)
    else:
        body = '"' + "\\n\"\n        \"".join(asm) + '\\n"'
    return ("\n".join(defs) + "\n" if compact else "") + f"""__global__ __launch_bounds__(256, 3) void {K}(FdecArgs a)
{{
    __shared__ __attribute__((aligned(16))) uint8_t ring[4 * {F3_WAVE_LDS}];
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t blk = {wg} * 4 + wave;
    if (blk >= a.nblocks) return;
    const int32_t rows = (int32_t)__builtin_amdgcn_readfirstlane((uint32_t)a.rows[blk]);
    const uint32_t ps0 = __builtin_amdgcn_readfirstlane(a.psel[2 * (uint64_t)blk]);
    const uint32_t ps1 = __builtin_amdgcn_readfirstlane(a.psel[2 * (uint64_t)blk + 1]);
    if (rows <= 0 || rows > 16 || ps1 != 0 || (ps0 >> {nr}) != 0u) return;
    const uint32_t e = (uint32_t)rows;
    const uint32_t tmax = 32u - (uint32_t)__builtin_clz(ps0);
    const uint64_t em = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane(a.emask[2 * (uint64_t)blk]) |
                        ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane(a.emask[2 * (uint64_t)blk + 1]) << 32);
    const uint32_t pk = a.num_data ? __builtin_amdgcn_readfirstlane((uint32_t)a.num_data[blk]) : {k}u;
    if (lane == 0) {{
        a.rows[blk] = 0;
        a.psel[2 * (uint64_t)blk] = 0;
    }}
    // lane-major items (lane_major 2): lane L < l4 holds items q * l4 + L.  All 64 lanes enter the
    // statement: it narrows EXEC to the l4 live lanes itself and widens it around the DMA pieces
    // (16 bytes per lane: n16 lanes in all, 64 in the first piece), whose offsets every lane needs
    const uint32_t l4 = (a.ips + 3u) / 4u;
    const uint32_t n16 = (a.vec + 15u) / 16u;
    const uint32_t n1 = n16 > 64u ? n16 - 64u : 1u;
    const uint64_t live = (1ull << l4) - 1ull;
    const uint64_t dm0 = n16 >= 64u ? ~0ull : (1ull << n16) - 1ull;
    const uint64_t dm1 = (1ull << n1) - 1ull;
    const uint32_t wb = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint8_t*)ring + wave * {F3_WAVE_LDS}u;
    const uint32_t dma = lane * 16u;
    const uint32_t lds = wb + lane * 8u;
    const uint8_t* base = a.base + (uint64_t)blk * a.block_stride;
    const uint8_t* cp = a.coef + (uint64_t)blk * a.coef_block_stride;
    const uint16_t* sp = a.out_slots + (uint64_t)blk * a.slots_stride;
    asm volatile(
        {body}
        :
        : [base] "s"(base), [em] "s"(em), [cp] "s"(cp), [sp] "s"(sp), [e] "s"(e), [ss] "s"(a.seg_stride),
          [acc] "s"(a.accumulate), [ps] "s"(ps0), [tmax] "s"(tmax), [pk] "s"(pk), [vec] "s"(a.vec),
          [live] "s"(live), [dm0] "s"(dm0), [dm1] "s"(dm1), [wb] "s"(wb),
          [q1] "s"(l4 * 8u), [q2] "s"(l4 * 16u), [q3] "s"(l4 * 24u),
          [dma] "v"(dma), [lds] "v"(lds)
        : {f3_clobbers()});
}}
"""


LPOL = SPOL = ""   # cache-policy suffixes (main: --nt-loads / --nt-stores)


def main_fdec3(path):
    """norm_amd/csrc/rs8_fdec3.hip: the fdec3 kernel in the compact form and its launcher.  One
    kernel serves (64, 32) and (64, 16): both compute z rows 0..15 and the first 16 generator
    rows of the two codes are the same (checked here).  (64, 8) stays on rs8_fdec_k64_m8."""
    k = 64
    assert [list(r) for r in generator(k, 32)[:16]] == [list(r) for r in generator(k, 16)[:16]]
    assert fdec3_stage1(k, 32) == fdec3_stage1(k, 16)
    parts = [
        "// GENERATED by tools/codegen/gen_fdec_asm.py --fdec3 -- do not edit by hand.",
        "// Fused RS8 erasure repair at 3 waves per SIMD (168 VGPRs, LDS column ring, z rows 8..15 parked",
        "// in LDS during the solve; DESIGN.md section 4) for k = 64, m = 32 or 16.  The assembly is written",
        "// with one macro per instruction shape; each expands to the instruction's text.",
        '#include "nfec_internal.hpp"',
    ] + (['#include "bitslice.hpp"'] if F3_PRODUCT["xcd"] else []) + [
        "",
        "namespace nfec {",
        "namespace {",
    ] + f3_defines() + [gen_kernel3(k, 32, compact=True)] + [f"#undef {n}" for n, _ in F3_FORMS] + [f"#undef U{r}" for r in range(16)] + [
        "}  // namespace",
        "",
        "// NFEC_ENOTSUP when the batch is not this kernel's (launch_rs8_fused_decode takes it then): it",
        "// needs lane-major items and a segment that fits the per-wave LDS region",
        "int launch_rs8_fdec3(uint32_t k, uint32_t m, const FdecArgs& a, hipStream_t s)",
        "{",
        f"    if (k != {k} || (m != 32 && m != 16) || a.lane_major != 2u || a.vec > {F3_MAX_VEC}u ||",
        "        !rs8_fused_decode_covers(k, m, a))",
        "        return NFEC_ENOTSUP;",
        "    if (a.nblocks == 0) return NFEC_OK;",
        f"    hipLaunchKernelGGL(rs8_fdec3_k{k}_m32, dim3((a.nblocks + 3) / 4), dim3(256), 0, s, a);",
        "    return hipGetLastError() == hipSuccess ? NFEC_OK : NFEC_EDEVICE;",
        "}",
        "",
        "}  // namespace nfec",
    ]
    open(path, "w").write("\n".join(parts) + "\n")


def main():
    # --diag: also emit the A/B probes and their NFEC_FDEC_VARIANT switch (the diagnostic
    # library, make -C norm_amd diag); the product library ships the default kernels only.
    # --nt-loads / --nt-stores: non-temporal column loads / repaired-row stores (A/B builds)
    global LPOL, SPOL
    if "--fdec3" in sys.argv:
        return main_fdec3([a for a in sys.argv if a != "--fdec3"][1])
    diag = "--diag" in sys.argv
    LPOL = " nt" if "--nt-loads" in sys.argv else ""
    SPOL = " nt" if "--nt-stores" in sys.argv else ""
    argv = [a for a in sys.argv if a not in ("--diag", "--nt-loads", "--nt-stores")]
    path = argv[1]
    shapes = DEFAULT_SHAPES
    if len(argv) > 2:
        shapes = [tuple(int(v) for v in s.split(",")) for s in argv[2:]]
    parts = [
        "// GENERATED by tools/codegen/gen_fdec_asm.py -- do not edit by hand.",
        "// Fused RS8 erasure repair (re-encode + e x e solve in registers, one wave per block) for",
        "// (k, m) in: " + ", ".join(f"({k},{m})" for k, m in shapes),
        "#include <cstdlib>",
        '#include "nfec_internal.hpp"',
    ] + (['#include "bitslice.hpp"'] if diag or F3_PRODUCT["xcd"] else []) + [
        "",
        "namespace nfec {",
        "namespace {",
    ]
    for k, m in shapes:
        parts.append(gen_kernel(k, m))
        if diag and (k, m) == (64, 32):
            for probe in PROBES.values():
                parts.append(gen_kernel(k, m, probe))
            for probe in F3_PROBES.values():
                parts.append(gen_kernel3(k, m, probe))
            for flags, probe in F3_VARIANTS.values():
                parts.append(gen_kernel3(k, m, probe, flags=flags))
    parts.append("}  // namespace")
    parts.append("")
    if diag:
        parts.append("static int fdec_variant()")
        parts.append("{")
        parts.append("    static const int v = [] { const char* e = std::getenv(\"NFEC_FDEC_VARIANT\"); return e ? std::atoi(e) : 0; }();")
        parts.append("    return v;")
        parts.append("}")
        parts.append("")
    parts.append("// true when launch_rs8_fused_decode runs a kernel for this shape and layout (the plan then")
    parts.append("// writes the inverse of the blocks it will take by parity row)")
    parts.append("bool rs8_fused_decode_covers(uint32_t k, uint32_t m, const FdecArgs& a)")
    parts.append("{")
    parts.append("    if ((a.vec & 7u) || a.vec > 2048 || a.coef_col_stride != 32 || (a.coef_block_stride & 15) ||")
    parts.append("        (a.slots_stride & 1) || (uint64_t)a.seg_stride * (k + 16) + a.vec >= (1ull << 31))")
    parts.append("        return false;")
    parts.append("    return " + " || ".join(f"(k == {k} && m == {m})" for k, m in shapes) + ";")
    parts.append("}")
    parts.append("")
    parts.append("// NFEC_ENOTSUP when (k, m) has no fused kernel or the batch shape needs the unfused path")
    parts.append("int launch_rs8_fused_decode(uint32_t k, uint32_t m, const FdecArgs& a, hipStream_t s)")
    parts.append("{")
    parts.append("    if (a.nblocks == 0) return NFEC_OK;")
    parts.append("    if (!rs8_fused_decode_covers(k, m, a)) return NFEC_ENOTSUP;")
    for v, probe in (PROBES.items() if diag else ()):
        parts.append(f"    if (k == 64 && m == 32 && fdec_variant() == {v}) {{")
        grid = "std::min((a.nblocks + 3) / 4, 1024u)" if probe == "persist" else "(a.nblocks + 3) / 4"
        parts.append(f"        hipLaunchKernelGGL(rs8_fdec_k64_m32_probe_{probe}, dim3({grid}), dim3(256), 0, s, a);")
        parts.append("        return hipGetLastError() == hipSuccess ? NFEC_OK : NFEC_EDEVICE;")
        parts.append("    }")
    for v, probe in (F3_PROBES.items() if diag else ()):
        parts.append(f"    if (k == 64 && m == 32 && fdec_variant() == {v} && a.lane_major == 2u && a.vec <= {F3_MAX_VEC}u) {{")
        parts.append(f"        hipLaunchKernelGGL(rs8_fdec3_k64_m32_probe_{probe}, dim3((a.nblocks + 3) / 4), dim3(256), 0, s, a);")
        parts.append("        return hipGetLastError() == hipSuccess ? NFEC_OK : NFEC_EDEVICE;")
        parts.append("    }")
    for v, (flags, probe) in (F3_VARIANTS.items() if diag else ()):
        name = f3_name(64, 32, flags, probe)
        parts.append(f"    if (k == 64 && m == 32 && fdec_variant() == {v} && a.lane_major == 2u && a.vec <= {F3_MAX_VEC}u) {{")
        parts.append(f"        hipLaunchKernelGGL({name}, dim3((a.nblocks + 3) / 4), dim3(256), 0, s, a);")
        parts.append("        return hipGetLastError() == hipSuccess ? NFEC_OK : NFEC_EDEVICE;")
        parts.append("    }")
    for k, m in shapes:
        parts.append(f"    if (k == {k} && m == {m}) {{")
        parts.append(f"        hipLaunchKernelGGL(rs8_fdec_k{k}_m{m}, dim3((a.nblocks + 3) / 4), dim3(256), 0, s, a);")
        parts.append("        return hipGetLastError() == hipSuccess ? NFEC_OK : NFEC_EDEVICE;")
        parts.append("    }")
    parts.append("    return NFEC_ENOTSUP;")
    parts.append("}")
    parts.append("")
    parts.append("}  // namespace nfec")
    open(path, "w").write("\n".join(parts) + "\n")


if __name__ == "__main__":
    main()
