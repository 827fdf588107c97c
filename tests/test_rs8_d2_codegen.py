"""Static properties of the 2-role-wave RS8(64,32) encode kernel (rs8_d2_enc_k64_m32) as
tools/codegen/gen_rs8_d2.py emits it, and its instruction stream run on a small interpreter.

The kernel exists for 3 waves per SIMD: it must fit 168 VGPRs without scratch and a sixth of a
CU's LDS, or the occupancy is lost without any GPU test failing.  The interpreter executes the
generated text of both role waves (the instruction subset the generator uses) against a batch in
host memory with the two worst-case timings of its asynchronous operations, so a wrong wait
count, LDS offset or generator coefficient shows without a GPU."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = os.path.join(ROOT, "tools", "codegen", "gen_rs8_d2.py")
sys.path.insert(0, os.path.join(ROOT, "tools", "codegen"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_rs8_d2 as d2  # noqa: E402
from gen_rs8_bitsliced import generator, mul  # noqa: E402
from test_fdec3_codegen import _expand, _vgprs  # noqa: E402

MAX_VGPR = 167                       # 512 registers per SIMD lane / 3 waves, in granules of 8: 168
KERNEL = "rs8_d2_enc_k64_m32"
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def generated(tmp_path_factory):
    d = tmp_path_factory.mktemp("d2")
    out = {}
    for name, flags in (("product", []), ("diag", ["--diag"])):
        path = str(d / f"{name}.hip")
        subprocess.run([sys.executable, GEN, path] + flags, check=True)
        out[name] = open(path).read()
    out["dir"] = str(d)
    return out


def _asm_lines(src):
    return re.findall(r'"((?:[^"\\]|\\.)*?)\\n"', src)


def _roles(text, name):
    """the asm lines of the two role functions of kernel `name`"""
    out = []
    for w in range(d2.NW):
        start = text.index(f"void {name}_role{w}(")
        out.append(_asm_lines(text[start:text.index("\n        :\n", start)]))
    return out


def test_committed_file_is_the_generator_output(generated):
    with open(os.path.join(ROOT, "norm_amd", "csrc", "rs8_enc_d2.hip")) as f:
        assert f.read() == generated["product"]
    assert len(generated["product"]) < (1 << 20)


def test_compact_form_is_the_plain_instructions(generated):
    G = generator(d2.K, d2.M)
    roles = _roles(_expand(generated["product"]), KERNEL)
    for w in range(d2.NW):
        plain = d2.role_asm(G, w)
        assert len(plain) > 10000 and roles[w] == plain, w


def test_product_has_no_probes_or_knobs(generated):
    text = generated["product"]
    assert "probe" not in text and "getenv" not in text and "VARIANT" not in text
    assert KERNEL in text and "launch_rs8_d2_encode" in text
    assert {f"{KERNEL}_probe_{p}" for p in d2.PROBES.values()} <= set(re.findall(r"void (\w+)\(bs::EncArgs", generated["diag"]))


@pytest.mark.parametrize("which", ["product", "diag"])
def test_register_and_lds_budget_of_the_source(generated, which):
    text = _expand(generated[which]) if which == "product" else generated[which]
    names = [KERNEL] if which == "product" else [f"{KERNEL}_probe_{p}" for p in d2.PROBES.values()]
    for name in names:
        for w in range(d2.NW):
            start = text.index(f"void {name}_role{w}(")
            src = text[start:text.index("\n}", start)]
            body, clob = src.split("\n        :\n")[0], src.split("\n        : ")[-1]
            used = _vgprs(body)
            assert max(used) <= MAX_VGPR, (name, max(used))
            clobbered = {int(a) for a in re.findall(r'"v(\d+)"', clob)}
            free = set(range(MAX_VGPR + 1)) - clobbered
            assert len(free) == 2 and used <= clobbered, (name, sorted(free), sorted(used - clobbered))
        mt = re.search(r"__launch_bounds__\((\d+), (\d+)\) void " + name + r"\(", text)
        assert (int(mt.group(1)), int(mt.group(2))) == (128, 3), name
    # 6 workgroups per CU (3 waves per SIMD x 4 SIMDs / 2 waves) at both candidate allocation granules
    lds = {int(x) for x in re.findall(r"__shared__[^;]*\[(\d+) / 4\];", text)}
    assert lds == {d2.LDS_BYTES}
    for granule in (512, 1280):
        assert 6 * (-(-d2.LDS_BYTES // granule) * granule) <= 160 * 1024, granule
    # every LDS offset lies inside the allocation and M0 targets stay 16-byte aligned
    for off in re.findall(r"offset:(\d+)", text):
        assert int(off) + 64 * 16 <= d2.LDS_BYTES or int(off) + 64 * 8 <= d2.LDS_BYTES, off
    for off in re.findall(r"s_add_u32 m0, %\[lb\], (\d+)", text):
        assert int(off) % 16 == 0 and int(off) + 1024 <= d2.EX0, off


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_code_object_fits_three_waves_per_simd(generated):
    """the cross-compiled kernel: at most 168 VGPRs, occupancy 3, no scratch, the LDS size above"""
    src = os.path.join(generated["dir"], "product.hip")
    asm = os.path.join(generated["dir"], "product.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-Wno-inline-asm",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "norm_amd", "csrc"), src, "-o", asm],
                   check=True)
    text = open(asm).read()
    meta = text[text.index(".amdhsa_kernel"):]

    def field(name):
        vals = re.findall(r"^\s*\." + name + r":\s*(\d+)", meta, re.M)
        assert len(vals) == 1, name
        return int(vals[0])
    assert field("vgpr_count") <= 168
    assert field("private_segment_fixed_size") == 0 and field("vgpr_spill_count") == 0 and field("sgpr_spill_count") == 0
    assert field("group_segment_fixed_size") == d2.LDS_BYTES
    assert re.findall(r"; Occupancy: (\d+)", text) == ["3"]
    assert "scratch_" not in text.split(";;#ASMSTART")[0]


# ---- the instruction stream on an interpreter ----
class _Wave:
    """one role wave: 64 lanes of VGPRs, SGPRs, its pending LDS reads and LDS-DMA pieces.
    late_dma: a DMA piece lands when the vmcnt wait retires it, else when it is issued; LDS reads
    return their data at the lgkmcnt wait that covers them in the first case and at issue in the
    second, so both a read ahead of its DMA and a DMA ahead of a slot's last read go wrong."""

    def __init__(self, lines, env, mem, lds, late_dma):
        self.lines, self.env, self.mem, self.lds, self.late = lines, env, mem, lds, late_dma
        self.v = np.zeros((168, 64), np.uint32)
        self.s = {}
        self.scc = 0
        self.m0 = 0
        self.vcc = 0
        self.vm, self.lgkm = [], []
        self.labels = {ln[:-1]: i for i, ln in enumerate(lines) if ln.endswith(":")}
        self.stores = 0

    def sval(self, t):
        if t in self.env:
            return self.env[t]
        if t.startswith("s"):
            return self.s[int(t[1:])]
        return int(t, 0) & 0xFFFFFFFF

    def vsrc(self, t):
        if t in self.env:
            t = self.env[t]
        if isinstance(t, str) and t.startswith("v"):
            return self.v[int(t[1:])]
        return np.uint32(self.sval(t))

    def vreg(self, t):
        t = self.env.get(t, t)
        return int(t[1:])

    def retire(self, q, n):
        while len(q) > n:
            q.pop(0)()

    def lds_read64(self, addr):
        out = np.zeros((2, 64), np.uint32)
        for lane in range(64):
            out[:, lane] = self.lds[addr[lane]:addr[lane] + 8].view(np.uint32)
        return out

    def desc(self, lo):
        base = self.s[lo] | ((self.s[lo + 1] & 0xFFFF) << 32)
        assert self.s[lo + 1] >> 16 == 0 and self.s[lo + 3] == 0x00020000
        return base, self.s[lo + 2]

    def run(self):
        """generator: yields at every s_barrier"""
        pc = 0
        while pc < len(self.lines):
            ln = self.lines[pc]
            pc += 1
            if ln.endswith(":"):
                continue
            op, _, rest = ln.partition(" ")
            a = [x.strip() for x in rest.split(",")] if rest else []
            if op == "s_mov_b32":
                self.s[int(a[0][1:])] = self.sval(a[1])
            elif op == "s_mov_b64":
                lo = int(a[0][2:a[0].index(":")])
                val = self.vcc if a[1] == "vcc" else self.env[a[1]]
                self.s[lo], self.s[lo + 1] = val & 0xFFFFFFFF, val >> 32
            elif op == "s_mul_i32":
                self.s[int(a[0][1:])] = (self.sval(a[1]) * self.sval(a[2])) & 0xFFFFFFFF
            elif op in ("s_add_u32", "s_addc_u32"):
                t = self.sval(a[1]) + self.sval(a[2]) + (self.scc if op == "s_addc_u32" else 0)
                self.scc = t >> 32
                if a[0] == "m0":
                    self.m0 = t & 0xFFFFFFFF
                else:
                    self.s[int(a[0][1:])] = t & 0xFFFFFFFF
            elif op == "s_cmp_eq_u32":
                self.scc = int(self.sval(a[0]) == self.sval(a[1]))
            elif op == "s_cmp_lg_u64":
                lo = int(a[0][2:a[0].index(":")])
                self.scc = int((self.s[lo] | (self.s[lo + 1] << 32)) != int(a[1], 0))
            elif op == "s_or_b64":
                lo = int(a[0][2:a[0].index(":")])
                assert a[1] == a[0] and a[2] == "vcc"
                self.s[lo], self.s[lo + 1] = self.s[lo] | (self.vcc & 0xFFFFFFFF), self.s[lo + 1] | (self.vcc >> 32)
            elif op in ("s_cbranch_scc1", "s_cbranch_scc0"):
                if self.scc == int(op[-1]):
                    pc = self.labels[a[0]]
            elif op == "v_cmp_le_i32":
                assert a[0] == "vcc"
                m = self.vsrc(a[1]).astype(np.int32) <= self.vsrc(a[2]).astype(np.int32)
                self.vcc = sum(1 << i for i in range(64) if np.broadcast_to(m, 64)[i])
            elif op == "v_not_b32":
                self.v[self.vreg(a[0])] = ~self.vsrc(a[1])
            elif op == "v_and_or_b32":
                self.v[self.vreg(a[0])] = (self.vsrc(a[1]) & self.vsrc(a[2])) | self.vsrc(a[3])
            elif op == "s_nop":
                pass
            elif op == "s_barrier":
                assert not self.lgkm, "barrier with LDS operations in flight"
                yield
            elif op == "s_waitcnt":
                mt = re.fullmatch(r"(vmcnt|lgkmcnt)\((\d+)\)", rest)
                self.retire(self.vm if mt.group(1) == "vmcnt" else self.lgkm, int(mt.group(2)))
            elif op in ("v_xor_b32", "v_lshrrev_b32", "v_lshlrev_b32", "v_mov_b32"):
                d = self.vreg(a[0])
                if op == "v_mov_b32":
                    self.v[d] = self.vsrc(a[1])
                elif op == "v_xor_b32":
                    self.v[d] = self.vsrc(a[1]) ^ self.vsrc(a[2])
                elif op == "v_lshrrev_b32":
                    self.v[d] = self.vsrc(a[2]) >> np.uint32(int(a[1]))
                else:
                    self.v[d] = self.vsrc(a[2]) << np.uint32(int(a[1]))
            elif op == "v_bitop3_b32":
                c, tt = a[3].split(" bitop3:")
                x, y, z = self.vsrc(a[1]), self.vsrc(a[2]), self.vsrc(c)
                if tt == "0x96":
                    r = x ^ y ^ z
                else:
                    assert tt == "0xca"
                    r = (x & y) | (~x & z)
                self.v[self.vreg(a[0])] = r
            elif op == "ds_read_b64":
                lo, hi = (int(x) for x in re.fullmatch(r"v\[(\d+):(\d+)\]", a[0]).groups())
                assert hi == lo + 1
                adr, off = a[1].split(" offset:")
                addr = self.vsrc(adr).astype(np.int64) + int(off)
                assert addr.min() >= 0 and addr.max() + 8 <= len(self.lds)
                self.v[lo:hi + 1] = 0xDEADBEEF   # not valid before the wait

                def land(lo=lo, addr=addr, data=None if self.late else self.lds_read64(addr)):
                    self.v[lo:lo + 2] = self.lds_read64(addr) if data is None else data
                self.lgkm.append(land)
            elif op == "ds_write_b64":
                adr, (lo, hi), off = a[0], re.fullmatch(r"v\[(\d+):(\d+)\] offset:(\d+)", a[1]).groups()[:2], a[1].split("offset:")[1]
                addr = self.vsrc(adr).astype(np.int64) + int(off)
                assert addr.min() >= 0 and addr.max() + 8 <= len(self.lds)
                for lane in range(64):
                    self.lds[addr[lane]:addr[lane] + 8] = self.v[int(lo):int(lo) + 2, lane].copy().view(np.uint8)
                self.lgkm.append(lambda: None)
            elif op == "buffer_load_dwordx4":
                assert a[-1].endswith("offen lds") and a[-1].split()[0] == "0"
                base, nrec = self.desc(int(a[1][2:a[1].index(":")]))
                voff = self.vsrc(a[0]).astype(np.int64)
                dst = self.m0
                assert dst % 16 == 0 and dst + 1024 <= len(self.lds)
                data = np.zeros((64, 16), np.uint8)
                for lane in range(64):
                    if voff[lane] + 16 <= nrec:
                        p = base + voff[lane]
                        assert 0 <= p and p + 16 <= len(self.mem), "DMA outside the batch"
                        data[lane] = self.mem[p:p + 16]

                def land(dst=dst, data=data):
                    self.lds[dst:dst + 1024] = data.reshape(-1)
                if self.late:
                    self.vm.append(land)
                else:
                    land()
                    self.vm.append(lambda: None)
            elif op in ("buffer_load_dwordx2", "buffer_store_dwordx2", "buffer_store_dwordx4"):
                lo, hi = (int(x) for x in re.fullmatch(r"v\[(\d+):(\d+)\]", a[0]).groups())
                nb = 4 * (hi - lo + 1)
                assert nb == 4 * int(op[-1]) and (nb == 8 or lo % 4 == 0)
                base, nrec = self.desc(int(a[2][2:a[2].index(":")]))
                soff = a[3].split()
                assert soff[1] == "offen"
                voff = self.vsrc(a[1]).astype(np.int64)
                for lane in range(64):
                    if voff[lane] + nb > nrec:
                        continue
                    p = base + voff[lane] + self.sval(soff[0])
                    assert 0 <= p and p + nb <= len(self.mem), "access outside the batch"
                    if op.startswith("buffer_store"):
                        self.mem[p:p + nb] = self.v[lo:hi + 1, lane].copy().view(np.uint8)
                        self.stores += nb // 8
                    else:
                        self.v[lo:lo + 2, lane] = self.mem[p:p + 8].view(np.uint32)
                self.vm.append(lambda: None)
            else:
                raise AssertionError(f"instruction outside the interpreter's subset: {ln}")
        assert not self.lgkm, "LDS operations in flight at the end"


def _run_workgroup(roles, wg, mem, base, out, nblocks, vec, seg_stride, block_stride, accumulate, late_dma, order):
    """the kernel's C++ prologue (pair offsets parked in LDS), then both role waves barrier to barrier"""
    lds = np.zeros(d2.LDS_BYTES, np.uint8)
    pps = (vec + 15) // 16
    total = nblocks * pps
    g0 = wg * 128
    b0 = min(g0, total - 1) // pps
    park = lds.view(np.uint32)
    for w in range(2):
        for lane in range(64):
            for p in range(2):
                g = g0 + 64 * p + lane
                gg = g if g < total else g0
                b, o = gg // pps, (gg % pps) * 16
                off = (b - b0) * block_stride + o
                i = d2.PARK0 // 4 + w * (d2.PARK // 4) + 2 * lane + p
                park[i] = off if g < total else 0x80000000
                park[i + 128] = off + 8 if g < total and o + 16 <= vec else 0x80000000
    waves = []
    for w in range(2):
        env = {"%[ib]": base + b0 * block_stride, "%[ob]": out + b0 * block_stride, "%[ss]": seg_stride,
               "%[acc]": accumulate, "%[lb]": 0, "%[la]": "v0", "%[la2]": "v1"}
        wv = _Wave(roles[w], env, mem, lds, late_dma)
        wv.v[0] = np.arange(64, dtype=np.uint32) * 8
        wv.v[1] = np.arange(64, dtype=np.uint32) * 16
        waves.append(wv)
    runs = [wv.run() for wv in waves]
    live = [True, True]
    while any(live):
        for w in order:
            if live[w]:
                try:
                    next(runs[w])
                except StopIteration:
                    live[w] = False
        assert live[0] == live[1], "the role waves pass different numbers of barriers"
    return sum(wv.stores for wv in waves)


def _reference(batch, k, m, vec):
    G = generator(k, m)
    tab = np.array([[mul(c, x) for x in range(256)] for c in range(256)], np.uint8)
    ref = batch.copy()
    for r in range(m):
        acc = np.zeros(batch[:, 0, :vec].shape, np.uint8)
        for j in range(k):
            acc ^= tab[G[r][j]][batch[:, j, :vec]]
        ref[:, k + r, :vec] = acc
    return ref


@pytest.mark.parametrize("vec,seg_stride,nblocks,accumulate,late_dma,order,separate_out", [
    (24, 24, 3, 0, True, (0, 1), False),        # half-valid pairs at every segment end, a partial item group
    (24, 32, 47, 0, False, (1, 0), False),      # 94 pairs over 47 blocks in one item group, padded segments
    (200, 200, 1, 1, False, (0, 1), False),     # accumulate onto nonzero parity, half-valid last pair
    (1040, 1048, 1, 0, True, (1, 0), False),    # an item group's second pair row, vec % 16 = 0
    (40, 48, 5, 1, True, (0, 1), True),         # parity (accumulated) into another buffer than the sources'
])
def test_instruction_stream_encodes(vec, seg_stride, nblocks, accumulate, late_dma, order, separate_out):
    k, m = d2.K, d2.M
    G = generator(k, m)
    roles = [d2.role_asm(G, w) for w in range(2)]
    rng = np.random.default_rng(vec * 131 + nblocks)
    pad = 40                                      # the batch starts 8 mod 16 inside its buffer
    block_stride = (k + m) * seg_stride + 8
    batch = rng.integers(0, 256, (nblocks, block_stride), dtype=np.uint8)
    dest = rng.integers(0, 256, batch.shape, dtype=np.uint8) if separate_out else batch
    mem = np.concatenate([np.full(pad, 0xA5, np.uint8), batch.reshape(-1), np.full(64, 0x5A, np.uint8)] +
                         ([dest.reshape(-1), np.full(64, 0x3C, np.uint8)] if separate_out else []))
    before = mem.copy()
    out = pad + batch.size + 64 if separate_out else pad
    view = batch[:, :(k + m) * seg_stride].reshape(nblocks, k + m, seg_stride)
    ref = _reference(view, k, m, vec)
    if accumulate:
        ref[:, k:, :vec] ^= dest[:, :(k + m) * seg_stride].reshape(nblocks, k + m, seg_stride)[:, k:, :vec]
    pairs = nblocks * ((vec + 15) // 16)
    stores = 0
    for wg in range((pairs + 127) // 128):
        stores += _run_workgroup(roles, wg, mem, pad, out, nblocks, vec, seg_stride, block_stride, accumulate, late_dma, order)
    assert stores == nblocks * m * (vec // 8)     # one store per valid item and parity row, none dropped or doubled
    want = before.copy()
    dst = want[out:out + batch.size].reshape(nblocks, block_stride)
    for r in range(m):
        dst[:, (k + r) * seg_stride:(k + r) * seg_stride + vec] = ref[:, k + r, :vec]
    bad = np.nonzero(mem != want)[0]              # parity right; sources, padding and the bytes around unchanged
    assert bad.size == 0, (bad.size, bad[:8])
