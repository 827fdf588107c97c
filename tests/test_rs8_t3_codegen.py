"""Static properties of the 3-role-wave Karatsuba RS8(64,32) encode kernel (rs8_t3_enc_k64_m32) as
tools/codegen/gen_rs8_t3.py emits it, the algebra it rests on, and its three instruction streams
run on test_rs8_d2_codegen.py's interpreter.

The kernel must fit 168 VGPRs without scratch and a quarter of a CU's LDS (4 workgroups of 3
waves: 3 waves per SIMD).  The interpreter runs the generated text of roles A, B and C barrier to
barrier against a batch in host memory, with late and with early landing of the asynchronous
operations and with the roles taking their turns in several orders, so a wrong wait count, LDS
offset, coefficient or a hand-over read too early shows without a GPU."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = os.path.join(ROOT, "tools", "codegen", "gen_rs8_t3.py")
sys.path.insert(0, os.path.join(ROOT, "tools", "codegen"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_rs8_d2 as d2  # noqa: E402
import gen_rs8_t3 as t3  # noqa: E402
from gen_rs8_bitsliced import generator, mul  # noqa: E402
from test_fdec3_codegen import _expand, _vgprs  # noqa: E402
from test_rs8_d2_codegen import _Wave, _asm_lines, _reference  # noqa: E402

MAX_VGPR = 167                       # 512 registers per SIMD lane / 3 waves, in granules of 8: 168
KERNEL = "rs8_t3_enc_k64_m32"
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def generated(tmp_path_factory):
    d = tmp_path_factory.mktemp("t3")
    out = {}
    for name, flags in (("product", []), ("diag", ["--diag"])):
        path = str(d / f"{name}.hip")
        subprocess.run([sys.executable, GEN, path] + flags, check=True)
        out[name] = open(path).read()
    out["dir"] = str(d)
    return out


@pytest.fixture(scope="module")
def streams():
    G = generator(t3.K, t3.M)
    return [t3.role_asm(G, r) for r in range(t3.NW)]


def _roles(text, name):
    out = []
    for r in range(t3.NW):
        start = text.index(f"void {name}_role{r}(")
        out.append(_asm_lines(text[start:text.index("\n        :\n", start)]))
    return out


def test_committed_file_is_the_generator_output(generated):
    with open(os.path.join(ROOT, "norm_amd", "csrc", "rs8_enc_t3.hip")) as f:
        assert f.read() == generated["product"]
    assert len(generated["product"]) < (1 << 20)


def test_compact_form_is_the_plain_instructions(generated, streams):
    roles = _roles(_expand(generated["product"]), KERNEL)
    for r in range(t3.NW):
        assert len(streams[r]) > 5000 and roles[r] == streams[r], r


def test_product_has_no_probes_or_knobs(generated):
    text = generated["product"]
    assert "probe" not in text and "getenv" not in text and "VARIANT" not in text
    assert KERNEL in text and "launch_rs8_t3_encode" in text
    assert {f"{KERNEL}_probe_{p}" for p in t3.PROBES.values()} <= set(re.findall(r"void (\w+)\(bs::EncArgs", generated["diag"]))
    assert "launch_rs8_t3_probe" in generated["diag"] and "NFEC_T3_VARIANT" in generated["diag"]


@pytest.mark.parametrize("which", ["product", "diag"])
def test_register_and_lds_budget_of_the_source(generated, which):
    text = _expand(generated[which]) if which == "product" else generated[which]
    names = [KERNEL] if which == "product" else [f"{KERNEL}_probe_{p}" for p in t3.PROBES.values()]
    for name in names:
        for r in range(t3.NW):
            start = text.index(f"void {name}_role{r}(")
            src = text[start:text.index("\n}", start)]
            body, clob = src.split("\n        :\n")[0], src.split("\n        : ")[-1]
            used = _vgprs(body)
            assert not used or max(used) <= MAX_VGPR, (name, max(used))
            clobbered = {int(a) for a in re.findall(r'"v(\d+)"', clob)}
            free = set(range(MAX_VGPR + 1)) - clobbered
            assert len(free) == 2 and used <= clobbered, (name, sorted(free), sorted(used - clobbered))
        mt = re.search(r"__launch_bounds__\((\d+), (\d+)\) void " + name + r"\(", text)
        assert (int(mt.group(1)), int(mt.group(2))) == (192, 3), name
    # 4 workgroups per CU (3 waves per SIMD x 4 SIMDs / 3 waves) at both candidate allocation granules
    lds = {int(x) for x in re.findall(r"__shared__[^;]*\[(\d+) / 4\];", text)}
    assert lds == {t3.LDS_BYTES} and t3.LDS_BYTES <= 40960
    for granule in (512, 1280):
        assert 4 * (-(-t3.LDS_BYTES // granule) * granule) <= 160 * 1024, granule
    # every LDS offset lies inside the allocation and M0 targets stay 16-byte aligned, inside the rings
    for off in re.findall(r"offset:(\d+)", text):
        assert int(off) + 64 * 16 <= t3.LDS_BYTES or int(off) + 64 * 8 <= t3.LDS_BYTES, off
    for off in re.findall(r"s_add_u32 m0, %\[lb\], (\d+)", text):
        assert int(off) % 16 == 0 and int(off) + 1024 <= t3.EX0, off


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
    assert field("group_segment_fixed_size") == t3.LDS_BYTES
    assert field("max_flat_workgroup_size") == 192
    assert re.findall(r"; Occupancy: (\d+)", text) == ["3"]
    assert "scratch_" not in text.split(";;#ASMSTART")[0]


# ---- the algebra ----
def test_generator_factors_into_scalings_and_a_toeplitz_core():
    """G[p][j] = W(y_p) tau(k + p - j) c_j for every parity row p and column j >= 1"""
    G = generator(t3.K, t3.M)
    Wy, c, tau = t3.algebra()
    assert all(Wy) and all(c[1:])
    for p in range(t3.M):
        for j in range(1, t3.K):
            assert G[p][j] == mul(mul(Wy[p], tau(t3.K + p - j)), c[j]), (p, j)


def test_three_role_identity_for_every_entry():
    """what the roles apply sums to the generator: every (p, j), column 0 and the missing column 64"""
    G = generator(t3.K, t3.M)
    steps, Wy = t3.plan(G)
    assert len(steps) == t3.STEPS
    seen = set()
    for st in steps:
        j0, j1 = st["j0"], st["j1"]
        seen.add(j0)
        for p in range(16):
            lo, hi = mul(Wy[p], st["s1"][p]), mul(Wy[16 + p], st["s1"][p])
            assert lo == G[p][j0] and hi ^ st["s3"][p] == G[16 + p][j0], (p, j0)
            if j1 is None:
                assert st["s2"][p] == G[p][0] and st["s3x"][p] == G[16 + p][0]
            else:
                assert mul(lo, st["gamma"]) ^ st["s2"][p] == G[p][j1] and mul(hi, st["gamma"]) == G[16 + p][j1], (p, j1)
        seen.add(0 if j1 is None else j1)
    assert seen == set(range(t3.K)) and steps[-1]["j1"] is None


def test_three_role_form_encodes_random_bytes():
    G = generator(t3.K, t3.M)
    steps, Wy = t3.plan(G)
    tab = np.array([[mul(c, x) for x in range(256)] for c in range(256)], np.uint8)
    d = np.random.default_rng(3).integers(0, 256, (t3.K, 257), dtype=np.uint8)
    s1, s2, s3 = (np.zeros((16, 257), np.uint8) for _ in range(3))
    for st in steps:
        u = d[st["j0"]].copy()
        if st["j1"] is not None:
            u ^= tab[st["gamma"]][d[st["j1"]]]
        own_b = d[0 if st["j1"] is None else st["j1"]]
        for p in range(16):
            s1[p] ^= tab[st["s1"][p]][u]
            s2[p] ^= tab[st["s2"][p]][own_b]
            s3[p] ^= tab[st["s3"][p]][d[st["j0"]]]
            if st["j1"] is None:
                s3[p] ^= tab[st["s3x"][p]][d[0]]
    for p in range(16):
        lo = np.zeros(257, np.uint8)
        hi = np.zeros(257, np.uint8)
        for j in range(t3.K):
            lo ^= tab[G[p][j]][d[j]]
            hi ^= tab[G[16 + p][j]][d[j]]
        assert np.array_equal(tab[Wy[p]][s1[p]] ^ s2[p], lo) and np.array_equal(tab[Wy[16 + p]][s1[p]] ^ s3[p], hi), p


def test_fewer_vector_instructions_than_d2(streams):
    """0.86 derived from the block products (three instead of four per pair of column groups, one
    transpose per column as before), plus slack for moves"""
    G = generator(t3.K, t3.M)

    def valu(lines):
        return sum(1 for ln in lines if ln.startswith("v_"))
    new = sum(valu(s) for s in streams)
    old = sum(valu(d2.role_asm(G, w)) for w in range(d2.NW))
    assert new <= 0.88 * old, (new, old)


# ---- the instruction streams on the interpreter ----
def _run_workgroup(roles, wg, mem, base, out, nblocks, vec, seg_stride, block_stride, accumulate, late, order):
    """the kernel's C++ prologue (waves 1 and 2 park their pair offsets), then the three role waves
    barrier to barrier in the given order of turns; -> (items stored, column 0's exchange reads)"""
    lds = np.zeros(t3.LDS_BYTES, np.uint8)
    pps = (vec + 15) // 16
    total = nblocks * pps
    g0 = wg * t3.PAIRS
    b0 = min(g0, total - 1) // pps
    park = lds.view(np.uint32)
    for w in range(2):
        for lane in range(64):
            for p in range(2):
                g = g0 + 64 * p + lane
                gg = g if g < total else g0
                b, o = gg // pps, (gg % pps) * 16
                off = (b - b0) * block_stride + o
                i = t3.PARK0 // 4 + w * (t3.PARK // 4) + 2 * lane + p
                park[i] = off if g < total else 0x80000000
                park[i + 128] = off + 8 if g < total and o + 16 <= vec else 0x80000000
    waves = []
    for r in range(t3.NW):
        env = {"%[ib]": base + b0 * block_stride, "%[ob]": out + b0 * block_stride, "%[ss]": seg_stride,
               "%[acc]": accumulate, "%[lb]": 0, "%[la]": "v0", "%[la2]": "v1"}
        wv = _Wave(roles[r], env, mem, lds, late)
        wv.v[0] = np.arange(64, dtype=np.uint32) * 8
        wv.v[1] = np.arange(64, dtype=np.uint32) * 16
        waves.append(wv)
    runs = [wv.run() for wv in waves]
    live = [True] * t3.NW
    while any(live):
        for r in order:
            if live[r]:
                try:
                    next(runs[r])
                except StopIteration:
                    live[r] = False
        assert len(set(live)) == 1, "the role waves pass different numbers of barriers"
    assert waves[0].stores == 0                    # role A stores nothing
    return sum(wv.stores for wv in waves)


CASES = [
    # vec, seg_stride, nblocks, accumulate, separate_out
    (24, 24, 3, 0, False),        # half-valid pairs at every segment end, a partial item group
    (24, 32, 47, 0, False),       # 94 pairs over 47 blocks in one item group, padded segments
    (200, 200, 1, 1, False),      # accumulate onto nonzero parity, half-valid last pair
    (1040, 1048, 1, 0, False),    # an item group's second pair row, vec % 16 = 0
    (40, 48, 5, 1, True),         # parity (accumulated) into another buffer than the sources'
    (16, 16, 1, 0, False),        # one pair: column 0 and the step without a column 64 decide every byte
]
ORDERS = [(0, 1, 2), (1, 2, 0), (2, 0, 1)]   # role A first, role A last, role A between


def test_last_step_carries_column_zero(streams):
    """the step whose j1 would be 64: role B loads column 0, role C reads its planes from role
    B's half of the exchange, role A reads role C's planes only"""
    a, b, c = streams
    last = (t3.STEPS - 1) % 2
    assert sum(1 for ln in b if ln == f"s_mul_i32 s{d2.S_COL}, %[ss], 0") == 1
    assert not any(ln == f"s_mul_i32 s{d2.S_COL}, %[ss], 0" for ln in c)
    c0 = [i for i, ln in enumerate(c) if ln.startswith("ds_read_b64") and ln.endswith(f"%[la] offset:{t3.ex(last, 0)}")]
    barriers = [i for i, ln in enumerate(c) if ln == "s_barrier"]
    assert len(c0) == 1 and barriers[t3.STEPS - 1] < c0[0] < barriers[t3.STEPS]
    reads_b = [i for i, ln in enumerate(a) if ln.startswith("ds_read_b64") and ln.endswith(f"%[la] offset:{t3.ex(last, 0)}")]
    reads_c = [i for i, ln in enumerate(a) if ln.startswith("ds_read_b64") and ln.endswith(f"%[la] offset:{t3.ex(last, 1)}")]
    assert len(reads_b) == t3.STEPS // 2 - 1 and len(reads_c) == t3.STEPS // 2


@pytest.mark.parametrize("late", [True, False])
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("vec,seg_stride,nblocks,accumulate,separate_out", CASES)
def test_instruction_streams_encode(streams, vec, seg_stride, nblocks, accumulate, separate_out, order, late):
    k, m = t3.K, t3.M
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
    for wg in range((pairs + t3.PAIRS - 1) // t3.PAIRS):
        stores += _run_workgroup(streams, wg, mem, pad, out, nblocks, vec, seg_stride, block_stride, accumulate, late, order)
    assert stores == nblocks * m * (vec // 8)     # one store per valid item and parity row, none dropped or doubled
    want = before.copy()
    dst = want[out:out + batch.size].reshape(nblocks, block_stride)
    for r in range(m):
        dst[:, (k + r) * seg_stride:(k + r) * seg_stride + vec] = ref[:, k + r, :vec]
    bad = np.nonzero(mem != want)[0]              # parity right; sources, padding and the bytes around unchanged
    assert bad.size == 0, (bad.size, bad[:8])


def test_interpreter_rejects_unequal_barrier_counts(streams):
    """the harness's own check: a role with one barrier less is caught"""
    a = list(streams[0])
    a.remove("s_barrier")
    with pytest.raises(AssertionError):
        mem = np.zeros(40 + 96 * 16 + 8 + 64, np.uint8)
        _run_workgroup([a, streams[1], streams[2]], 0, mem, 40, 40, 1, 16, 16, 96 * 16 + 8, 0, True, (0, 1, 2))
