"""Static properties of the 3-waves-per-SIMD fused repair kernels (rs8_fdec3_*) as
tools/codegen/gen_fdec_asm.py emits them: they must fit 168 VGPRs and a third of a CU's LDS, or
the occupancy they exist for is lost without any test failing."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = os.path.join(ROOT, "tools", "codegen", "gen_fdec_asm.py")

MAX_VGPR = 167                       # 512 registers per SIMD lane / 3 waves, in granules of 8: 168
# 160 KiB of LDS per CU, three workgroups, rounded down to a multiple of both candidate allocation
# granules (512 B and 1,280 B)
LDS_BUDGET = (160 * 1024 // 3) // 2560 * 2560


@pytest.fixture(scope="module")
def generated(tmp_path_factory):
    """product: the committed rs8_fdec3.hip's generator run (compact form, expanded here);
    diag: gen_fdec_asm.hip of the diagnostic library, which carries the kernel's probes"""
    d = tmp_path_factory.mktemp("fdec3")
    out = {}
    for name, flags in (("product", ["--fdec3"]), ("diag", ["--diag"])):
        path = str(d / f"{name}.hip")
        subprocess.run([sys.executable, GEN] + flags + [path], check=True)
        out[name] = open(path).read()
    out["product_raw"] = out["product"]
    out["product"] = _expand(out["product"])
    return out


def _expand(text):
    """replace the calls of the file's instruction macros by the text they stand for"""
    text = text.replace("\\\n", " ")
    macros = {}
    for name, params, body in re.findall(r"^#define (\w+)(?:\(([^)]*)\))? (.*)$", text, re.M):
        macros[name] = ([p.strip() for p in params.split(",")] if params else [], body)
    code = "\n".join(ln for ln in text.split("\n") if not ln.startswith(("#define", "#undef")))
    leaf = {n for n, (_, body) in macros.items() if body.lstrip().startswith('"')}

    def call(mt):
        params, body = macros[mt.group(1)]
        args = [a.strip() for a in mt.group(2).split(",")] if mt.group(2) else []
        assert len(args) == len(params), mt.group(0)
        val = dict(zip(params, args))
        if mt.group(1) not in leaf:  # a run of other macros' calls: substitute the parameters
            return re.sub(r"\b[a-p]\b", lambda x: val.get(x.group(0), x.group(0)), body)
        pieces = re.findall(r'"((?:[^"\\]|\\.)*)"|#(\w+)', body)
        return '"' + "".join(lit if not par else val[par] for lit, par in pieces) + '"'

    def rx(names, fn):
        alt = "|".join(sorted(names, key=len, reverse=True))
        if fn:
            return rf"(?<![\w\"\[%])({alt})\(([^()\"]*)\)"
        return rf"(?<![\w\"\[%.])({alt})()(?![\w\"(])"

    groups = [({n for n in macros if n not in leaf and not macros[n][0]}, False),   # K<n>
              ({n for n in macros if n not in leaf and macros[n][0]}, True),        # U<r>
              ({n for n in leaf if macros[n][0]}, True), ({n for n in leaf if not macros[n][0]}, False)]
    for names, fn in groups:
        if names:
            code = re.sub(rx(names, fn), call, code)
    return code


def _kernels(text):
    """name -> source of every rs8_fdec3_* kernel"""
    parts = re.split(r"(?=__global__ )", text)
    out = {}
    for p in parts:
        mt = re.match(r"__global__ __launch_bounds__\((\d+), (\d+)\) void (rs8_fdec3_\w+)\(", p)
        if mt:
            out[mt.group(3)] = (p[:p.index("\n}\n") + 3], int(mt.group(1)), int(mt.group(2)))
    return out


def _vgprs(src):
    regs = set()
    for a, b in re.findall(r"\bv\[(\d+):(\d+)\]", src):
        regs.update(range(int(a), int(b) + 1))
    regs.update(int(a) for a in re.findall(r"\bv(\d+)\b", src))
    return regs


@pytest.mark.parametrize("which", ["product", "diag"])
def test_fdec3_fits_three_waves_per_simd(generated, which):
    ks = _kernels(generated[which])
    want = {"rs8_fdec3_k64_m32"}   # (it serves m = 16 too)
    if which == "diag":
        want = {f"rs8_fdec3_k64_m32_probe_{p}" for p in ("nos2", "nos1", "noload")}
    assert set(ks) == want
    for name, (src, threads, waves) in ks.items():
        assert (threads, waves) == (256, 3), name
        body, clob = src.split("\n        : [base]")[0], src.split("\n        : ")[-1]
        used = _vgprs(body)
        assert len(used) > 100 and max(used) <= MAX_VGPR, (name, max(used))
        clobbered = {int(a) for a in re.findall(r'"v(\d+)"', clob)}
        assert max(clobbered) <= MAX_VGPR, name
        # the registers left to the compiler (the clobber-free set) lie below the limit too: every
        # register above it is neither named nor clobbered, and the body names no unclobbered one
        # but the compiler's
        free = set(range(MAX_VGPR + 1)) - clobbered
        assert free and max(free) <= MAX_VGPR and len(free) <= 2, (name, sorted(free))
        assert used <= clobbered, (name, sorted(used - clobbered))
        lds = re.findall(r"__shared__[^;]*\[([^\]]+)\];", src)
        assert len(lds) == 1, name
        nbytes = eval(lds[0], {"__builtins__": {}})
        assert nbytes % 4 == 0 and nbytes <= LDS_BUDGET, (name, nbytes)
        assert (nbytes // 4) % 16 == 0, name   # per-wave parts stay 16-byte aligned (DMA pieces)
        assert "s_barrier" not in src, name


def test_fdec3_product_has_no_probes_or_switches(generated):
    text = generated["product_raw"]
    assert "_probe_" not in text and "getenv" not in text and "VARIANT" not in text
    assert "rs8_fdec3_k64_m32" in text and "launch_rs8_fdec3" in text


def test_fdec3_committed_file_is_the_generator_output(generated):
    with open(os.path.join(ROOT, "norm_amd", "csrc", "rs8_fdec3.hip")) as f:
        assert f.read() == generated["product_raw"]
    assert len(generated["product_raw"]) < (1 << 20)


def test_fdec3_compact_form_is_the_plain_instructions(generated):
    """the macro calls of the committed form expand to the instruction text that the generator
    writes as plain strings for the diagnostic library's no-solve probe, up to the solve's rows"""
    def lines(src):
        return re.findall(r'"((?:[^"\\]|\\.)*?)\\n"', src)

    prod = lines(_kernels(generated["product"])["rs8_fdec3_k64_m32"][0])
    probe = lines(_kernels(generated["diag"])["rs8_fdec3_k64_m32_probe_nos2"][0])
    assert len(prod) > 20000
    stage1 = probe.index("s_cmp_le_u32 %[tmax], 8")
    assert stage1 > 10000 and prod[:stage1] == probe[:stage1]
    # the snippet table (the last 256 * 9 + 1 lines before the end label) is the same too
    assert prod[-2400:] == probe[-2400:]
