"""The fused RS8 repair's block map and column stream (rs8_fdec3.hip), byte for byte and status for
status against the oracle, over what the stream options of tools/codegen/gen_fdec_asm.py touch:

  * grids of 1, 2, 8, 9, 25 and 65 workgroups (nblocks 1, 5, 29, 33, 97, 259): below the 8 XCDs and
    every remainder path of bs::wg_index, every block with content of its own, so that a block
    repaired from another block's columns or coefficients shows;
  * seg_stride = vec (adjacent columns contiguous, what a paired refill relies on) and vec + 8 (not
    contiguous; the pad bytes hold junk that must neither be read into a repair nor written);
  * erased columns at 2i, at 2i + 1 and at both (a refill pair with one or two 0-record halves), the
    first and the last column, 0 / 1 / 7 / 8 / 9 / 15 / 16 erasures, up to three lost parity rows
    below row 16;
  * next to them in the same batch a block with 17 erasures, one whose substitute parity is row 16
    (both leave the fused kernel for the unfused ones behind the gate) and an undecodable one;
  * overwrite and accumulate, and all of it as a sequence of calls on one codec, mixed and all-fused
    batches in turn, so that a gate generation left over from an earlier call shows.

The reference is computed once per (m, vec) on the largest batch; a smaller batch is its first blocks
(a block's erasures depend on its index only).  With the diagnostic library loaded the XCD-contiguous
block map (its variant 20) runs the same cases in a process of its own."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from norm_amd import NFEC_RS8, NormDecoderRS8  # noqa: E402
from norm_amd import _native as N  # noqa: E402

K = 64
NBS = [1, 5, 29, 33, 97, 259]
VECS = [8, 1400, 1408, 1664]
PAD = 8
COUNTS = [0, 1, 7, 8, 9, 15, 16]
_REF = {}


def erasures_of(b, m):
    """block b's erased slots (sorted; source column c at slot c, parity row r at slot K + r)"""
    rng = np.random.default_rng(1000 * m + b)

    def sources(e, must=()):
        must = list(dict.fromkeys(must))[:e]
        rest = [c for c in range(K) if c not in must]
        return sorted(must + [int(c) for c in rng.choice(rest, e - len(must), replace=False)])

    if b == 0:
        return sources(16, [0, K - 1])
    if b == 1:
        return sources(17)                                   # m = 32: unfused; m = 16: undecodable
    if b == 2:                                               # m = 32: substitute parity rows 15 and 16
        return sources(2) + [K + r for r in range(min(15, m - 2))]
    if b == 3:
        return sources(m + 1)                                # undecodable: status 0, left as it came
    if b == 4:
        return []
    j = b - 5
    e = COUNTS[j % 7]
    i = int(rng.integers(0, K // 2))
    must = [[2 * i], [2 * i + 1], [2 * i, 2 * i + 1]][j % 3]
    must += [[0], [K - 1], [], [0, K - 1], []][j % 5]
    lost = min((j // 7) % 4, m - e)
    rows = sorted(int(r) for r in rng.choice(16, lost, replace=False))
    return sources(e, must) + [K + r for r in rows]


def reference(orc, m, vec):
    """(clean, locs, counts, repaired, status) of the largest batch at seg_stride vec + PAD"""
    if (m, vec) in _REF:
        return _REF[(m, vec)]
    nb = max(NBS)
    rng = np.random.default_rng(7 * m + vec)
    clean = orc.encode_blocks(NFEC_RS8, K, m, vec, orc.make_blocks(K, m, vec, nb, seg_stride=vec + PAD))
    clean[:, :, vec:] = rng.integers(0, 256, (nb, K + m, PAD), dtype=np.uint8)
    locs = np.zeros((nb, m + 1), np.uint16)
    counts = np.zeros(nb, np.uint16)
    for b in range(nb):
        e = erasures_of(b, m)
        assert e == sorted(set(e)) and len(e) <= m + 1
        locs[b, :len(e)] = e
        counts[b] = len(e)
    rx = clean.copy()
    for b in range(nb):
        rx[b, locs[b, :counts[b]], :vec] = 0
    ok = counts <= m          # a longer list is undecodable: the reference's matrix build fails, status 0
    part = rx[ok].copy()
    status = np.zeros(nb, np.int32)
    status[ok] = orc.decode_blocks(NFEC_RS8, K, m, vec, part, locs[ok, :m], counts[ok])
    repaired = rx.copy()
    repaired[ok] = part
    assert np.array_equal(repaired[:, :, vec:], clean[:, :, vec:])
    # the fixture holds what it is meant to: fused blocks, the three kinds that are not, all counts
    assert status[3] == 0 and set(COUNTS) - {0} <= set(int(c) for c in counts[status != 0])
    for a in (clean, locs, counts, repaired, status):
        a.setflags(write=False)
    _REF[(m, vec)] = (clean, locs, counts, repaired, status)
    return _REF[(m, vec)]


def _i16(a):
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.uint16).view(np.int16)).cuda()


def run_case(orc, m, vec, pad, nbs=NBS):
    clean, locs, counts, repaired, status = reference(orc, m, vec)
    w = vec + pad
    dec = NormDecoderRS8()
    assert dec.Init(K, m, vec)
    rng = np.random.default_rng(vec + pad + m)
    for nb in list(nbs) + [nbs[0], nbs[-1]]:
        for accumulate in (False, True):
            rx = np.array(clean[:nb, :, :w])
            want = np.array(repaired[:nb, :, :w])
            for b in range(nb):
                sl = locs[b, :counts[b]].astype(int)
                src = sl[sl < K]
                rx[b, sl, :vec] = 0
                if accumulate:   # the repair XORs into what the erased source segments hold
                    junk = rng.integers(0, 256, (len(src), vec), dtype=np.uint8)
                    rx[b, src, :vec] = junk
                    want[b, src, :vec] = junk ^ clean[b, src, :vec] if status[b] else junk
            dev = torch.from_numpy(rx).cuda()
            assert dev.stride(1) == w
            st = dec.decode_blocks(dev, _i16(locs[:nb]), _i16(counts[:nb]), accumulate=accumulate)
            torch.cuda.synchronize()
            what = f"m={m} vec={vec} seg_stride={w} nblocks={nb} accumulate={accumulate}"
            assert np.array_equal(st.cpu().numpy(), status[:nb]), what
            bad = np.argwhere(dev.cpu().numpy() != want)
            assert bad.size == 0, f"{what}: {len(bad)} bytes differ, first (block, slot, byte) = {bad[0]}"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from norm_amd import device_count

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    assert device_count() >= 1, "no gfx950 device visible to libnfec"


@pytest.mark.parametrize("pad", [0, PAD])
@pytest.mark.parametrize("vec", VECS)
@pytest.mark.parametrize("m", [32, 16])
def test_fdec3_stream(orc, m, vec, pad):
    run_case(orc, m, vec, pad)


def test_fdec3_stream_xcd_block_map_of_the_diagnostic_library(orc):
    """variant 20 of the diagnostic library (each XCD a contiguous range of blocks) on the same
    cases; the product library has one block map, which test_fdec3_stream covers"""
    if "diag" not in os.path.basename(N.LIB_PATH):
        return
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, NFEC_FDEC3="0", NFEC_FDEC_VARIANT="20", PYTHONPATH=root)
    subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, cwd=root, check=True, timeout=300)


if __name__ == "__main__":
    from oracle import pyoracle

    for case_vec in (1400, 1664):
        for case_pad in (0, PAD):
            run_case(pyoracle, 32, case_vec, case_pad)
    print("xcd block map: ok")
