"""Every dispatch route on batches that are embedded in a larger allocation, and every ladder walked
by layout, byte for byte against the oracle (tests/batch_layouts.py has the layouts and bounds).

Part one runs each route's batch at three placements (batch_layouts.placements): base 8 mod 16 with
blocks 8 bytes apart, base 8 mod 256 with padded slots, spare slots and a gap, and every other block
of a pool.  Part two runs each case of batch_layouts.LADDERS at the last block_stride a rung's 2^31
predicate accepts and at the first it refuses; tests/test_batch_layouts.py checks on the host that
those strides are what they claim.  The knobs that used to force the later rungs are compiled out of
the product library, so a layout is the only way to reach them there.

Every run asserts the path counter of the rung that must take the batch (and the tail counter),
compares statuses and every writable byte with the oracle, and compares everything else near the
batch -- slot padding, spare slots, the gap behind each block, 4 KiB in front of and behind each
block, all seeded junk -- with what was put there.  All runs share one pool of at most 3 GiB, of
which only the placed blocks and their bands are ever touched.
"""
import functools
from collections import namedtuple

import numpy as np
import pytest

import batch_layouts as L

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from norm_amd import (NFEC_FEATURE_RS16_TOEPLITZ, NFEC_MDP, NFEC_RS8, NFEC_RS16, NormDecoderMDP,  # noqa: E402
                      NormDecoderRS8, NormDecoderRS16, NormEncoderMDP, NormEncoderRS8, NormEncoderRS16)
from norm_amd import _native as N  # noqa: E402

KIND = {"RS8": NFEC_RS8, "RS16": NFEC_RS16, "MDP": NFEC_MDP}
ENC = {"RS8": NormEncoderRS8, "RS16": NormEncoderRS16, "MDP": NormEncoderMDP}
DEC = {"RS8": NormDecoderRS8, "RS16": NormDecoderRS16, "MDP": NormDecoderMDP}
OFF, ON, SHARED = N.NFEC_OPT_RS16_TOEPLITZ_OFF, N.NFEC_OPT_RS16_TOEPLITZ_ON, N.NFEC_OPT_RS16_SHARED_TABLES
OPTS = {"": 0, "toeplitz_off": OFF, "toeplitz_on": ON, "shared": SHARED | OFF}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from norm_amd import device_count

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    assert device_count() >= 1, "no gfx950 device visible to libnfec"


@pytest.fixture(scope="module")
def pool():
    """The one allocation of this module, in a one-element list: never initialised as a whole,
    dropped at module end and handed back to the device.  The list, not the tensor, is what pytest
    keeps among a test's arguments (it holds those past the module's teardown), so clearing it
    drops the last reference."""
    base = torch.cuda.memory_allocated()
    holder = [torch.empty(L.pool_bytes(), dtype=torch.uint8, device="cuda")]
    assert holder[0].data_ptr() % 4096 == 0
    yield holder
    holder.clear()
    torch.cuda.empty_cache()
    assert torch.cuda.memory_allocated() < base + L.pool_bytes(), "the pool outlived its module"


def _i16(a):
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.uint16).view(np.int16)).cuda()


# ---- one batch: data and the oracle's answer, built once per case and only read ----
# pattern: per block (cycled) (source erasures, parity rows lost: a list, or a count of random rows)
Case = namedtuple("Case", "id call kind k m vec nb path nd opts pattern acc")
Case.__new__.__defaults__ = (None, 0, (), False)


def _tail(c, path):
    """the tail kernels run beside the fixed and runtime rungs of RS8 / MDP when vec % 8 != 0"""
    return int(c.vec % 8 != 0 and c.kind != "RS16" and path in ("fixed", "runtime"))


@functools.lru_cache(maxsize=None)
def _data(cid, acc):
    from oracle import pyoracle as orc

    c = CASES[cid]
    k, m, vec, nb, kind = c.k, c.m, c.vec, c.nb, KIND[c.kind]
    rng = np.random.default_rng([len(cid), vec, k, m, int(acc)] + [ord(ch) for ch in cid])
    nd = np.full(nb, k, np.uint16) if c.nd is None else np.asarray(c.nd, np.uint16)
    ndarg = None if c.nd is None else nd
    src = orc.make_blocks(k, m, vec, nb, num_data=ndarg, first_block=getattr(c, "b0", 0))
    clean = orc.encode_blocks(kind, k, m, vec, src.copy(), ndarg)
    if c.call == "enc":
        return dict(nd=nd, ndarg=ndarg, src=src, ref=clean)
    locs = np.zeros((nb, m), np.uint16)
    counts = np.zeros(nb, np.uint16)
    for b in range(nb):
        n = int(nd[b])
        es, par = c.pattern[b % len(c.pattern)]
        if es == "orc":     # tests/test_gpu_parity.py's _erasures(orc, ..., 90, 20, num_data, seed_off=77)
            bi = b + c.pattern[0][1]
            s_ = orc.erasure_pattern(bi + 77, n, min(90, n))
            p_ = (n + orc.erasure_pattern(bi + 9000 + 77, m, 20)).astype(np.uint16)
            e = np.concatenate([s_, p_])[:m]
        else:
            es = min(es, n)
            rows = np.sort(rng.choice(m, par, replace=False)) if isinstance(par, int) else np.asarray(par, int)
            assert es + len(rows) <= m
            e = np.concatenate([np.sort(rng.choice(n, es, replace=False)), n + rows])
        counts[b] = len(e)
        locs[b, :len(e)] = e
    rx = clean.copy()
    for b in range(nb):
        for s in locs[b, :counts[b]]:
            # reference contract: erased buffers zero-filled; accumulate: the repair XORs into junk
            rx[b, s, :vec] = rng.integers(0, 256, vec, dtype=np.uint8) if acc and s < nd[b] else 0
    ref = rx.copy()
    st = orc.decode_blocks(kind, k, m, vec, ref, locs, counts, ndarg)
    assert (st == counts).all(), "every block of these cases is decodable"
    return dict(nd=nd, ndarg=ndarg, rx=rx, ref=ref, st=st, locs=locs, counts=counts)


def _run(pool, c, lay, path, acc=False, seed=1):
    pool = pool[0]
    d = _data(c.id, acc)
    k, m, vec, nb, nd = c.k, c.m, c.vec, c.nb, d["nd"]
    lay.check(k, m, vec)
    rs16 = c.kind == "RS16"
    codec = (ENC if c.call == "enc" else DEC)[c.kind](options=c.opts)
    assert codec.Init(k, m, vec)
    if c.opts & ON:
        assert codec.features() & NFEC_FEATURE_RS16_TOEPLITZ
    view = L.embed(pool, lay.lead, nb, lay.slots, lay.seg_stride, lay.block_stride)
    assert view.data_ptr() == pool.data_ptr() + lay.lead and view.stride() == (lay.block_stride, lay.seg_stride, 1)
    ndt = None if d["ndarg"] is None else _i16(nd)
    t0 = codec.tail_batches()
    if c.call == "enc":
        before = L.put(pool, lay, vec, d["src"], nd, seed)      # junk in the parity slots and past them
        masks = [L.writable("enc", rs16, vec, int(nd[b]), m, lay.slots) for b in range(nb)]
        p0 = codec.encode_paths()
        codec.encode_blocks(view, num_data=ndt, accumulate=acc)
        torch.cuda.synchronize()
        p1 = codec.encode_paths()
        want = d["ref"].copy()
        if acc:
            for b in range(nb):
                n = int(nd[b])
                for s in range(n, n + m):
                    want[b, s, :vec] ^= before.slot(b, s)[:vec]
    else:
        before = L.put(pool, lay, vec, d["rx"], nd + m, seed)
        masks = [L.writable("dec", rs16, vec, int(nd[b]), m, lay.slots, d["locs"][b, :d["counts"][b]], d["st"][b] > 0)
                 for b in range(nb)]
        p0 = codec.decode_paths()
        st = codec.decode_blocks(view, _i16(d["locs"]), _i16(d["counts"]), num_data=ndt, accumulate=acc)
        torch.cuda.synchronize()
        p1 = codec.decode_paths()
        assert np.array_equal(st.cpu().numpy(), d["st"])
        want = d["ref"]
    after = before.download(pool)
    assert {n: p1[n] - p0[n] for n in p1 if p1[n] != p0[n]} == {path: 1}, (p0, p1)
    t1 = codec.tail_batches()
    key = "encode" if c.call == "enc" else "decode"
    assert t1[key] - t0[key] == _tail(c, path), (t0, t1)
    for b in range(nb):
        for s in range(int(nd[b]) + m):
            row = masks[b][s]
            if row.any():
                bad = np.nonzero(after.slot(b, s)[:vec][row] != want[b, s, :vec][row])[0]
                assert bad.size == 0, ("differs from the oracle", c.id, lay, b, s, bad.size, bad[:8])
    L.check_untouched(before, after, masks)
    codec.Destroy()


# ---- part one: every route on embedded batches ----
ND7 = (64, 63, 1, 17, 64, 32, 48)
FUSED32 = ((1, []), (8, [3]), (9, []), (16, []), (17, []), (32, []), (16, [0, 15]))   # e = 17, 32: unfused
PART_ONE = [
    # encode
    Case("enc-rs8-64-32-v24-t3", "enc", "RS8", 64, 32, 24, 7, "fixed"),
    Case("enc-rs8-64-32-v1400-t3", "enc", "RS8", 64, 32, 1400, 5, "fixed"),
    Case("enc-rs8-64-32-v1397-tail", "enc", "RS8", 64, 32, 1397, 5, "fixed"),
    Case("enc-rs8-64-32-short-q4", "enc", "RS8", 64, 32, 1400, 7, "fixed", ND7),
    Case("enc-rs8-64-16-v1408", "enc", "RS8", 64, 16, 1408, 5, "fixed"),
    Case("enc-rs8-64-8-v200", "enc", "RS8", 64, 8, 200, 7, "fixed"),
    Case("enc-rs8-20-10-v1000", "enc", "RS8", 20, 10, 1000, 5, "runtime"),
    Case("enc-rs8-20-10-v1003", "enc", "RS8", 20, 10, 1003, 5, "runtime"),
    Case("enc-rs8-20-10-v1000-short", "enc", "RS8", 20, 10, 1000, 5, "runtime", (20, 1, 19, 7, 10)),
    Case("enc-rs8-20-10-v1003-short", "enc", "RS8", 20, 10, 1003, 5, "runtime", (20, 1, 19, 7, 10)),
    Case("enc-rs8-200-55-v136", "enc", "RS8", 200, 55, 136, 5, "runtime"),
    Case("enc-mdp-64-32-v1400", "enc", "MDP", 64, 32, 1400, 5, "fixed"),
    Case("enc-mdp-30-20-v203", "enc", "MDP", 30, 20, 203, 5, "runtime"),
    Case("enc-mdp-30-20-v203-short", "enc", "MDP", 30, 20, 203, 5, "runtime", (30, 1, 29, 7, 15)),
    Case("enc-rs16-40-10-v66-tower", "enc", "RS16", 40, 10, 66, 5, "rs16_product", None, OFF),
    Case("enc-rs16-100-20-v1400-tower", "enc", "RS16", 100, 20, 1400, 5, "rs16_product", None, OFF),
    Case("enc-rs16-128-32-v1408-split", "enc", "RS16", 128, 32, 1408, 5, "rs16_split", None, ON),
    Case("enc-rs16-400-100-v64-split2", "enc", "RS16", 400, 100, 64, 5, "rs16_split", None, ON),
    Case("enc-rs16-40-10-v66-tower-short", "enc", "RS16", 40, 10, 66, 5, "rs16_product", (40, 1, 39, 7, 20), OFF),
    Case("enc-rs16-32-8-v64-shared", "enc", "RS16", 32, 8, 64, 5, "rs16_product", None, SHARED | OFF),
    Case("enc-rs16-32-8-v64-shared-short", "enc", "RS16", 32, 8, 64, 5, "generic", (32, 1, 31, 7, 16), SHARED | OFF),
    # decode
    Case("dec-rs8-64-32-v1400-fdec3", "dec", "RS8", 64, 32, 1400, 7, "fixed", None, 0, FUSED32),
    Case("dec-rs8-64-16-v1400-fdec3", "dec", "RS8", 64, 16, 1400, 5, "fixed", None, 0,
         ((1, []), (8, [2]), (9, []), (16, []), (5, [0]))),
    Case("dec-rs8-64-8-v1400-fdec", "dec", "RS8", 64, 8, 1400, 5, "fixed", None, 0,
         ((1, []), (8, []), (5, [1]), (3, []), (7, []))),
    Case("dec-rs8-64-32-v1672-fdec", "dec", "RS8", 64, 32, 1672, 5, "fixed", None, 0,
         ((1, []), (8, [3]), (16, []), (17, []), (9, []))),
    Case("dec-rs8-64-32-short", "dec", "RS8", 64, 32, 1400, 7, "fixed", ND7, 0, FUSED32),
    Case("dec-rs8-64-32-v1397-tail", "dec", "RS8", 64, 32, 1397, 5, "fixed", None, 0,
         ((16, []), (8, [3]), (17, []), (1, []), (32, []))),
    Case("dec-rs8-20-10-v1000-rt", "dec", "RS8", 20, 10, 1000, 5, "runtime", None, 0,
         ((10, []), (3, [1]), (1, []), (7, [0, 2, 5]), (5, []))),
    Case("dec-rs8-20-10-v1003-rt", "dec", "RS8", 20, 10, 1003, 5, "runtime", None, 0,
         ((10, []), (3, [1]), (1, []), (7, [0, 2, 5]), (5, []))),
    Case("dec-rs8-128-127-v72-rt", "dec", "RS8", 128, 127, 72, 5, "runtime", None, 0,
         ((100, []), (100, [5]), (127, []), (1, []), (100, 20))),
    Case("dec-mdp-64-32-v1400-rt", "dec", "MDP", 64, 32, 1400, 5, "runtime", None, 0,
         ((16, []), (20, [1, 2]), (1, []), (32, []), (12, [0]))),
    Case("dec-mdp-64-32-v1397-rt", "dec", "MDP", 64, 32, 1397, 5, "runtime", None, 0,
         ((16, []), (20, [1, 2]), (1, []), (32, []), (12, [0]))),
    Case("dec-mdp-30-20-v203-short-rt", "dec", "MDP", 30, 20, 203, 5, "runtime", (30, 1, 29, 7, 15), 0,
         ((12, 3), (1, []), (20, []), (5, 10), (8, [0]))),
    Case("dec-rs16-40-10-v66-tower", "dec", "RS16", 40, 10, 66, 5, "rs16_tower", None, 0,
         ((7, 3), (10, []), (1, []), (4, [0]), (6, 2))),
    Case("dec-rs16-400-100-v64-tower", "dec", "RS16", 400, 100, 64, 5, "rs16_tower", None, 0,
         ((40, 10), (25, 25), (2, []), (50, []), (30, 20))),
    Case("dec-rs16-32-8-v64-shared", "dec", "RS16", 32, 8, 64, 5, "generic", None, SHARED,
         ((8, []), (3, [1]), (1, []), (5, 2), (6, []))),
    Case("dec-rs16-160-80-v64-shared-big-plan", "dec", "RS16", 160, 80, 64, 5, "generic", None, SHARED,
         ((80, []), (70, 10), (65, [0]), (1, []), (80, []))),
    Case("dec-rs16-300-400-v64-scratch-plan", "dec", "RS16", 300, 400, 64, 5, "generic", None, 0,
         ((280, []), (280, 10), (257, [0]), (1, []), (300, []))),
]


# ---- part two: batch_layouts.LADDERS as cases of the same runner ----
class _LadderCase(namedtuple("_LadderCase", Case._fields + ("b0",))):
    pass


def _ladder_case(c):
    nd = L.ladder_num_data(c)
    if (c.k, c.m) == (128, 127):
        pattern = (("orc", c.b0),)
    elif c.es == -1:    # a block the snippet solve could take (<= 16 erased source) and one past it
        pattern = ((12, 2), (20, 1))
    else:
        pattern = ((c.es, c.ep),)
    return _LadderCase(c.id, c.call, c.kind, c.k, c.m, c.vec, c.nb, None, None if nd is None else tuple(int(x) for x in nd),
                       OPTS[c.opts], pattern, c.acc, c.b0)


CASES = {c.id: c for c in PART_ONE}
CASES.update({c.id: _ladder_case(c) for c in L.LADDERS})
assert len(CASES) == len(PART_ONE) + len(L.LADDERS)


def _placed(c, name):
    p = L.placements(c.k, c.m, c.vec)[name]
    return L.Layout(p["lead"], c.nb, p["slots"], p["seg_stride"], p["block_stride"])


@pytest.mark.parametrize("place", ["A", "B", "C"])
@pytest.mark.parametrize("c", PART_ONE, ids=[c.id for c in PART_ONE])
def test_route_on_an_embedded_batch(pool, c, place):
    _run(pool, c, _placed(c, place), c.path, seed=ord(place))


@pytest.mark.parametrize("c", [c for c in PART_ONE if c.kind != "MDP"], ids=[c.id for c in PART_ONE if c.kind != "MDP"])
def test_route_accumulates_on_an_embedded_batch(pool, c):
    """NFEC_ACCUMULATE at placement B (MDP refuses it).  The split does not accumulate: such a
    batch takes the product kernel (encode_rs16)."""
    path = "rs16_product" if c.path == "rs16_split" else c.path
    _run(pool, c, _placed(c, "B"), path, acc=True, seed=7)


LADDER_RUNS = [pytest.param(c, side, lay, expect, id=f"{c.id}-{side}")
               for c in L.LADDERS for side, lay, expect in L.ladder_layouts(c)]


@pytest.mark.parametrize("c,side,lay,expect", LADDER_RUNS)
def test_ladder_by_layout(pool, c, side, lay, expect):
    """The rung that must take the batch, by its counter; expect[1] names the kernel family where
    the counter cannot (rs8_t3 and rs8_q4 both count as "fixed"): that is pinned by the restated
    predicates in tests/test_batch_layouts.py, not here."""
    assert lay.extent <= pool[0].numel()
    _run(pool, CASES[c.id], lay, expect[0], acc=c.acc, seed=3 + (side == "first-refused"))
