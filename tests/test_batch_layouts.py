"""The layout helper (tests/batch_layouts.py) on the host: the restated 2^31 predicates, the two
strides every case of tests/test_gpu_layouts.py's second part runs at, and the byte bookkeeping of
the embedded batches.  No GPU: what is checked here is that each case really sits on both sides of
the bound it names, that the rungs after it answer what the case expects, and that its extent fits
the one pool."""
import numpy as np
import pytest

import batch_layouts as L
from batch_layouts import F


@pytest.mark.parametrize("c", L.LADDERS, ids=[c.id for c in L.LADDERS])
def test_ladder_case_sits_on_both_sides_of_its_bound(c):
    ss, n = L._ss(c), c.k + c.m
    ok, bad = L.flip(lambda bs: c.bound(c, bs), n * ss)
    assert bad == ok + 8 and c.bound(c, ok) and not c.bound(c, bad)
    assert c.bound(c, ok - 8) and not c.bound(c, bad + 8)       # one flip, not a window
    lays = L.ladder_layouts(c)
    assert len(lays) == sum(e is not None for e in c.expect) >= 1
    for side, lay, expect in lays:
        lay.check(c.k, c.m, c.vec)                               # check_batch's rules, the pool cap
        assert lay.block_stride == (ok if side == "last-accepted" else bad)
        # the whole restated dispatcher, every later rung included, names the expected rung
        assert L.ladder_rung(c, lay.block_stride) == expect, (side, lay)
        assert lay.extent <= L.pool_bytes() <= L.POOL_CAP


def test_every_layout_selected_rung_is_walked():
    """each row the counters can show only by layout has a case that expects it"""
    seen = {(c.call, c.kind, e) for c in L.LADDERS for e in c.expect if e is not None}
    for want in [("dec", "RS8", ("fixed", "RS8_FIXED")), ("dec", "RS8", ("runtime", "RS8_RT")),
                 ("dec", "RS8", ("generic", "RS_GENERIC")), ("dec", "MDP", ("runtime", "MDP_RT")),
                 ("dec", "MDP", ("generic", "MDP_SOLVE")), ("dec", "RS16", ("rs16_tower", "RS16_TOWER")),
                 ("dec", "RS16", ("generic", "RS_GENERIC")), ("enc", "RS8", ("fixed", "rs8_t3")),
                 ("enc", "RS8", ("fixed", "rs8_q4")), ("enc", "RS8", ("runtime", "rs8_rt")),
                 ("enc", "RS8", ("generic", "gf8_matmul")), ("enc", "MDP", ("runtime", "rs8_rt")),
                 ("enc", "MDP", ("generic", "gf8_matmul")), ("enc", "RS16", ("rs16_split", "tmvp_tw")),
                 ("enc", "RS16", ("rs16_product", "gf16_tw")), ("enc", "RS16", ("generic", "gf16_bs_encode")),
                 ("enc", "RS16", ("generic", "gf16_matmul")), ("enc", "RS16", ("rs16_product", "gf16_t3")),
                 ("dec", "RS16", ("generic", "RS_GENERIC/product"))]:
        assert want in seen, want


def test_bounds_by_hand():
    """the restatements at numbers worked out from the source lines they cite"""
    # 3 bs + 256 ss < 2^31, ss = 1400
    ok, bad = L.flip(lambda bs: L.offsets_fit(bs, 1400), 96 * 1400)
    assert ok == (F - 1 - 256 * 1400) // 3 // 8 * 8 and bad == ok + 8
    # t3: vec 24 -> 2 pairs per segment, span = min(66, 128 / 2 + 2) = 66
    ok, _ = L.flip(lambda bs: L.t3_takes(66, 24, bs, 24), 96 * 24)
    assert ok == (F - 1 - 96 * 24 - 16) // 66 // 8 * 8
    assert L.t3_takes(3, 24, ok, 24) and L.t3_takes(3, 24, 10 * ok, 24)     # span = nb = 3
    # the runtime-coefficient kernel, flat: vec 8 -> nbg = 258; out slots k + m
    ok, _ = L.flip(lambda bs: L.rs8_rt_covers(8, bs, 8, 20, 30, False), 30 * 8)
    assert ok == (F - 1 - 30 * 8 - 8) // 258 // 8 * 8
    # ... per block: nbg = 1
    ok, _ = L.flip(lambda bs: L.rs8_rt_covers(1000, bs, 1008, 30, 30, True), 30 * 1008)
    assert ok == (F - 1 - 30 * 1008 - 1000) // 8 * 8
    # rt_dec adds the whole vector, not its 8-byte pieces
    ok, _ = L.flip(lambda bs: L.rt_dec(20, 10, 1003, bs, 1008), 30 * 1008)
    assert ok == (F - 1 - 30 * 1008 - 1003) // 8 * 8
    # tower: vec 64 -> nbg = 66; shared tables: nbg = 130; the split: 512 / 8 + 2 = 66
    assert L.flip(lambda bs: L.tw_prepare(64, bs, 64, 50), 50 * 64)[0] == (F - 1 - 50 * 64) // 66 // 8 * 8
    assert L.flip(lambda bs: L.t3_prepare(64, bs, 64, 50), 50 * 64)[0] == (F - 1 - 50 * 64) // 130 // 8 * 8
    for vec8 in (8, 24, 64, 1400, 1408, 4096, 8192):
        for bs in (F // 70, F // 66, F // 4, F // 3, F // 2):
            assert L.tmvp_offsets_fit(128, 32, vec8, bs, vec8) == L.tw_prepare(vec8, bs, vec8, 160)
    # the tower decode's second bound needs a slot stride near 2^31 / (k + m): never the layouts here
    assert L.rs16_twdec_covers(40, 10, 64, 50 * 64, 64) and not L.rs16_twdec_covers(40, 10, 64, F // 50 + 64, F // 50 + 8)


def test_routes_at_dense_layouts():
    """a dense batch takes the first rung of every ladder"""
    assert L.decode_route("RS8", 64, 32, 1400, 96 * 1400, 1400) == ("fixed", "RS8_FIXED")
    assert L.decode_route("RS8", 20, 10, 1003, 30 * 1008, 1008) == ("runtime", "RS8_RT")
    assert L.decode_route("RS8", 128, 127, 72, 255 * 72, 72) == ("runtime", "RS8_RT")
    assert L.decode_route("MDP", 64, 32, 1397, 96 * 1400, 1400) == ("runtime", "MDP_RT")
    assert L.decode_route("RS16", 40, 10, 66, 50 * 72, 72) == ("rs16_tower", "RS16_TOWER")
    assert L.decode_route("RS16", 32, 8, 64, 40 * 64, 64, tower=False) == ("generic", "RS_GENERIC/product")
    assert L.decode_route("RS16", 32, 8, 64, 40 * 64, 64, tower=False, short=True) == ("generic", "RS_GENERIC")
    assert L.decode_route("RS16", 300, 400, 64, 700 * 64, 64) == ("generic", "RS_GENERIC/product")   # min(k, m) > 256
    assert L.encode_rung("RS8", 64, 32, 1400, 5, 96 * 1400, 1400) == ("fixed", "rs8_t3")
    assert L.encode_rung("RS8", 64, 32, 1400, 5, 96 * 1400, 1400, short=True) == ("fixed", "rs8_q4_sh")
    assert L.encode_rung("RS8", 200, 55, 136, 5, 255 * 136, 136) == ("runtime", "rs8_rt")
    assert L.encode_rung("MDP", 64, 32, 1400, 5, 96 * 1400, 1400) == ("fixed", "mdp_q4")
    assert L.encode_rung("MDP", 30, 20, 203, 5, 50 * 208, 208, short=True) == ("runtime", "rs8_rt")
    assert L.encode_rung("RS16", 32, 8, 64, 5, 40 * 64, 64, tower=False) == ("rs16_product", "gf16_t3")
    assert L.encode_rung("RS16", 32, 8, 64, 5, 40 * 64, 64, tower=False, short=True) == ("generic", "gf16_bs_encode")


@pytest.mark.parametrize("name", ["A", "B", "C"])
@pytest.mark.parametrize("k,m,vec", [(64, 32, 1400), (64, 32, 1397), (20, 10, 1003), (40, 10, 66)])
def test_placements_are_legal_batches(name, k, m, vec):
    p = L.placements(k, m, vec)[name]
    lay = L.Layout(p["lead"], 5, p["slots"], p["seg_stride"], p["block_stride"])
    lay.check(k, m, vec)
    assert (lay.lead - L.BAND) % 16 == (8 if name in "AB" else 0)
    assert lay.block_stride > (k + m) * lay.seg_stride          # a block gap in every placement


def test_image_holds_every_byte_once_and_junk_differs():
    lay = L.Layout(L.BAND + 8, 3, 13, 40, 13 * 40 + 8)
    dense = np.arange(3 * 13 * 33, dtype=np.uint32).astype(np.uint8).reshape(3, 13, 33)
    img = L.put(None, lay, 33, dense, [13, 10, 13], 5)
    assert img.starts == [8] and img.bufs[0].size == lay.extent - 8     # everything merges into one run
    assert np.array_equal(L.get(img, 10), dense[:, :10])
    flat = img.bufs[0]
    assert len(set(flat[:L.BAND].tolist())) > 200                        # junk, not a constant
    assert not np.array_equal(img.slot(1, 10)[:33], dense[1, 10])        # an unused slot keeps its junk
    assert not np.array_equal(img.slot(0, 0)[33:], img.slot(0, 1)[33:])  # padding differs slot to slot
    other = L.put(None, lay, 33, dense, [13, 10, 13], 6)
    assert not np.array_equal(other.bufs[0], flat)


def test_image_of_a_sparse_batch_keeps_bands_only():
    lay = L.Layout(L.BAND + 8, 3, 96, 1400, 1 << 28)
    img = L.Image(lay, 1400)
    assert len(img.bufs) == 3
    assert all(b.size == 2 * L.BAND + 96 * 1400 for b in img.bufs)
    big = L.Image(L.Layout(L.BAND, 2, 8, 16 << 20, 8 * (16 << 20)), 1400)  # 256 MiB of slot bytes
    assert big.width == 1464 and sum(b.size for b in big.bufs) < (1 << 20)
    assert big.slot(1, 7).size == 1464


def test_check_untouched_sees_each_region():
    lay = L.Layout(L.BAND + 8, 2, 7, 24, 7 * 24 + 16)
    dense = np.zeros((2, 7, 20), np.uint8)
    before = L.put(None, lay, 20, dense, [6, 6], 1)
    masks = [L.writable("enc", False, 20, 4, 2, 7) for _ in range(2)]
    assert masks[0][4:6].all() and not masks[0][:4].any() and not masks[0][6].any()
    after = before.copy()
    after.slot(0, 4)[:20] ^= 0xFF        # parity: writable
    L.check_untouched(before, after, masks)
    for where in ("source", "padding", "spare slot", "gap", "band in front", "band behind"):
        bad = after.copy()
        if where == "source":
            bad.slot(1, 3)[0] ^= 1
        elif where == "padding":
            bad.slot(0, 5)[20] ^= 1
        elif where == "spare slot":
            bad.slot(1, 6)[3] ^= 1
        elif where == "gap":
            bad.bufs[0][lay.block(0) + lay.span + 9 - bad.starts[0]] ^= 1
        elif where == "band in front":
            bad.bufs[0][lay.block(0) - 1 - bad.starts[0]] ^= 1
        else:
            bad.bufs[0][-1] ^= 1
        with pytest.raises(AssertionError):
            L.check_untouched(before, bad, masks)
    # RS16 codes vec / 2 symbols: the odd last byte is not writable; decode: erased source only
    assert not L.writable("enc", True, 21, 4, 2, 7)[4:6, 20].any()
    d = L.writable("dec", False, 20, 4, 2, 7, erased=(1, 5))
    assert d[1].all() and d.sum() == 20
    assert not L.writable("dec", False, 20, 4, 2, 7, erased=(1,), decodable=False).any()
