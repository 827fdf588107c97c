"""Sender assembly on the device: nfec_tx_list and nfec_tx_emit.

Once a block's parity exists, NormObject::NextSenderMsg (reference src/common/normObject.cpp) walks
the blocks and their pending masks in order (:1877, :1989), picks each segment's payload length
(:2035, :2050, :2071), writes the FEC payload ID in front of it (:2078) and clears the pending bit
(:2075).  These tests hold the device path to that: the list against nfec_tx_list_host (itself held
to a plain-loop restatement in tests/test_tx_host.py, whose masks and lengths are used here too),
the wire buffer byte for byte against a NumPy assembly with nfec_payload_id_write's IDs, and the
whole chain encode -> list -> emit -> loss -> place -> repair against the oracle's source."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import norm_amd  # noqa: E402
from norm_amd import _native as N  # noqa: E402
from norm_amd import (NFEC_MDP, NFEC_RS8, NFEC_RS16, NormDecoderMDP, NormDecoderRS8, NormDecoderRS16,  # noqa: E402
                      NormEncoderMDP, NormEncoderRS8, NormEncoderRS16)
from test_tx_host import build_lengths, build_pending, num_data_for  # noqa: E402

ENC = {NFEC_RS8: NormEncoderRS8, NFEC_RS16: NormEncoderRS16, NFEC_MDP: NormEncoderMDP}
DEC = {NFEC_RS8: NormDecoderRS8, NFEC_RS16: NormDecoderRS16, NFEC_MDP: NormDecoderMDP}
SIGNED = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32, np.dtype(np.uint16): np.int16}
FIRST_BLOCK_ID = 0xFFFFFE  # the 24-bit block field of fec_id 5 wraps within a batch


def _dev(a):
    """a NumPy unsigned array as the signed torch tensor of the same bits, on the GPU"""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(SIGNED[a.dtype])).cuda()


def _np(t, dtype):
    return t.cpu().numpy().view(dtype)


def _list_np(res):
    return [_np(t, dt) for t, dt in zip(res, (np.uint64, np.uint32, np.uint16, np.uint16, np.uint64))]


LIST_SHAPES = [(NFEC_RS8, 8, 2, 1), (NFEC_RS8, 8, 2, 5), (NFEC_RS8, 8, 2, 4099), (NFEC_RS8, 64, 32, 24),
               (NFEC_RS16, 400, 100, 24), (NFEC_RS16, 4096, 256, 3)]


@pytest.mark.parametrize("kind,k,m,nb", LIST_SHAPES)
def test_list_equals_the_host_rule(kind, k, m, nb):
    """(8, 2, 4099) crosses the block scan's tiles of 1,024; (4096, 256, 3) has 136 mask words, three
    rounds of 64"""
    vec = 64 if k == 4096 else 1400
    rng = np.random.default_rng(k * 41 + m + nb)
    enc = ENC[kind]()
    assert enc.Init(k, m, vec)
    names = ("offsets", "block_index", "symbol_id", "length", "block_start")
    cut = nothing = 0
    for variant in range(5):
        nd = num_data_for(k, nb, variant)
        words = (k + m + 31) // 32 + variant % 2
        mask = build_pending(k, m, nd, rng, words, first=variant + (1 if nb == 1 else 0))
        mask2 = mask.copy()
        lstride = k + 3 * (variant % 2)
        lens, _ = build_lengths(k, m, vec, nd, mask2, rng, lstride)
        nothing += int(((nd < 1) | (nd > k)).sum())
        dnd, dlens = _dev(nd), _dev(lens)
        for gap in (0, 13):
            for pm, hl, dl in ((mask, None, None), (mask2, lens, dlens)):
                dmask = _dev(pm)
                want = norm_amd.tx_list_host(k, m, vec, pm, nd, hl, gap)
                got = _list_np(enc.list_pending(dmask, num_data=dnd, seg_length=dl, gap=gap))
                for name, g, w in zip(names, got, want):
                    assert np.array_equal(g, w), (variant, gap, hl is not None, name)
                assert np.array_equal(_np(dmask, np.uint32), pm)  # read only
                total = int(want[4][nb, 0])
                if total < 2:
                    continue
                # capacity below the total: the totals and block_start stay the full numbers, the first
                # `capacity` entries are written and nothing past them
                cap = total // 2
                arrs = [torch.full((total,), -86, dtype=dt, device="cuda")
                        for dt in (torch.int64, torch.int32, torch.int16, torch.int16)]
                start = torch.zeros((nb + 1, 2), dtype=torch.int64, device="cuda")
                rc = N.lib().nfec_tx_list(enc._h, dmask.data_ptr(), words, dnd.data_ptr(), nb,
                                          dl.data_ptr() if dl is not None else None, lstride if dl is not None else 0,
                                          gap, *[a.data_ptr() for a in arrs], cap, start.data_ptr(),
                                          torch.cuda.current_stream().cuda_stream)
                assert rc == N.NFEC_OK
                assert np.array_equal(_np(start, np.uint64), want[4])
                for a, w in zip(arrs, want[:4]):
                    a = a.cpu().numpy()
                    assert np.array_equal(a[:cap].view(w.dtype), w[:cap]) and (a[cap:] == -86).all()
                cut += 1
        if variant == 0 and nb > 1:  # num_data NULL = k
            full = build_pending(k, m, np.full(nb, k, np.uint16), rng, words)
            want = norm_amd.tx_list_host(k, m, vec, full, None, None, 13)
            got = _list_np(enc.list_pending(_dev(full), gap=13))
            for name, g, w in zip(names, got, want):
                assert np.array_equal(g, w), name
    assert cut and nothing


def _payload_id(fec_id, fec_m, block_id, s, nd):
    buf = np.zeros(8, np.uint8)
    n = N.lib().nfec_payload_id_write(fec_id, fec_m, block_id & 0xFFFFFFFF, s, nd, buf.ctypes.data)
    assert n == N.lib().nfec_payload_id_length(fec_id)
    return buf[:n]


def _idlen(fec_id):
    return N.lib().nfec_payload_id_length(fec_id) if fec_id else 0


def numpy_emit(wire, batch, entries, fec_id, fec_m, nd):
    for off, b, s, ln in entries:
        if fec_id:
            pid = _payload_id(fec_id, fec_m, FIRST_BLOCK_ID + b, s, int(nd[b]))
            wire[off - len(pid):off] = pid
        wire[off:off + ln] = batch[b, s, :ln]


def _upload(entries, rng=None):
    e = list(entries)
    if rng is not None:
        e = [e[i] for i in rng.permutation(len(e))]
    cols = list(zip(*e)) if e else [(), (), (), ()]
    return dict(offsets=_dev(np.array(cols[0], np.uint64)), block_index=_dev(np.array(cols[1], np.uint32)),
                symbol_id=_dev(np.array(cols[2], np.uint16)), length=_dev(np.array(cols[3], np.uint16)))


def wire_layout(rng, idlen, vec, slots):
    """Messages laid one after the other: every length class at every residue of the payload offset
    modulo 16; about every other message starts right behind the one before it (only its payload ID
    between the two payloads), the rest behind a junk gap.  Returns (entries, touching, pairs seen,
    wire bytes)."""
    lengths = [0, 1, 7, 8, 9, 15, 16, 17, vec - 1, vec]
    need = [(ln, r) for ln in lengths for r in range(16)]
    need = [need[i] for i in rng.permutation(len(need))]
    entries, seen, touching = [], set(), 0
    pos = 0  # the end of the message before
    slot_iter = iter(slots)

    def add(ln, off, touch):
        nonlocal pos, touching
        b, s = next(slot_iter)
        entries.append((off, b, s, ln))
        seen.add((ln, off % 16))
        touching += touch
        pos = off + ln

    # the first of `slots`, the batch's last slot, goes out whole: the read rule's edge
    add(vec, idlen + 3, 0)
    need.remove((vec, (idlen + 3) % 16))
    while need:
        res = (pos + idlen) % 16
        fit = next((p for p in need if p[1] == res), None) if entries and len(entries) % 2 else None
        if fit is not None:
            need.remove(fit)
            add(fit[0], pos + idlen, 1)
        else:
            ln, r = need.pop()
            off = pos + idlen + 1
            off += (r - off) % 16
            add(ln, off, 0)
    while touching * 2 < len(entries):  # make up for the steps no needed pair fitted
        add(int(rng.integers(0, vec + 1)), pos + idlen, 1)
    return entries, touching, seen, pos + 29


EMIT_SHAPES = [(NFEC_RS8, 8, 2, 24, 24), (NFEC_RS8, 64, 32, 1405, 1408), (NFEC_RS16, 400, 100, 1460, 1464)]
FEC = [(0, 8), (5, 8), (2, 16), (129, 8)]


@pytest.mark.parametrize("kind,k,m,vec,stride", EMIT_SHAPES)
def test_emission_is_byte_exact(kind, k, m, vec, stride):
    """The shapes and numData of the receiver's placement test (numData's last two values change
    places: the batch's very last slot, which ends the allocation, must be a slot of its block)."""
    rng = np.random.default_rng(k * 131 + vec)
    nb = 6
    nd = np.array([k, max(1, k // 2), k - 1, 1, max(1, k - 3), k], np.uint16)
    enc = ENC[kind]()
    assert enc.Init(k, m, vec)
    batch = rng.integers(1, 256, (nb, k + m, stride), dtype=np.uint8)
    dbatch = torch.from_numpy(batch.copy()).cuda()
    dnd = _dev(nd)
    last_slot = (nb - 1, k + m - 1)
    must = [last_slot] + [(b, 0) for b in range(nb)] + [(b, int(nd[b]) + m - 1) for b in range(nb - 1)]
    valid = [(b, s) for b in range(nb) for s in range(int(nd[b]) + m)]
    for fec_id, fec_m in FEC:
        idlen = _idlen(fec_id)
        slots = must + [valid[i] for i in rng.integers(0, len(valid), 400)]
        entries, touching, seen, nbytes = wire_layout(rng, idlen, vec, slots)
        assert all((ln, r) in seen for ln in (0, 1, 7, 8, 9, 15, 16, 17, vec - 1, vec) for r in range(16))
        assert touching * 2 >= len(entries) and len(entries) - touching >= 40
        assert set(must) <= {(b, s) for _, b, s, _ in entries}
        assert (last_slot[0], last_slot[1], vec) in {(b, s, ln) for _, b, s, ln in entries}
        junk = rng.integers(1, 256, nbytes, dtype=np.uint8)
        want = junk.copy()
        numpy_emit(want, batch, entries, fec_id, fec_m, nd)
        wire = torch.from_numpy(junk.copy()).cuda()
        stats = torch.zeros(2, dtype=torch.int32, device="cuda")
        enc.emit_segments(dbatch, wire, num_data=dnd, fec_id=fec_id, fec_m=fec_m, first_block_id=FIRST_BLOCK_ID,
                          stats=stats, **_upload(entries, rng))
        torch.cuda.synchronize()
        got = wire.cpu().numpy()
        assert stats.cpu().tolist() == [len(entries), 0]
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (fec_id, bad[:8], len(bad))
    assert np.array_equal(dbatch.cpu().numpy(), batch)


def test_rejections_mask_and_count_dev():
    k, m, vec, stride = 64, 32, 1405, 1408
    fec_id, fec_m, idlen = 5, 8, 4
    rng = np.random.default_rng(11)
    nd = np.array([64, 40, 0, 64, 65], np.uint16)
    nb = len(nd)
    enc = NormEncoderRS8()
    assert enc.Init(k, m, vec)
    batch = rng.integers(1, 256, (nb, k + m, stride), dtype=np.uint8)
    dbatch = torch.from_numpy(batch.copy()).cuda()
    dnd = _dev(nd)
    P = 16 * 1500 + 5
    good = [
        (idlen, 0, 5, vec),                    # the first message: off == idlen
        (1500 + 3, 1, 40 + m - 1, 11),         # a shortened block's last parity slot
        (3000 + 7, 3, 0, 0),                   # an empty payload: the ID alone
        (4500 + 9, 3, k + m - 1, vec),
        (P - 77, 0, k, 77),                    # ends exactly at payload_bytes
    ]
    bad = [
        (6000 + 1, nb, 0, 16),                 # block_index == nblocks
        (7500 + 2, 2, 0, 16),                  # numData 0
        (9000 + 3, 4, 0, 16),                  # numData k + 1
        (10500 + 4, 1, 40 + m, 16),            # symbol_id == nd_b + m
        (12000 + 5, 0, 6, vec + 1),            # length == vec + 1
        (idlen - 1, 0, 7, 16),                 # off < idlen
        (P - 76, 3, 9, 77),                    # off + len == payload_bytes + 1
        (P + 8, 3, 10, 0),                     # off beyond the buffer
    ]
    held = [(13500 + 6, 0, 20, 100), (15000 + 7, 3, 21, vec)]  # good, but past *count_dev
    junk = rng.integers(1, 256, P, dtype=np.uint8)
    words = 4  # one more than (k + m + 31) / 32
    ones = np.full((nb, words), 0xFFFFFFFF, np.uint32)

    def run(entries, count_dev, pending, shuffle):
        wire = torch.from_numpy(junk.copy()).cuda()
        stats = torch.zeros(2, dtype=torch.int32, device="cuda")
        mask = _dev(pending) if pending is not None else None
        enc.emit_segments(dbatch, wire, count_dev=count_dev, num_data=dnd, fec_id=fec_id, fec_m=fec_m,
                          first_block_id=FIRST_BLOCK_ID, pending=mask, stats=stats,
                          **_upload(entries, rng if shuffle else None))
        torch.cuda.synchronize()
        return wire.cpu().numpy(), stats.cpu().tolist(), None if mask is None else _np(mask, np.uint32)

    want = junk.copy()
    numpy_emit(want, batch, good, fec_id, fec_m, nd)
    want_mask = ones.copy()
    for _, b, s, _ in good:
        want_mask[b, s // 32] &= np.uint32(~(1 << (s % 32)) & 0xFFFFFFFF)
    # good and bad entries mixed; every rejected entry's bit stays set
    got, stats, mask = run(good + bad, None, ones, True)
    assert stats == [len(good), len(bad)]
    assert np.array_equal(got, want)
    assert np.array_equal(mask, want_mask)
    # count_dev below count: the entries past it write nothing and clear nothing
    order = [good[0], bad[0], good[1], bad[4], good[2], good[3], bad[6], good[4]] + held
    cd = torch.tensor([len(order) - len(held)], dtype=torch.int64, device="cuda")
    got, stats, mask = run(order, cd, ones, False)
    assert stats == [len(good), 3]
    assert np.array_equal(got, want) and np.array_equal(mask, want_mask)
    # count_dev above count: count bounds it; no mask, no stats
    cd = torch.tensor([1 << 40], dtype=torch.int64, device="cuda")
    got, stats, mask = run(order, cd, None, False)
    numpy_emit(want, batch, held, fec_id, fec_m, nd)
    assert stats == [len(good) + len(held), 3] and np.array_equal(got, want)
    wire = torch.from_numpy(junk.copy()).cuda()
    enc.emit_segments(dbatch, wire, num_data=dnd, fec_id=fec_id, first_block_id=FIRST_BLOCK_ID, **_upload(good))
    # zero entries and zero blocks: NFEC_OK, nothing written
    enc.emit_segments(dbatch, wire, num_data=dnd, fec_id=fec_id, **_upload([]))
    none = torch.zeros((0, k + m, stride), dtype=torch.uint8, device="cuda")
    enc.emit_segments(none, wire, fec_id=fec_id, **_upload(good))
    torch.cuda.synchronize()
    ref = junk.copy()
    numpy_emit(ref, batch, good, fec_id, fec_m, nd)
    assert np.array_equal(wire.cpu().numpy(), ref)
    assert np.array_equal(dbatch.cpu().numpy(), batch)


LOOP = [
    # kind, k, m, vec, seg stride, fec_id, fec_m
    (NFEC_RS8, 64, 32, 1405, 1408, 5, 8),
    (NFEC_RS8, 8, 2, 24, 24, 2, 8),
    (NFEC_RS16, 400, 100, 1460, 1464, 2, 16),
    (NFEC_MDP, 64, 32, 1400, 1400, 129, 8),
]


@pytest.mark.parametrize("kind,k,m,vec,stride,fec_id,fec_m", LOOP)
def test_loopback_against_the_oracles_source(orc, kind, k, m, vec, stride, fec_id, fec_m):
    """encode -> list -> emit -> loss -> place -> repair, all on the device"""
    rng = np.random.default_rng(k * 19 + m + vec)
    nb, gap = 8, 13
    p = min(m, 8)  # parity segments sent per block; p - 1 source segments are lost
    nd = np.full(nb, k, np.uint16)
    nd[[2, 5]] = [k - 1, max(p, k // 2)]
    host = orc.make_blocks(k, m, vec, nb, seg_stride=stride, num_data=nd)
    # block 3's last source segment is short: the sender pads the runt with zeros before it encodes
    # (normObject.cpp:2047-2048) and sends only its own bytes
    lens = np.full((nb, k), vec, np.uint16)
    short = vec // 3
    lens[3, nd[3] - 1] = short
    host[3, nd[3] - 1, short:] = 0
    enc, dec = ENC[kind](), DEC[kind]()
    assert enc.Init(k, m, vec) and dec.Init(k, m, vec)
    dev = torch.from_numpy(host.copy()).cuda()
    dnd = _dev(nd)
    words = (k + m + 31) // 32
    pend = np.zeros((nb, words), np.uint32)
    for b in range(nb):
        for s in range(int(nd[b]) + p):
            pend[b, s // 32] |= np.uint32(1 << (s % 32))
    dpend = _dev(pend)
    count = int(nd.sum()) + nb * p
    nbytes = count * (gap + vec) - (vec - short)
    wire = torch.from_numpy(rng.integers(1, 256, nbytes + 40, dtype=np.uint8)).cuda()
    stats = torch.zeros(2, dtype=torch.int32, device="cuda")
    # 1-4: encode, list, emit chained on the stream: the list's total bounds the emission on the device
    enc.encode_blocks(dev, num_data=dnd)
    off, blk, sym, ln, start = enc.list_pending(dpend, num_data=dnd, seg_length=_dev(lens), gap=gap)
    enc.emit_segments(dev, wire, off, blk, sym, ln, count_dev=start[nb, :1], fec_id=fec_id, fec_m=fec_m,
                      first_block_id=FIRST_BLOCK_ID, pending=dpend, num_data=dnd, stats=stats)
    torch.cuda.synchronize()
    assert _np(start, np.uint64)[nb].tolist() == [count, nbytes]
    assert stats.cpu().tolist() == [count, 0]
    assert not _np(dpend, np.uint32).any()  # every pending bit was cleared
    h_off, h_blk, h_sym, h_ln = [a[:count] for a in _list_np((off, blk, sym, ln, start))[:4]]
    # what a receiver reads in front of every payload
    hw = wire.cpu().numpy()
    bid, sid, blen = ctypes.c_uint32(), ctypes.c_uint16(), ctypes.c_uint16()
    idlen = _idlen(fec_id)
    # the fields' widths: fec_id 5 and 2 / m 8 carry 24 + 8 bits, 2 / m 16 16 + 16, 129 32 + 16
    bmask, smask = {(5, 8): (0xFFFFFF, 0xFF), (2, 8): (0xFFFFFF, 0xFF), (2, 16): (0xFFFF, 0xFFFF),
                    (129, 8): (0xFFFFFFFF, 0xFFFF)}[(fec_id, fec_m)]
    for i in range(count):
        at = int(h_off[i]) - idlen
        assert N.lib().nfec_payload_id_read(fec_id, fec_m, hw[at:].ctypes.data, ctypes.byref(bid), ctypes.byref(sid),
                                            ctypes.byref(blen)) == idlen
        assert (bid.value, sid.value) == ((FIRST_BLOCK_ID + int(h_blk[i])) & bmask, int(h_sym[i]) & smask)
        assert fec_id != 129 or blen.value == nd[h_blk[i]]
    assert h_ln[(h_blk == 3) & (h_sym == nd[3] - 1)].tolist() == [short]
    # 5: the loss, on the host: p - 1 source segments of every block never arrive; the rest out of order
    keep = np.ones(count, bool)
    for b in range(nb):
        mine = np.nonzero((h_blk == b) & (h_sym < nd[b]))[0]
        keep[rng.choice(mine, p - 1, replace=False)] = False
    order = rng.permutation(np.nonzero(keep)[0])
    # 6-7: place into a junk-filled batch, repair from the reception mask
    dev2 = torch.from_numpy(rng.integers(1, 256, host.shape, dtype=np.uint8)).cuda()
    mask = norm_amd.received_mask(nb, k, m)
    rstats = torch.zeros(3, dtype=torch.int32, device="cuda")
    dec.place_segments(dev2, mask, wire, _dev(h_off[order]), _dev(h_blk[order]), _dev(h_sym[order]),
                       _dev(h_ln[order]), num_data=dnd, stats=rstats)
    st = dec.decode_received(dev2, mask, num_data=dnd)
    torch.cuda.synchronize()
    assert rstats.cpu().tolist() == [len(order), 0, 0]
    # the erasure lists: the lost source segments and the parity that was never sent
    erasures = (p - 1) + (m - p) if p > 1 else 0
    assert st.cpu().tolist() == [erasures] * nb
    got = dev2.cpu().numpy()
    sent = dev.cpu().numpy()
    for b in range(nb):
        n = int(nd[b])
        assert np.array_equal(got[b, :n, :vec], sent[b, :n, :vec]), b
        assert np.array_equal(got[b, :n, :vec], host[b, :n, :vec]), b
