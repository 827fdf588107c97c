"""Receiver intake on the device: nfec_rx_ingest.

nfec_tx_emit's mirror: a receiver whose datagrams are in device memory hands over the wire buffer
and, per message, where its payload lies; the FEC payload ID in front of the payload (NormPayloadId,
reference include/normMessage.h:396-567) names the block and the slot, and the payload is placed as
NormObject::HandleObjectMessage places it (src/common/normObject.cpp:1548-1644).  These tests hold the
call to nfec_rx_parse_host (itself held to oracle/wire_ref.py in tests/test_rx_parse_host.py) followed
by nfec_rx_place, byte for byte, and run the whole chain object -> blocks -> parity -> wire -> blocks
-> repair -> object on one stream without a descriptor built on the host."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import norm_amd  # noqa: E402
from norm_amd import _native as N  # noqa: E402
from norm_amd import (NFEC_MDP, NFEC_RS8, NFEC_RS16, NormDecoderMDP, NormDecoderRS8, NormDecoderRS16,  # noqa: E402
                      NormEncoderRS8)
from oracle import wire_ref as R  # noqa: E402
from test_gpu_tx import FIRST_BLOCK_ID, _dev, _np, numpy_emit, wire_layout  # noqa: E402
from test_tx_host import num_data_for  # noqa: E402

DEC = {NFEC_RS8: NormDecoderRS8, NFEC_RS16: NormDecoderRS16, NFEC_MDP: NormDecoderMDP}
FILL = 0xA5
BITS = {(5, 8): 24, (2, 8): 24, (2, 16): 16, (129, 8): 32}
ALL_ONES = (0xFFFFFFFF, 0xFFFF)

# kind, k, m, vec, seg stride, blocks, fec_id, fec_m: the smallest shapes that reach every branch.
# 1,400 bytes are 88 pieces of 16, so a wave needs a second round; vec 40 / 41 end in a whole and in
# a partial 8-byte piece below a 48-byte stride
SHAPES = [
    (NFEC_RS8, 8, 2, 40, 48, 5, 2, 8),
    (NFEC_RS8, 64, 32, 1400, 1400, 3, 5, 8),
    (NFEC_RS16, 400, 100, 1400, 1400, 2, 2, 16),
    (NFEC_MDP, 8, 2, 41, 48, 5, 129, 8),
]
IDS = ["%d-%d-fec%d" % (s[1], s[3], s[6]) for s in SHAPES]


def _decoder(kind, k, m, vec):
    dec = DEC[kind]()
    assert dec.Init(k, m, vec)
    return dec


def _idlen(fec_id):
    return N.lib().nfec_payload_id_length(fec_id)


def _filled(nb, k, m, stride):
    return torch.full((nb, k + m, stride), FILL, dtype=torch.uint8, device="cuda")


def _outputs(n):
    return (torch.full((n,), -86, dtype=torch.int32, device="cuda"),
            torch.full((n,), -86, dtype=torch.int16, device="cuda"))


def _emit(wire, batch, entries, fec_id, fec_m, first, nd):
    """numpy_emit with any first_block_id: oracle/wire_ref.py's ID, then the slot's first bytes"""
    field = (1 << BITS[(fec_id, fec_m)]) - 1
    for off, b, s, ln in entries:
        pid = np.frombuffer(R.payload_id(fec_id, fec_m, (first + b) & field, s, int(nd[b])), np.uint8)
        wire[off - len(pid):off] = pid
        wire[off:off + ln] = batch[b, s, :ln]


def _accepts(b, s, ln, nb, nd, k, m, vec):
    return b < nb and 1 <= int(nd[b]) <= k and s < int(nd[b]) + m and ln <= vec


@pytest.mark.parametrize("kind,k,m,vec,stride,nb,fec_id,fec_m", SHAPES, ids=IDS)
def test_ingest_equals_host_parse_and_place(kind, k, m, vec, stride, nb, fec_id, fec_m):
    """Every length class at every residue of the payload offset, touching messages and junk gaps
    (wire_layout), shortened and invalid numData.  The messages go in as calls in which no slot
    appears twice (a pass over every slot of the batch, in shuffled arrival order), so what a call
    leaves does not depend on which wave runs first; the masks start each call at zero."""
    rng = np.random.default_rng(k * 53 + vec + fec_id)
    dec = _decoder(kind, k, m, vec)
    idlen = _idlen(fec_id)
    nd = num_data_for(k, nb, 0)
    assert nb < 5 or ((nd < 1) | (nd > k)).any()
    src = rng.integers(1, 256, (nb, k + m, stride), dtype=np.uint8)
    every = [(b, s) for b in range(nb) for s in range(k + m)]
    passes = [[every[i] for i in rng.permutation(len(every))] for _ in range(400 // len(every) + 1)]
    entries, touching, seen, nbytes = wire_layout(rng, idlen, vec, [p for one in passes for p in one])
    assert all((ln, r) in seen for ln in (0, 1, 7, 8, 9, 15, 16, 17, vec - 1, vec) for r in range(16))
    assert touching * 2 >= len(entries)
    wire = rng.integers(1, 256, nbytes, dtype=np.uint8)
    numpy_emit(wire, src, entries, fec_id, fec_m, nd)
    dwire = torch.from_numpy(wire.copy()).cuda()
    dnd = _dev(nd)
    words = (k + m + 31) // 32 + 1
    dev_a, dev_b = _filled(nb, k, m, stride), _filled(nb, k, m, stride)
    mask_a = torch.zeros((nb, words), dtype=torch.int32, device="cuda")
    mask_b = torch.zeros_like(mask_a)
    placed = rejected = 0
    for at in range(0, len(entries), len(every)):
        call = entries[at:at + len(every)]
        call = [call[i] for i in rng.permutation(len(call))]
        off = np.array([e[0] for e in call], np.uint64)
        ln = np.array([e[3] for e in call], np.uint16)
        h_blk, h_sym, h_len = norm_amd.rx_parse_host(fec_id, fec_m, FIRST_BLOCK_ID, wire, off, ln)
        assert h_blk.tolist() == [e[1] for e in call] and h_sym.tolist() == [e[2] for e in call]
        assert fec_id != 129 or h_len.tolist() == [int(nd[e[1]]) for e in call]
        mask_a.zero_()
        mask_b.zero_()
        stats_a = torch.zeros(3, dtype=torch.int32, device="cuda")
        stats_b = torch.zeros(3, dtype=torch.int32, device="cuda")
        out_blk, out_sym = _outputs(len(call))
        doff, dln = _dev(off), _dev(ln)
        dec.ingest_messages(dev_a, mask_a, dwire, doff, dln, fec_id, fec_m, first_block_id=FIRST_BLOCK_ID,
                            num_data=dnd, block_index_out=out_blk, symbol_id_out=out_sym, stats=stats_a)
        dec.place_segments(dev_b, mask_b, dwire, doff, _dev(h_blk), _dev(h_sym), dln, num_data=dnd, stats=stats_b)
        torch.cuda.synchronize()
        got, ref = dev_a.cpu().numpy(), dev_b.cpu().numpy()
        assert stats_a.cpu().tolist() == stats_b.cpu().tolist()
        assert np.array_equal(_np(mask_a, np.uint32), _np(mask_b, np.uint32))
        bad = np.argwhere(got != ref)
        assert bad.size == 0, (at, bad[:4], len(bad))
        assert (got[:, :, vec:] == FILL).all()  # the stride padding keeps the caller's bytes
        assert np.array_equal(_np(out_blk, np.uint32), h_blk) and np.array_equal(_np(out_sym, np.uint16), h_sym)
        # and against the sender's batch: the payload, then zeros up to vec
        want = [_accepts(b, s, n, nb, nd, k, m, vec) for _, b, s, n in call]
        assert stats_a.cpu().tolist() == [sum(want), 0, len(call) - sum(want)]
        for (_, b, s, n), ok in zip(call, want):
            if ok:
                assert np.array_equal(got[b, s, :n], src[b, s, :n]) and not got[b, s, n:vec].any(), (b, s, n)
        placed += sum(want)
        rejected += len(call) - sum(want)
    assert placed >= 50 and (rejected or nb < 3)
    assert torch.equal(dwire.cpu(), torch.from_numpy(wire))  # read only


WRAP = [
    # kind, k, m, vec, seg stride, fec_id, fec_m, first_block_id: two below the block field's wrap
    (NFEC_RS8, 8, 2, 40, 48, 5, 8, 0xFFFFFE),
    (NFEC_RS8, 8, 2, 40, 48, 2, 8, 0xFFFFFE),
    (NFEC_RS16, 400, 100, 1400, 1400, 2, 16, 0xFFFE),
    (NFEC_MDP, 8, 2, 41, 48, 129, 8, 0xFFFFFFFE),
    # the same window seen through a narrower field: only the field's bits of first_block_id count
    (NFEC_RS8, 8, 2, 40, 48, 5, 8, 0xABFFFFFE),
    (NFEC_RS16, 400, 100, 1400, 1400, 2, 16, 0x1234FFFE),
]


@pytest.mark.parametrize("kind,k,m,vec,stride,fec_id,fec_m,first", WRAP)
def test_windows_that_wrap_the_block_field(kind, k, m, vec, stride, fec_id, fec_m, first):
    rng = np.random.default_rng(k + fec_id + fec_m)
    nb = 5  # block IDs wrap - 2, wrap - 1, 0, 1, 2
    dec = _decoder(kind, k, m, vec)
    idlen = _idlen(fec_id)
    nd = np.full(nb, k, np.uint16)
    src = rng.integers(1, 256, (nb, k + m, stride), dtype=np.uint8)
    slots = [(b, s) for b in range(nb) for s in range(k + m)]
    if len(slots) > 300:  # a few hundred messages are enough; every block stays among them
        slots = [slots[i] for i in rng.permutation(len(slots))[:300]]
    entries, pos = [], 0
    for b, s in slots:
        ln = int(rng.integers(0, vec + 1))
        off = pos + idlen + int(rng.integers(0, 5))
        entries.append((off, b, s, ln))
        pos = off + ln
    wire = rng.integers(1, 256, pos + 7, dtype=np.uint8)
    _emit(wire, src, entries, fec_id, fec_m, first, nd)
    entries = [entries[i] for i in rng.permutation(len(entries))]
    dev = _filled(nb, k, m, stride)
    mask = norm_amd.received_mask(nb, k, m)
    stats = torch.zeros(3, dtype=torch.int32, device="cuda")
    out_blk, out_sym = _outputs(len(entries))
    dec.ingest_messages(dev, mask, torch.from_numpy(wire).cuda(), _dev(np.array([e[0] for e in entries], np.uint64)),
                        _dev(np.array([e[3] for e in entries], np.uint16)), fec_id, fec_m, first_block_id=first,
                        block_index_out=out_blk, symbol_id_out=out_sym, stats=stats)
    torch.cuda.synchronize()
    assert stats.cpu().tolist() == [len(entries), 0, 0]
    assert _np(out_blk, np.uint32).tolist() == [e[1] for e in entries]
    assert _np(out_sym, np.uint16).tolist() == [e[2] for e in entries]
    want = np.full(src.shape, FILL, np.uint8)
    want_mask = np.zeros((nb, (k + m + 31) // 32), np.uint32)
    for _, b, s, ln in entries:
        want[b, s, :ln] = src[b, s, :ln]
        want[b, s, ln:vec] = 0
        want_mask[b, s // 32] |= np.uint32(1 << (s % 32))
    assert {e[1] for e in entries} == set(range(nb))
    assert np.array_equal(dev.cpu().numpy(), want)
    assert np.array_equal(_np(mask, np.uint32), want_mask)


@pytest.mark.parametrize("kind,k,m,vec,stride,fec_id,fec_m", [(NFEC_MDP, 8, 2, 41, 48, 129, 8),
                                                              (NFEC_RS8, 8, 2, 40, 48, 5, 8)])
def test_rejections_write_nothing(kind, k, m, vec, stride, fec_id, fec_m):
    rng = np.random.default_rng(5 + fec_id)
    dec = _decoder(kind, k, m, vec)
    idlen = _idlen(fec_id)
    nd = np.array([k, k - 1, 1, 0, k + 1], np.uint16)
    nb = len(nd)
    first = 0xFFFFFE
    P = 1024
    wire = rng.integers(1, 256, P, dtype=np.uint8)

    def put(off, block, s, block_len):
        wire[off - idlen:off] = np.frombuffer(R.payload_id(fec_id, fec_m, (first + block) & 0xFFFFFF if fec_id != 129
                                                            else first + block, s, block_len), np.uint8)

    # (offset, length, unreadable)
    msgs = [(idlen - 1, 3, True),          # the ID would start in front of the buffer
            (P - 10, 11, True),            # the payload ends one past payload_bytes
            (100, 16, False),              # block nblocks
            (200 + 3, 16, False),          # symbol nd_b + m of a shortened block
            (300 + 5, vec + 1, False),     # longer than the vector
            (500 + 7, 16, False),          # a block whose numData is 0
            (600 + 9, 16, False)]          # ... and one whose numData is k + 1
    put(P - 10, 0, 0, k)                   # (a well-formed ID: only the payload's end is wrong)
    put(100, nb, 0, k)
    put(200 + 3, 1, k - 1 + m, k - 1)
    put(300 + 5, 0, 3, k)
    put(500 + 7, 3, 0, 0)
    put(600 + 9, 4, 0, k + 1)
    if fec_id == 129:
        msgs.append((700 + 11, 16, False))  # the ID's block length is not the block's numData
        put(700 + 11, 0, 4, k - 1)
    off = np.array([x[0] for x in msgs], np.uint64)
    ln = np.array([x[1] for x in msgs], np.uint16)
    h_blk, h_sym, _ = norm_amd.rx_parse_host(fec_id, fec_m, first, wire, off, ln)
    dev = _filled(nb, k, m, stride)
    mask = norm_amd.received_mask(nb, k, m)
    stats = torch.zeros(3, dtype=torch.int32, device="cuda")
    out_blk, out_sym = _outputs(len(msgs))
    dec.ingest_messages(dev, mask, torch.from_numpy(wire).cuda(), _dev(off), _dev(ln), fec_id, fec_m,
                        first_block_id=first, num_data=_dev(nd), block_index_out=out_blk, symbol_id_out=out_sym,
                        stats=stats)
    torch.cuda.synchronize()
    assert stats.cpu().tolist() == [0, 0, len(msgs)]
    assert (dev.cpu().numpy() == FILL).all() and not mask.any()
    got = list(zip(_np(out_blk, np.uint32).tolist(), _np(out_sym, np.uint16).tolist()))
    assert got == list(zip(h_blk.tolist(), h_sym.tolist()))
    assert [g == ALL_ONES for g in got] == [x[2] for x in msgs]
    assert got[2][0] == nb and got[3] == (1, k - 1 + m)


def test_duplicates():
    k, m, vec, stride, nb = 64, 32, 1400, 1400, 3
    fec_id, fec_m, idlen, first = 5, 8, 4, 7
    rng = np.random.default_rng(17)
    dec = _decoder(NFEC_RS8, k, m, vec)
    wire = rng.integers(1, 256, 8192, dtype=np.uint8)

    def put(off, b, s):
        wire[off - idlen:off] = np.frombuffer(R.payload_id(fec_id, fec_m, first + b, s), np.uint8)

    put(16 + 5, 1, 9)        # the message listed three times, then once more
    put(1600 + 11, 2, 40)    # two payloads for one slot
    put(3200 + 2, 2, 40)
    put(4800 + 14, 0, 0)     # a bystander
    dwire = torch.from_numpy(wire).cuda()
    dev = _filled(nb, k, m, stride)
    mask = norm_amd.received_mask(nb, k, m)
    stats = torch.zeros(3, dtype=torch.int32, device="cuda")
    one = [(16 + 5, vec)] * 3 + [(1600 + 11, vec), (3200 + 2, vec - 5), (4800 + 14, 9)]
    one = [one[i] for i in rng.permutation(len(one))]
    two = [(16 + 5, vec), (4800 + 14, 9)]
    for msgs in (one, two):
        dec.ingest_messages(dev, mask, dwire, _dev(np.array([x[0] for x in msgs], np.uint64)),
                            _dev(np.array([x[1] for x in msgs], np.uint16)), fec_id, fec_m, first_block_id=first,
                            stats=stats)
    torch.cuda.synchronize()
    got = dev.cpu().numpy()
    # three slots placed once each.  Duplicates: 2 + 1 = 3 copies of the first message over the two
    # calls, and beside them the loser of the contested pair and the bystander's second arrival
    assert stats.cpu().tolist() == [3, 3 + 2, 0]
    assert np.array_equal(got[1, 9, :vec], wire[21:21 + vec])
    a = wire[1611:1611 + vec]
    b = np.concatenate([wire[3202:3202 + vec - 5], np.zeros(5, np.uint8)])
    assert np.array_equal(got[2, 40, :vec], a) or np.array_equal(got[2, 40, :vec], b)  # one of them, whole
    assert np.array_equal(got[0, 0, :9], wire[4814:4823]) and not got[0, 0, 9:vec].any()
    want_mask = np.zeros((nb, 3), np.uint32)
    for b_, s_ in ((1, 9), (2, 40), (0, 0)):
        want_mask[b_, s_ // 32] |= np.uint32(1 << (s_ % 32))
    assert np.array_equal(_np(mask, np.uint32), want_mask)
    got[1, 9] = got[2, 40] = got[0, 0] = FILL
    assert (got == FILL).all()


def test_count_dev_bounds_the_messages():
    k, m, vec, stride, nb = 8, 2, 40, 48, 5
    fec_id, fec_m, idlen, first = 2, 8, 4, 0xFFFFFE
    rng = np.random.default_rng(23)
    dec = _decoder(NFEC_RS8, k, m, vec)
    src = rng.integers(1, 256, (nb, k + m, stride), dtype=np.uint8)
    nd = np.full(nb, k, np.uint16)
    slots = [(b, s) for b in range(nb) for s in range(k + m)]
    slots = [slots[i] for i in rng.permutation(len(slots))]
    entries = [(idlen + i * (vec + idlen + 3), b, s, vec - i % 7) for i, (b, s) in enumerate(slots)]
    wire = rng.integers(1, 256, entries[-1][0] + vec + 1, dtype=np.uint8)
    _emit(wire, src, entries, fec_id, fec_m, first, nd)
    dwire = torch.from_numpy(wire).cuda()
    off = _dev(np.array([e[0] for e in entries], np.uint64))
    ln = _dev(np.array([e[3] for e in entries], np.uint16))
    for have, done in ((37, 37), (0, 0), (1 << 40, len(entries))):  # below count, nothing, above count
        dev = _filled(nb, k, m, stride)
        mask = norm_amd.received_mask(nb, k, m)
        stats = torch.zeros(3, dtype=torch.int32, device="cuda")
        out_blk, out_sym = _outputs(len(entries))
        cd = torch.tensor([have], dtype=torch.int64, device="cuda")
        dec.ingest_messages(dev, mask, dwire, off, ln, fec_id, fec_m, first_block_id=first, count_dev=cd,
                            block_index_out=out_blk, symbol_id_out=out_sym, stats=stats)
        torch.cuda.synchronize()
        assert stats.cpu().tolist() == [done, 0, 0]
        want = np.full(src.shape, FILL, np.uint8)
        for _, b, s, n in entries[:done]:
            want[b, s, :n] = src[b, s, :n]
            want[b, s, n:vec] = 0
        assert np.array_equal(dev.cpu().numpy(), want)
        ob, os_ = out_blk.cpu().numpy(), out_sym.cpu().numpy()
        assert ob[:done].tolist() == [e[1] for e in entries[:done]] and (ob[done:] == -86).all()
        assert os_[:done].tolist() == [e[2] for e in entries[:done]] and (os_[done:] == -86).all()
        assert int(np.unpackbits(_np(mask, np.uint32).view(np.uint8)).sum()) == done


@pytest.mark.parametrize("k,m,seg,vec,stride,nb", [(8, 2, 32, 40, 48, 7), (64, 32, 1392, 1400, 1400, 4)])
def test_whole_chain_on_one_stream_without_a_host_descriptor(orc, k, m, seg, vec, stride, nb):
    """read_object -> encode_blocks -> list_pending -> emit_segments -> ingest_messages ->
    decode_received -> write_object with no synchronize and no host-built array between them: the
    intake takes the list's offsets / length tensors and its total as they lie in device memory"""
    rng = np.random.default_rng(k * 31 + seg)
    enc, dec = NormEncoderRS8(), NormDecoderRS8()
    assert enc.Init(k, m, vec) and dec.Init(k, m, vec)
    nseg = nb * k - nb // 2
    lay = norm_amd.object_layout((nseg - 1) * seg + seg - 1, seg, k)
    assert lay.num_blocks == nb
    sizes = norm_amd.object_block_sizes(lay, 0, nb)
    # the oracle's source, cut into an object: segment after segment, the last one a byte short
    source = orc.make_blocks(k, m, seg, nb, seg_stride=stride, num_data=sizes)
    source[nb - 1, int(sizes[nb - 1]) - 1, seg - 1:] = 0
    obj = np.concatenate([source[b, s, :seg] for b in range(nb) for s in range(int(sizes[b]))])[:lay.object_size]
    assert obj.size == lay.object_size
    # the loss, taken out of the pending mask: up to m slots of a block, source and parity
    words = (k + m + 31) // 32
    pend = np.zeros((nb, words), np.uint32)
    lost = [(b * 5 + m) % (m + 1) for b in range(nb)]
    lost[1] = 0
    dropped = []
    for b in range(nb):
        n = int(sizes[b]) + m
        gone = set(int(x) for x in rng.choice(n, lost[b], replace=False))
        if b == nb - 1:
            gone = set(list(gone)[:max(0, lost[b] - 1)]) | {int(sizes[b]) - 1}  # the short last segment among them
        dropped.append(gone)
        for s in range(n):
            if s not in gone:
                pend[b, s // 32] |= np.uint32(1 << (s % 32))
    assert max(len(g) for g in dropped) == m and not dropped[1]
    gap, fec_id, fec_m, first = 13, 5, 8, 0xFFFFFD
    count = int(sizes.sum()) + nb * m - sum(len(g) for g in dropped)
    dobj = torch.from_numpy(obj).cuda()
    dev = torch.zeros((nb, k + m, stride), dtype=torch.uint8, device="cuda")
    dnd = torch.zeros(nb, dtype=torch.int16, device="cuda")
    dlens = torch.zeros((nb, k), dtype=torch.int16, device="cuda")
    dpend = _dev(pend)
    wire = torch.from_numpy(rng.integers(1, 256, count * (gap + vec) + 40, dtype=np.uint8)).cuda()
    dev2 = _filled(nb, k, m, stride)
    mask = norm_amd.received_mask(nb, k, m)
    rstats = torch.zeros(3, dtype=torch.int32, device="cuda")
    dout = torch.full((lay.object_size,), FILL, dtype=torch.uint8, device="cuda")
    # sender
    enc.read_object(dobj, lay, dev, num_data=dnd, seg_length=dlens)
    enc.encode_blocks(dev, num_data=dnd)
    off, blk, sym, ln, start = enc.list_pending(dpend, num_data=dnd, seg_length=dlens, gap=gap)
    enc.emit_segments(dev, wire, off, blk, sym, ln, count_dev=start[nb, :1], fec_id=fec_id, fec_m=fec_m,
                      first_block_id=first, num_data=dnd)
    # receiver: nothing but the wire buffer and the list's offsets, lengths and total
    dec.ingest_messages(dev2, mask, wire, off, ln, fec_id, fec_m, first_block_id=first, count_dev=start[nb, :1],
                        num_data=dnd, stats=rstats)
    st = dec.decode_received(dev2, mask, num_data=dnd)
    dec.write_object(dout, lay, dev2, received=mask, status=st)
    torch.cuda.synchronize()
    assert int(_np(start, np.uint64)[nb, 0]) == count
    assert rstats.cpu().tolist() == [count, 0, 0]
    want_st = [len(g) if any(s < sizes[b] for s in g) else 0 for b, g in enumerate(dropped)]
    assert st.cpu().tolist() == want_st and any(want_st)
    assert np.array_equal(dout.cpu().numpy(), obj)
    got = dev2.cpu().numpy()
    for b in range(nb):
        n = int(sizes[b])
        assert np.array_equal(got[b, :n, :seg], source[b, :n, :seg]), b


@pytest.mark.parametrize("last_len", [1400, 7, 0])
def test_wire_buffer_that_ends_its_allocation(last_len):
    """The last message's payload ends on the last byte of a tensor of exactly 2 MiB, and
    payload_bytes is the tensor's size.  Every load of the intake is an aligned chunk of at most 16
    bytes that holds a byte of the message, so none of them leaves the tensor's last page; the test
    holds the result at that boundary (the rule itself is a property of the kernel's code)."""
    k, m, vec, stride, nb = 64, 32, 1400, 1400, 3
    fec_id, fec_m, idlen, first = 129, 8, 8, 0xFFFFFFFE
    P = 2 << 20
    rng = np.random.default_rng(last_len)
    dec = _decoder(NFEC_MDP, k, m, vec)
    src = rng.integers(1, 256, (nb, k + m, stride), dtype=np.uint8)
    nd = np.full(nb, k, np.uint16)
    # the last message, and in front of it messages whose IDs and payloads cross the last chunks
    entries = [(P - last_len, 2, 95, last_len)]
    pos = P - last_len - idlen
    for i, ln in enumerate((1, 15, 16, 17, 1400, 33)):
        off = pos - ln - (i % 2) * 3
        entries.append((off, i % nb, 10 + i, ln))
        pos = off - idlen
    wire = np.zeros(P, np.uint8)
    wire[pos - 64:] = rng.integers(1, 256, P - pos + 64, dtype=np.uint8)
    _emit(wire, src, entries, fec_id, fec_m, first, nd)
    dwire = torch.from_numpy(wire).cuda()
    assert dwire.numel() == P and P % (2 << 20) == 0
    dev = _filled(nb, k, m, stride)
    mask = norm_amd.received_mask(nb, k, m)
    stats = torch.zeros(3, dtype=torch.int32, device="cuda")
    dec.ingest_messages(dev, mask, dwire, _dev(np.array([e[0] for e in entries], np.uint64)),
                        _dev(np.array([e[3] for e in entries], np.uint16)), fec_id, fec_m, first_block_id=first,
                        stats=stats)
    torch.cuda.synchronize()
    assert stats.cpu().tolist() == [len(entries), 0, 0]
    want = np.full(src.shape, FILL, np.uint8)
    for _, b, s, ln in entries:
        want[b, s, :ln] = src[b, s, :ln]
        want[b, s, ln:vec] = 0
    assert np.array_equal(dev.cpu().numpy(), want)
