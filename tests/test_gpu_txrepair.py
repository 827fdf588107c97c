"""Sender repair state on the device: nfec_tx_handle_nacks, nfec_tx_activate_repairs and
nfec_tx_end_blocks (norm_amd/csrc/kernels_txrepair.hip) against the host entries on the same bytes
(nfec_tx_*_host, themselves held to a serial walk of the reference's rule in
tests/test_txrepair_host.py): all four state arrays, the totals, an untouched pending mask and the
sentinels around the state arrays.  Then the full circle on the device: a sender and three receivers,
loss, repair requests, NACK handling by NORM's repair economy, until nothing is asked for.  (No
kernel scans over messages or blocks, so there is no scan tile to straddle.)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import norm_amd  # noqa: E402
from norm_amd import _native as N  # noqa: E402
from norm_amd import NormDecoderRS8, NormEncoderRS8, NormEncoderRS16  # noqa: E402
from test_gpu_tx import _dev as _dev_words, _np  # noqa: E402
from test_txrepair_host import (ITEMS, OBJ, SEGMENT, Case, Sender, block_range, corner_cases, order_pair, request,  # noqa: E402
                                same_state, seg_items, seg_range)



def _dev(a):
    """a NumPy unsigned array as the torch tensor of the same bits, on the GPU"""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.copy()).cuda() if a.dtype == np.uint8 else _dev_words(a)


GUARD = 64  # sentinel elements on either side of every state array
_CODECS = {}


def codec(k, m):
    if (k, m) not in _CODECS:
        enc = NormEncoderRS8() if k + m <= 255 else NormEncoderRS16()
        assert enc.Init(k, m, 64)
        _CODECS[(k, m)] = enc
    return _CODECS[(k, m)]


class Guarded:
    """a host state on the device, every array between sentinels"""

    def __init__(self, host):
        self.full, views = [], []
        for a, signed in zip(host.arrays(), (np.int32, np.int16, np.int32, np.int32)):
            flat = np.ascontiguousarray(a).view(signed).reshape(-1)
            t = torch.full((flat.size + 2 * GUARD,), 0x5A5A, dtype=torch.from_numpy(flat[:0]).dtype, device="cuda")
            t[GUARD:GUARD + flat.size] = torch.from_numpy(flat.copy()).cuda()
            self.full.append(t)
            views.append(t[GUARD:GUARD + flat.size].view(a.shape))
        self.state = norm_amd.TxRepairState(*views)

    def check(self, want):
        same_state(self.state.to_host(), want)
        for t in self.full:
            assert (t[:GUARD] == 0x5A5A).all() and (t[-GUARD:] == 0x5A5A).all()


def device_handle(case, before, unit_capacity=None, stream=None, wire=None, offsets=None):
    """the device entry on a copy of `before` (host state): (guarded state, totals)"""
    g = Guarded(before)
    wire = _dev(case.wire) if wire is None else wire
    if case.payload_bytes is not None:
        wire = wire[:case.payload_bytes]
    offsets = _dev(case.offsets) if offsets is None else offsets
    count_dev = None if case.count is None else _dev(np.array([case.count], np.uint64))
    totals = codec(case.k, case.m).handle_nacks(g.state, wire, offsets, _dev(case.lengths), _dev(np.array(case.nds, np.uint16)),
                                                case.fec[0], case.fec[1], OBJ, case.first, case.extra, unit_capacity,
                                                count_dev=count_dev, stream=stream)
    (stream.synchronize() if stream is not None else torch.cuda.synchronize())
    return g, _np(totals, np.uint64)


def compare(case, unit_capacity=None, stream=None):
    """handle, then activate and end_blocks on what it left: device against host"""
    before = case.sender().state(case.stride)
    pending0 = case.sender().pending(case.stride)
    h_state, h_totals = case.host(unit_capacity, before.clone())
    g, totals = device_handle(case, before, unit_capacity, stream)
    assert np.array_equal(totals, h_totals), (case.name, totals, h_totals)
    g.check(h_state)
    nds = np.array(case.nds, np.uint16)
    enc, d_pending = codec(case.k, case.m), _dev(pending0)
    t = enc.activate_repairs(g.state, d_pending, _dev(nds), case.auto, stream=stream)
    h_pending = pending0.copy()
    h_t = norm_amd.tx_activate_repairs_host(case.k, case.m, h_state, h_pending, nds, case.auto)
    torch.cuda.synchronize()
    assert np.array_equal(_np(t, np.uint64), h_t), (case.name, _np(t, np.uint64), h_t)
    assert np.array_equal(_np(d_pending, np.uint32), h_pending)
    g.check(h_state)
    d_pending.zero_()
    h_pending[:] = 0
    enc.end_blocks(g.state, d_pending, _dev(nds), stream=stream)
    norm_amd.tx_end_blocks_host(case.k, case.m, h_state, h_pending, nds)
    torch.cuda.synchronize()
    g.check(h_state)
    return h_totals


@pytest.mark.parametrize("case", corner_cases(), ids=lambda c: c.name)
def test_corner_contents(case):
    compare(case)


@pytest.mark.parametrize("units", [65, 129])
def test_a_request_of_more_than_64_units(units):
    """the wave's unit loop: one ITEMS request whose units alternate between two blocks and, in its
    second half, stay on one (E runs over the round's edge), with a foreign fec_id near its end"""
    k, m = 64, 32
    items = [(u % 2, 64 + u % 32) for u in range(units // 2)] + [(2, 64 + u % 32) for u in range(units - units // 2)]
    body = request(ITEMS, SEGMENT, items)
    totals = compare(Case(k, m, [k] * 3, [body, body + seg_range(2, 0, 3)], extra=1, name=f"{units} units"))
    assert totals[0] == 2 * units + 1
    bad = bytearray(body)
    bad[4 + 8 * (units - 2)] = 2  # the walk stops inside the second (or third) round
    totals = compare(Case(k, m, [k] * 3, [bytes(bad), seg_items(2, 70)], name=f"{units} units, cut"))
    assert totals[0] == units - 2 + 1 and totals[4] == 1


@pytest.mark.parametrize("messages", [70, 130])
@pytest.mark.parametrize("where", ["first", "last"])
def test_many_messages_for_one_block(messages, where):
    """the per-block ordering past one wave: every message asks for block 1, and the "order decides"
    pair stands first and last (A ... B) or last and first (B ... A) among them"""
    k, m = 8, 4
    a, b = seg_range(1, 8, 12), seg_range(1, 8, 10)
    rng = np.random.default_rng(messages)
    filler = [seg_items(1, int(s)) + seg_items(0, 8) for s in rng.integers(9, 12, messages - 2)]
    msgs = ([a] + filler + [b]) if where == "first" else ([b] + filler + [a])
    totals = compare(Case(k, m, [k] * 2, msgs, parity_offset=1, name=f"{messages} {where}"))
    assert totals[1] == 2 * messages - 2
    # and with a BLOCK-level unit in the middle: the units behind it open stretches and are dropped
    msgs[messages // 2] = block_range(1, 1) + msgs[messages // 2]
    totals = compare(Case(k, m, [k] * 2, msgs, parity_offset=1, name=f"{messages} {where} block"))
    assert totals[3] == 1 and totals[2] == messages - messages // 2


def test_five_thousand_messages_over_300_blocks():
    k, m, nb = 64, 32, 300
    rng = np.random.default_rng(5000)
    msgs = []
    for _ in range(5000):
        b, lo = int(rng.integers(0, nb)), int(rng.integers(0, k + m))
        hi = min(k + m - 1, lo + int(rng.integers(0, 6)))
        msgs.append(block_range(b, b) if rng.random() < 0.01 else seg_items(b, lo) if lo == hi else seg_range(b, lo, hi))
    totals = compare(Case(k, m, [k] * nb, msgs, gap=3, align=1, name="5000"))
    assert totals[0] == 5000 and totals[1] > 4000


def test_wire_buffer_that_ends_its_allocation():
    """The last message ends on the last byte of a tensor of exactly 2 MiB and starts at an odd
    offset; payload_bytes is the tensor's size.  Every load is an aligned chunk of at most 16 bytes
    that holds a byte of a message, so none leaves the tensor's last page (the rule itself is a
    property of the kernel's code; the test holds the result at that boundary)."""
    size = 2 << 20
    tail = seg_items(0, 8) + seg_range(1, 8, 10) + seg_items(1, 11) + b"\x01"  # (cut short: one byte of a header)
    assert len(tail) % 2 == 1
    case = Case(8, 4, [8, 8], [seg_items(1, 9), tail], name="end of allocation")
    wire = np.zeros(size, np.uint8)
    wire[:len(case.messages[0])] = np.frombuffer(case.messages[0], np.uint8)
    wire[size - len(tail):] = np.frombuffer(tail, np.uint8)
    case.wire, case.offsets = wire, np.array([0, size - len(tail)], np.uint64)
    assert int(case.offsets[1]) % 2 == 1
    dwire = torch.empty(size, dtype=torch.uint8, device="cuda")
    dwire.copy_(torch.from_numpy(wire))
    before = case.sender().state()
    h_state, h_totals = case.host(None, before.clone())
    g, totals = device_handle(case, before, wire=dwire)
    assert np.array_equal(totals, h_totals) and totals[4] == 1 and totals[1] == 4
    g.check(h_state)


def test_capacity_overflow_changes_nothing():
    case = corner_cases()[2]
    units = int(case.expected()[1][0])
    assert units >= 2
    before = case.sender().state()
    before.repair[:] = 0x0A0A
    before.parity[:] = 1
    g, totals = device_handle(case, before, unit_capacity=units - 1)
    g.check(before)
    assert totals.tolist()[:4] == [units, 0, 0, 0]
    compare(case, unit_capacity=units - 1)
    compare(case, unit_capacity=units)
    big = Case(64, 32, [64] * 40, [seg_items(b % 40, 64 + b % 7) for b in range(900)], name="overflow, many waves")
    compare(big, unit_capacity=899)
    compare(big, unit_capacity=900)


def test_a_non_default_stream():
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        compare(corner_cases()[3], stream=s)
        compare(order_pair("BA"), stream=s)


def test_argument_checks():
    enc = codec(8, 4)
    state = norm_amd.tx_repair_state(2, 8, 4, device="cuda")
    wire = _dev(np.frombuffer(seg_items(0, 8), np.uint8))
    off, ln = _dev(np.zeros(1, np.uint64)), _dev(np.array([12], np.uint16))

    def handle(**kw):
        try:
            enc.handle_nacks(state, wire, off, ln, **kw)
        except norm_amd.NfecError as e:
            return e.code
        return 0

    assert handle() == 0
    assert handle(fec_id=0) == N.NFEC_EINVAL and handle(fec_id=2, fec_m=12) == N.NFEC_EINVAL
    assert handle(extra_parity=65536) == N.NFEC_EINVAL
    assert handle(workspace=torch.zeros(64, dtype=torch.uint8, device="cuda")) == N.NFEC_EINVAL  # below the query's size
    need = N.lib().nfec_tx_nack_workspace_bytes(4, 1, 2)
    assert handle(unit_capacity=4, workspace=torch.zeros(need + 16, dtype=torch.uint8, device="cuda")[1:]) == N.NFEC_EINVAL
    assert handle(unit_capacity=4, workspace=torch.zeros(need, dtype=torch.uint8, device="cuda")) == 0
    narrow = norm_amd.tx_repair_state(2, 40, 30, device="cuda", mask_stride=1)
    with pytest.raises(norm_amd.NfecError):
        codec(40, 30).handle_nacks(narrow, wire, off, ln)
    with pytest.raises(norm_amd.NfecError):
        enc.activate_repairs(state, torch.zeros((2, 1), dtype=torch.int32, device="cuda"), auto_parity=5)
    st = state.struct()
    st.parity = None
    assert N.lib().nfec_tx_end_blocks(enc._h, None, 2, off.data_ptr(), 1, st, None) == N.NFEC_EINVAL
    # nothing to do: zero totals
    empty = norm_amd.tx_repair_state(0, 8, 4, device="cuda")
    assert _np(enc.handle_nacks(empty, wire, off, ln), np.uint64).tolist() == [0] * 6
    assert _np(enc.handle_nacks(state, wire, off[:0], ln[:0]), np.uint64).tolist() == [0] * 6
    torch.cuda.synchronize()


def split_messages(content, item_len, limit=1400):
    """the request headers of repair-request content -> (offsets, lengths) of messages of at most
    `limit` bytes that end at request boundaries"""
    off, ln, at, start = [], [], 0, 0
    while at < len(content):
        size = 4 + (int(content[at + 2]) << 8 | int(content[at + 3]))
        if at + size - start > limit:
            off.append(start), ln.append(at - start)
            start = at
        at += size
    if at > start:
        off.append(start), ln.append(at - start)
    return off, ln


def test_sender_and_three_receivers_until_nothing_is_asked_for():
    """encode -> (list -> emit -> end_blocks -> per-receiver loss -> ingest -> decode -> repair requests
    -> handle_nacks -> activate_repairs) ... until no receiver asks.  Every round loses 45 % of its
    messages independently per receiver, receiver 0 in round 1 also every message of 7 blocks.  Every
    round's state is the host entries' on the same bytes.  A mask-level simulation of this loop took
    12-13 rounds; the bound is 40."""
    k, m, vec, nb, R = 64, 32, 1400, 300, 3
    fec_id, fec_m, first, idlen, item_len = 5, 8, 0xFFFF00, 4, 8
    max_units = (1400 - 4) // (2 * item_len)  # a request fits a message
    rng = np.random.default_rng(300)
    enc = NormEncoderRS8()
    decs = [NormDecoderRS8() for _ in range(R)]
    assert enc.Init(k, m, vec) and all(d.Init(k, m, vec) for d in decs)
    src = torch.from_numpy(rng.integers(0, 256, (nb, k + m, vec), dtype=np.uint8)).cuda()
    enc.encode_blocks(src)
    rxb = [torch.zeros_like(src) for _ in range(R)]
    masks = [norm_amd.received_mask(nb, k, m) for _ in range(R)]
    state = norm_amd.tx_repair_state(nb, k, m, 0, device="cuda")
    h_state = norm_amd.tx_repair_state(nb, k, m, 0)
    words = (k + m + 31) // 32
    h_pending = Sender(k, m, [k] * nb).pending()  # TxInit: the sources
    pending = _dev(h_pending)
    gone = [int(b) for b in rng.choice(nb, 7, replace=False)]
    rounds, emitted, union_total, fresh_rounds = 0, 0, 0, 0
    while True:
        rounds += 1
        assert rounds <= 40
        off, blk, sym, ln, start = enc.list_pending(pending, gap=idlen)
        count, nbytes = (int(x) for x in _np(start, np.uint64)[nb])
        emitted += count
        wire = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        enc.emit_segments(src, wire, off, blk, sym, ln, count_dev=start[nb, :1], fec_id=fec_id, fec_m=fec_m,
                          first_block_id=first, pending=pending)
        enc.end_blocks(state, pending)
        torch.cuda.synchronize()
        assert not _np(pending, np.uint32).any()
        h_pending[:] = 0
        norm_amd.tx_end_blocks_host(k, m, h_state, h_pending)
        h_off, h_blk, h_ln = _np(off, np.uint64)[:count], _np(blk, np.uint32)[:count], _np(ln, np.uint16)[:count]
        contents = []
        for r in range(R):
            keep = rng.random(count) >= 0.45
            if rounds == 1 and r == 0:
                keep &= ~np.isin(h_blk, gone)
            decs[r].ingest_messages(rxb[r], masks[r], wire, _dev(h_off[keep]), _dev(h_ln[keep]), fec_id, fec_m,
                                    first_block_id=first)
            decs[r].decode_received(rxb[r], masks[r])
            content, _, totals = decs[r].repair_requests(masks[r], fec_id=fec_id, fec_m=fec_m, object_id=7,
                                                         first_block_id=first, max_units=max_units)
            contents.append(content.cpu().numpy()[:int(_np(totals, np.uint64)[0])])
        if not any(len(c) for c in contents):
            break
        # the NACKs of the round: every receiver's content split at request boundaries, in one wire buffer
        nack_wire = np.concatenate(contents)
        n_off, n_len, base = [], [], 0
        named = np.zeros((nb, k + m), bool)  # the union of all named slots
        for c in contents:
            o, ll = split_messages(c, item_len)
            assert all(x <= 1400 for x in ll)
            n_off += [base + x for x in o]
            n_len += ll
            base += len(c)
            fl, _, lo, hi, consumed = norm_amd.repair_parse_host(fec_id, fec_m, c)
            assert consumed == len(c)
            for i in range(len(fl)):
                b0, b1 = (int(lo[i, 1]) - first) & 0xFFFFFF, (int(hi[i, 1]) - first) & 0xFFFFFF
                if fl[i] & 2:
                    named[b0:b1 + 1, :k] = True
                else:
                    named[b0, int(lo[i, 3]):int(hi[i, 3]) + 1] = True
        union_total += int(named.sum())
        n_off, n_len = np.array(n_off, np.uint64), np.array(n_len, np.uint16)
        t = enc.handle_nacks(state, _dev(nack_wire), _dev(n_off), _dev(n_len), fec_id=fec_id, fec_m=fec_m, object_id=7,
                             first_block_id=first)
        a = enc.activate_repairs(state, pending)
        h_t = norm_amd.tx_handle_nacks_host(k, m, h_state, nack_wire, n_off, n_len, None, fec_id, fec_m, 7, first)
        h_a = norm_amd.tx_activate_repairs_host(k, m, h_state, h_pending)
        torch.cuda.synchronize()
        assert np.array_equal(_np(t, np.uint64), h_t) and np.array_equal(_np(a, np.uint64), h_a), (rounds, t, h_t, a, h_a)
        assert h_t[4] == 0 and h_t[5] == 0 and h_t[0] <= nack_wire.size // 8 + 1
        same_state(state.to_host(), h_state)
        got_pending = _np(pending, np.uint32)
        assert np.array_equal(got_pending, h_pending)
        bits = np.unpackbits(got_pending.view(np.uint8), axis=1, bitorder="little")[:, :k + m].astype(bool)
        fresh_rounds += bool((bits[:, k + 1:] & ~named[:, k + 1:]).any())  # parity at or past nd + 1 that nobody named
    print(f"rounds {rounds}, emitted {emitted} for {nb * k} sources, named {union_total}, rounds with fresh parity {fresh_rounds}")
    assert rounds >= 3 and fresh_rounds >= 1
    for r in range(R):
        assert torch.equal(rxb[r][:, :k], src[:, :k])  # every source byte is the original
    # fewer messages than the first transmission plus a retransmission of everything that was named
    assert emitted < nb * k + union_total, (emitted, union_total)
