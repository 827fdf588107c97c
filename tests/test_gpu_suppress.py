"""NACK suppression and repair advertisements on the device: nfec_rx_handle_repair_content,
nfec_rx_repair_pending (norm_amd/csrc/kernels_suppress.hip) and nfec_tx_repair_adv (the generalised
kernels of norm_amd/csrc/kernels_nack.hip) against their host entries on the same bytes (themselves
held to serial walks of the reference's rule in tests/test_suppress_host.py): every state and output
array between sentinels, the read-only arrays compared before and after.  Then the identities on the
device, and the full circle in HBM: tests/test_suppress_host.py's cycle model, with payloads."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import norm_amd  # noqa: E402
from norm_amd import _native as N  # noqa: E402
from norm_amd import NormDecoderRS8, NormEncoderRS8  # noqa: E402
from test_gpu_tx import _np  # noqa: E402
from test_gpu_txrepair import _dev, codec  # noqa: E402
from test_nack_host import to_words  # noqa: E402
from test_suppress_host import (CYCLE, CYCLE_OBSERVED, RX_INFO, RX_OBJECT, TX_INFO, TX_OBJECT, RxCase, cycle_model,  # noqa: E402
                                cycle_summary, random_content, random_reception, same_rx_state, tx_state, words_of)
from test_txrepair_host import (BITS, ITEMS, OBJ, SEGMENT, Case, block_range, damaged_case, request, same_state, seg_items,  # noqa: E402
                                seg_range)

GUARD = 64  # sentinel elements on either side of every guarded array
SIGNED = {np.dtype(np.uint8): np.uint8, np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}


class Guard:
    """a host array on the device between sentinels"""

    def __init__(self, a):
        a = np.ascontiguousarray(a)
        flat = a.view(SIGNED[a.dtype]).reshape(-1)
        self.dtype, self.shape = a.dtype, a.shape
        self.full = torch.full((flat.size + 2 * GUARD,), 0x5A, dtype=torch.from_numpy(flat[:0]).dtype, device="cuda")
        self.full[GUARD:GUARD + flat.size] = torch.from_numpy(flat.copy()).cuda()
        self.t = self.full[GUARD:GUARD + flat.size].view(a.shape)

    def host(self):
        assert (self.full[:GUARD] == 0x5A).all() and (self.full[-GUARD:] == 0x5A).all()
        return self.t.cpu().numpy().view(self.dtype).reshape(self.shape)


class GuardedRx:
    def __init__(self, host):
        self.guards = [Guard(a) for a in host.arrays()]
        self.state = norm_amd.RxRepairState(*(g.t for g in self.guards))

    def host(self):
        return norm_amd.RxRepairState(*(g.host() for g in self.guards))


def fec_for(k, m):
    return (5, 8) if k + m <= 256 else (2, 16)


def device_handle(rc, before=None, stream=None, wire=None):
    """the device entry on a copy of `before`: (guarded state, totals uint64 [6])"""
    c = rc.case
    before = norm_amd.rx_repair_state(len(c.nds), c.k, c.m, mask_stride=rc.stride) if before is None else before
    g, received, totals = GuardedRx(before), _dev(rc.words), Guard(np.full(6, 77, np.uint64))
    wire = _dev(c.wire) if wire is None else wire
    if c.payload_bytes is not None:
        wire = wire[:c.payload_bytes]
    count_dev = None if c.count is None else _dev(np.array([c.count], np.uint64))
    codec(c.k, c.m).handle_repair_content(g.state, received, wire, _dev(c.offsets), _dev(c.lengths),
                                          _dev(np.array(c.nds, np.uint16)), c.fec[0], c.fec[1], OBJ, c.first,
                                          count_dev=count_dev, totals=totals.t, stream=stream)
    (stream.synchronize() if stream is not None else torch.cuda.synchronize())
    assert np.array_equal(_np(received, np.uint32), rc.words)
    return g, totals.host()


def compare_handle(rc, before=None, stream=None):
    h_state, h_totals = rc.host(None if before is None else before.clone())
    g, totals = device_handle(rc, before, stream)
    assert np.array_equal(totals, h_totals), (rc.case.name, totals, h_totals)
    same_rx_state(g.host(), h_state)
    return h_state, h_totals


def compare_pending(k, m, words, nds, state, flags=0, stream=None):
    """device against host on (reception words, suppression state): totals and pending_blocks, which
    the device gets full of sentinel bits"""
    nb = words.shape[0]
    nd = None if nds is None else np.array(nds, np.uint16)
    h_totals, h_words = norm_amd.rx_repair_pending_host(k, m, state, words, nd, flags)
    g, received = GuardedRx(state), _dev(words)
    totals, out = Guard(np.full(4, 77, np.uint64)), Guard(np.full(max(1, (nb + 31) // 32), 0x5A5A5A5A, np.uint32))
    codec(k, m).repair_pending(g.state, received, None if nd is None else _dev(nd), flags, out.t, totals.t, stream=stream)
    (stream.synchronize() if stream is not None else torch.cuda.synchronize())
    assert np.array_equal(totals.host(), h_totals), (totals.host(), h_totals)
    assert np.array_equal(out.host(), h_words)
    same_rx_state(g.host(), state)  # only read
    assert np.array_equal(_np(received, np.uint32), words)
    return h_totals, h_words


def compare_adv(k, m, nds, st, fec=(5, 8), first=0, max_units=None, capacity=None, stream=None):
    nb = len(nds)
    nd = np.array(nds, np.uint16)
    h_content, h_start, h_totals = norm_amd.tx_repair_adv_host(k, m, st, nd, fec[0], fec[1], OBJ, first, max_units, capacity)
    guards = [Guard(a) for a in st.arrays()]
    d_state = norm_amd.TxRepairState(*(g.t for g in guards))
    content = Guard(np.zeros(h_content.size + (-h_content.size) % 4, np.uint8))
    _, start, totals = codec(k, m).repair_adv(d_state, _dev(nd), fec[0], fec[1], OBJ, first, max_units, h_content.size,
                                              content.t, stream=stream)
    (stream.synchronize() if stream is not None else torch.cuda.synchronize())
    assert np.array_equal(_np(totals, np.uint64), h_totals), (_np(totals, np.uint64), h_totals)
    assert np.array_equal(_np(start, np.uint64), h_start)
    assert np.array_equal(content.host()[:h_content.size], h_content) and not content.host()[h_content.size:].any()
    for g, a in zip(guards, st.arrays()):
        assert np.array_equal(g.host(), a)  # only read
    assert nb == 0 or h_totals[0] > 0
    return h_content, h_totals


# ---- device against host: the shapes ----

SHAPES = [(8, 4, 1), (8, 4, 33), (64, 32, 33), (2100, 60, 3), (8, 4, 8300)]


def reception(rng, k, m, nb, loss=0.45):
    got, nds = random_reception(rng, nb, k, m, loss)
    if nb == 1:
        got[0], nds = False, [k]
        got[0, :k - 2] = True  # needing: e = 2 > p = 0
    return got, nds


@pytest.mark.parametrize("k,m,nb", SHAPES, ids=lambda v: str(v))
def test_handle_shapes(k, m, nb):
    """random content of every level, own and foreign, partly damaged, at odd offsets; 9,000 messages
    for the largest batch (past 2,048 workgroups of four waves: the waves stride, the counters go
    through LDS once per workgroup)"""
    rng = np.random.default_rng(k + nb)
    fec = fec_for(k, m)
    first = (1 << BITS[fec]) - 3
    got, nds = reception(rng, k, m, nb)
    msgs = random_content(rng, nb, k, m, fec, first, 9000 if nb > 8000 else 60)
    if nb > 8000:
        msgs[17] = block_range(5, nb + 40, fec=fec, first=first) + msgs[17]
    rc = RxCase(Case(k, m, nds, msgs, fec=fec, first=first, align=1, gap=3, name="shapes"), got,
                stride=(k + m + 31) // 32 + (nb % 2), rng=rng)
    _, totals = compare_handle(rc)
    assert totals[1] > 0 and totals[0] > len(msgs)


@pytest.mark.parametrize("k,m,nb", SHAPES + [(8, 4, 262144 + 70)], ids=lambda v: str(v))
def test_pending_shapes(k, m, nb):
    """random suppression states over random receptions; 8,300 blocks have pending_blocks words whose
    blocks lie in different workgroups' reach, 262,214 blocks (8,195 words) are past 2,048 workgroups
    of four waves, one word a wave"""
    rng = np.random.default_rng(k * 3 + nb)
    stride = (k + m + 31) // 32 + (nb % 2)
    if nb > 100000:  # (straight from random words: the bool detour costs seconds)
        nds = None
        words = (rng.integers(0, 1 << 12, (nb, stride), dtype=np.uint32) & rng.integers(0, 1 << 12, (nb, stride), dtype=np.uint32))
        words[rng.random(nb) < 0.2] = 0
        rep = rng.integers(0, 1 << 32, (nb, stride), dtype=np.uint32)
        rep[rng.random(nb) < 0.3] = 0xFFFFFFFF
    else:
        got, nds = reception(rng, k, m, nb)
        words = to_words(got, nds, m, stride, rng)
        asked = rng.random((nb, k + m)) < 0.5
        asked[rng.random(nb) < 0.3] = True
        rep = to_words(asked, nds, m, stride, rng)
    for trial, word in enumerate((0, RX_INFO, RX_OBJECT)):
        st = norm_amd.rx_repair_state(nb, k, m, mask_stride=stride)
        st.repair[:] = rep
        st.block_repair[:] = words_of([b for b in np.flatnonzero(rng.random(nb) < 0.3)], nb) if nb < 100000 else rng.integers(
            0, 1 << 32, st.block_repair.shape, dtype=np.uint32) & rng.integers(0, 1 << 32, st.block_repair.shape, dtype=np.uint32)
        st.object[0] = word
        totals, _ = compare_pending(k, m, words, nds, st, flags=trial % 2 if nb > 1 else 1)
        if nb >= 33:
            assert totals[1] > 0 and totals[2] > 0
        if nb > 100000:
            break


@pytest.mark.parametrize("k,m,nb", SHAPES, ids=lambda v: str(v))
def test_adv_shapes(k, m, nb):
    rng = np.random.default_rng(k * 5 + nb)
    fec = fec_for(k, m)
    first = (1 << BITS[fec]) - 3
    nds = [k if rng.random() < 0.5 else k - 1 for _ in range(nb)]
    if nb > 2:
        nds[nb // 2] = 0
    repair = rng.random((nb, k + m)) < 0.3
    repair[rng.random(nb) < 0.4] = False
    repair[0, 3] = True
    bits = [int(b) for b in np.flatnonzero(rng.random(nb) < 0.4)]
    stride = (k + m + 31) // 32 + (nb % 2)
    for word, max_units in ((0, None), (TX_INFO, 1)):
        st = tx_state(k, m, nds, repair, bits, word, stride, rng)
        content, totals = compare_adv(k, m, nds, st, fec, first, max_units)
        if nb >= 33:
            assert totals[2] > 0 and totals[3] > 0
        if nb == 33 and word:
            for cap in (0, 5, len(content) // 2 + 1, len(content) - 3):  # capacities that cut a dword
                assert np.array_equal(compare_adv(k, m, nds, st, fec, first, max_units, capacity=cap)[1], totals)


def test_adv_of_a_whole_object():
    k, m, nds = 8, 4, [8, 7, 8]
    repair = np.zeros((3, 12), bool)
    repair[1, [2, 9]] = True
    for fec in ((5, 8), (129, 8)):
        content, totals = compare_adv(k, m, nds, tx_state(k, m, nds, repair, [2], TX_OBJECT | TX_INFO), fec, 9)
        L = 4 + N.lib().nfec_payload_id_length(fec[0])
        assert totals.tolist() == [4 + L, 1, 0, 0] and content[0] == N.REPAIR_ITEMS and content[1] == N.REPAIR_OBJECT
        compare_adv(k, m, nds, tx_state(k, m, nds, repair, [2], TX_OBJECT), fec, 9, capacity=5)
    content, totals = compare_adv(k, m, nds, tx_state(k, m, nds, np.zeros((3, 12), bool), [], TX_INFO))
    assert totals.tolist() == [12, 1, 0, 0] and content[1] == N.REPAIR_INFO  # the INFO-only request


# ---- device against host: the messages ----

def needing(nb, k, m):
    got = np.zeros((nb, k + m), bool)
    got[:, 0] = True
    return got


def test_damaged_unreadable_and_count_dev():
    _, totals = compare_handle(RxCase(damaged_case(), needing(3, 8, 4)))
    assert totals[4] == 5
    c = Case(8, 4, [8, 8], [seg_items(0, 8), seg_items(1, 8, 9), seg_items(0, 9)], name="unreadable")
    c.offsets = np.array([c.offsets[0], c.wire.size - 4, 1 << 40], np.uint64)
    _, totals = compare_handle(RxCase(c, needing(2, 8, 4)))
    assert totals[5] == 2 and totals[0] == 1
    c = Case(8, 4, [8, 8], [seg_items(0, 8), seg_items(1, 8, 9), seg_range(0, 0, 3)], name="count_dev below count")
    c.count = 2
    _, totals = compare_handle(RxCase(c, needing(2, 8, 4)))
    assert totals[0] == 3 and totals[1] == 3


def test_wire_buffer_that_ends_its_allocation():
    """the last message ends on the last byte of a tensor of exactly 2 MiB and starts at an odd offset"""
    size = 2 << 20
    tail = seg_items(0, 8) + seg_range(1, 8, 10) + block_range(0, 1) + b"\x01"  # (cut short: one byte of a header)
    assert len(tail) % 2 == 1
    case = Case(8, 4, [8, 8], [seg_items(1, 9), tail], name="end of allocation")
    wire = np.zeros(size, np.uint8)
    wire[:len(case.messages[0])] = np.frombuffer(case.messages[0], np.uint8)
    wire[size - len(tail):] = np.frombuffer(tail, np.uint8)
    case.wire, case.offsets = wire, np.array([0, size - len(tail)], np.uint64)
    rc = RxCase(case, needing(2, 8, 4))
    dwire = torch.empty(size, dtype=torch.uint8, device="cuda")
    dwire.copy_(torch.from_numpy(wire))
    h_state, h_totals = rc.host()
    g, totals = device_handle(rc, wire=dwire)
    assert np.array_equal(totals, h_totals) and totals[4] == 1 and totals[1] == 3 and totals[3] == 2
    same_rx_state(g.host(), h_state)


def test_many_messages_for_one_block_and_one_word():
    """130 messages that all name block 1's slots and the blocks of one block_repair word: the
    atomics meet on two words, and the newly-set count is still exact"""
    k, m, nb = 8, 4, 40
    rng = np.random.default_rng(130)
    msgs = [seg_items(1, int(rng.integers(0, 12))) + block_range(int(rng.integers(0, 8)), int(rng.integers(8, 31)))
            + seg_range(1, 2, int(rng.integers(2, 12))) for _ in range(130)]
    _, totals = compare_handle(RxCase(Case(k, m, [k] * nb, msgs, gap=1, name="130"), needing(nb, k, m)))
    assert totals[1] == 260 and 23 <= totals[3] <= 31


def test_a_block_range_over_200_blocks():
    k, m, nb = 8, 4, 300
    for lo, hi in ((37, 236), (32, 255), (0, 299), (63, 64), (5, 100000)):
        before = norm_amd.rx_repair_state(nb, k, m)
        before.block_repair[2] = 0x00F0F000  # some of them are set already
        h_state, totals = compare_handle(RxCase(Case(k, m, [k] * nb, [block_range(lo, hi)], name="range"), needing(nb, k, m)), before)
        bits = np.unpackbits(h_state.block_repair.view(np.uint8), bitorder="little")[:nb].astype(bool)
        want = np.zeros(nb, bool)
        want[lo:hi + 1] = True
        want[76:80], want[84:88] = True, True
        assert np.array_equal(bits, want)
        assert totals[3] == int(want.sum()) - 8  # the newly set ones


def test_a_request_of_more_than_64_units():
    """the wave's unit loop: units that alternate between two blocks, a silent one among them, and a
    foreign fec_id inside the second round"""
    k, m = 64, 32
    got = needing(3, k, m)
    got[1, :k] = True  # block 1 is complete: its units are not applied
    items = [(u % 3, 60 + u % 30) for u in range(150)]
    body = request(ITEMS, SEGMENT, items)
    _, totals = compare_handle(RxCase(Case(k, m, [k] * 3, [body, body], name="150 units"), got))
    assert totals[0] == 300 and totals[1] == 200 and totals[2] == 100
    bad = bytearray(body)
    bad[4 + 8 * 100] = 2
    _, totals = compare_handle(RxCase(Case(k, m, [k] * 3, [bytes(bad)], name="cut"), got))
    assert totals[0] == 100 and totals[4] == 1


# ---- the identities, which fail without the feature: the entries do not exist ----

def device_content(content, totals):
    return content[:int(totals[0])]


def device_overhear(k, m, mask, nds, contents, fec, first, flags=0, stream=None):
    """a receiver with reception mask `mask` (device) handles device `contents` and decides:
    (totals, pending words, state), all on the device"""
    enc = codec(k, m)
    state = enc.rx_repair_state(mask.shape[0], device="cuda")
    if contents:
        lens = [int(c.numel()) for c in contents]
        wire = torch.cat(contents)
        off = _dev(np.cumsum([0] + lens[:-1]).astype(np.uint64))
        enc.handle_repair_content(state, mask, wire, off, _dev(np.array(lens, np.uint16)), nds, fec[0], fec[1], OBJ, first,
                                  stream=stream)
    totals, words = enc.repair_pending(state, mask, nds, flags, stream=stream)
    return totals, words, state


@pytest.mark.parametrize("flags", [0, N.NFEC_NACK_INFO])
def test_self_suppression(flags):
    k, m, nb = 8, 4, 500
    rng = np.random.default_rng(3 + flags)
    fec, first = (5, 8), 0xFFFF00
    got, nds = random_reception(rng, nb, k, m, 0.45)
    mask, d_nds = _dev(to_words(got, nds, m)), _dev(np.array(nds, np.uint16))
    content, _, t = codec(k, m).repair_requests(mask, d_nds, fec[0], fec[1], OBJ, first, flags)
    t = _np(t, np.uint64)
    assert t[2] > 0 and t[3] > 0
    totals, words, _ = device_overhear(k, m, mask, d_nds, [device_content(content, t)], fec, first, flags)
    assert _np(totals, np.uint64).tolist() == [0, 0, int(t[2]), int(t[3])] and not _np(words, np.uint32).any()
    totals, words, _ = device_overhear(k, m, mask, d_nds, [], fec, first, flags)
    assert _np(totals, np.uint64).tolist() == [1, int(t[2] + t[3]), 0, 0]


@pytest.mark.parametrize("word", [0, TX_INFO, TX_OBJECT | TX_INFO])
def test_adv_round_trip(word):
    k, m, nb = 64, 32, 70
    rng = np.random.default_rng(word + 1)
    fec, first = (129, 8), 0xFFFFFFF0
    nds = [k if rng.random() < 0.5 else k - 1 for _ in range(nb)]
    repair = rng.random((nb, k + m)) < 0.3
    repair[rng.random(nb) < 0.3] = False
    for b in range(nb):
        repair[b, nds[b] + m:] = False
    bits = [int(b) for b in np.flatnonzero(rng.random(nb) < 0.3)]
    st = tx_state(k, m, nds, repair, bits, word)
    d_nds = _dev(np.array(nds, np.uint16))
    content, _, t = codec(k, m).repair_adv(st.to_device(), d_nds, fec[0], fec[1], OBJ, first)
    mask = _dev(to_words(needing(nb, k, m), nds, m))
    _, _, rx = device_overhear(k, m, mask, d_nds, [device_content(content, t)], fec, first)
    rx = rx.to_host()
    if word & TX_OBJECT:
        assert rx.object[0] == RX_OBJECT and not rx.repair.any() and not rx.block_repair.any()
        return
    want = st.repair.copy()
    want[bits] = 0  # a whole block's segment bits are not advertised
    assert rx.object[0] == (RX_INFO if word & TX_INFO else 0)
    assert np.array_equal(rx.block_repair, st.block_repair) and np.array_equal(rx.repair, want)


def test_chained_on_a_non_default_stream():
    """repair_adv -> handle_repair_content -> repair_pending on one stream without a synchronize: the
    advertisement's length goes from its totals to the message list on the device"""
    k, m, nb = 8, 4, 33
    rng = np.random.default_rng(33)
    nds = [k] * nb
    repair = np.ones((nb, k + m), bool)  # everything a needing block asks for is advertised ...
    repair[:, 1:5] = rng.random((nb, 4)) < 0.5  # (... but for the four pending slots no request names)
    bits = [3, 4, 5, 31, 32]
    st = tx_state(k, m, nds, repair, bits, TX_INFO)
    got = needing(nb, k, m)
    got[7, :] = False  # absent, and not advertised as a whole block: it stays pending
    words = to_words(got, nds, m)
    h_content, _, h_t = norm_amd.tx_repair_adv_host(k, m, st)
    h_rx = norm_amd.rx_repair_state(nb, k, m)
    norm_amd.rx_handle_repair_content_host(k, m, h_rx, words, h_content, [0], [int(h_t[0])])
    h_totals, h_words = norm_amd.rx_repair_pending_host(k, m, h_rx, words, flags=N.NFEC_NACK_INFO)
    enc = codec(k, m)
    d_st, mask, rx = st.to_device(), _dev(words), enc.rx_repair_state(nb, device="cuda")
    off = _dev(np.zeros(1, np.uint64))
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        content, _, t = enc.repair_adv(d_st, stream=s)
        length = t[:1].to(torch.int16)
        enc.handle_repair_content(rx, mask, content, off, length, stream=s)
        totals, out = enc.repair_pending(rx, mask, flags=N.NFEC_NACK_INFO, stream=s)
    s.synchronize()
    assert np.array_equal(_np(totals, np.uint64), h_totals) and np.array_equal(_np(out, np.uint32), h_words)
    same_rx_state(rx.to_host(), h_rx)
    assert h_totals.tolist()[:2] == [1, 1] and h_words[0] == 1 << 7


def test_argument_checks():
    enc = codec(8, 4)
    rx = enc.rx_repair_state(2, device="cuda")
    mask = norm_amd.received_mask(2, 8, 4)
    wire = _dev(np.frombuffer(seg_items(0, 8), np.uint8))
    off, ln = _dev(np.zeros(1, np.uint64)), _dev(np.array([12], np.uint16))

    def code(fn, *a, **kw):
        try:
            fn(*a, **kw)
        except norm_amd.NfecError as e:
            return e.code
        return 0

    assert code(enc.handle_repair_content, rx, mask, wire, off, ln) == 0
    assert code(enc.handle_repair_content, rx, mask, wire, off, ln, fec_id=0) == N.NFEC_EINVAL
    assert code(enc.repair_pending, rx, mask, flags=2) == N.NFEC_EINVAL
    tx = norm_amd.tx_repair_state(2, 8, 4, device="cuda")
    assert code(enc.repair_adv, tx) == 0
    assert code(enc.repair_adv, tx, max_units=0) == N.NFEC_EINVAL
    assert code(enc.repair_adv, tx, content=torch.zeros(65, dtype=torch.uint8, device="cuda")[1:]) == N.NFEC_EINVAL
    narrow = norm_amd.rx_repair_state(2, 40, 30, device="cuda", mask_stride=1)
    assert code(codec(40, 30).repair_pending, narrow, mask) == N.NFEC_EINVAL
    empty = enc.rx_repair_state(0, device="cuda")
    assert _np(enc.handle_repair_content(empty, mask[:0], wire, off, ln), np.uint64).tolist() == [0] * 6
    assert _np(enc.handle_repair_content(rx, mask, wire, off[:0], ln[:0]), np.uint64).tolist() == [0] * 6
    assert _np(enc.repair_pending(empty, mask[:0], flags=1)[0], np.uint64).tolist() == [0] * 4
    assert _np(enc.repair_adv(norm_amd.tx_repair_state(0, 8, 4, device="cuda"))[2], np.uint64).tolist() == [0] * 4
    torch.cuda.synchronize()


# ---- the full circle in HBM ----

def test_sender_and_three_receivers_with_suppression():
    """tests/test_suppress_host.py's cycle model, with payloads: emit -> ingest -> decode, then per
    receiver in the model's back-off order handle_repair_content -> repair_pending -> (repair_requests
    -> handle_nacks when it sends) with the sender's repair_adv behind the NACKs, then
    activate_repairs.  Every round's decisions, pending-block words, NACK bytes and the sender's
    state and pending masks are the model's; every receiver ends with the object."""
    k, m, nb, R = CYCLE["k"], CYCLE["m"], CYCLE["nb"], CYCLE["receivers"]
    fec, first, obj, vec, idlen = CYCLE["fec"], CYCLE["first"], CYCLE["object_id"], 64, 4
    model = cycle_model(**CYCLE)
    assert cycle_summary(model) == CYCLE_OBSERVED
    rng = np.random.default_rng(1)
    enc = NormEncoderRS8()
    decs = [NormDecoderRS8() for _ in range(R)]
    assert enc.Init(k, m, vec) and all(d.Init(k, m, vec) for d in decs)
    src = torch.from_numpy(rng.integers(0, 256, (nb, k + m, vec), dtype=np.uint8)).cuda()
    enc.encode_blocks(src)
    rxb = [torch.zeros_like(src) for _ in range(R)]
    masks = [norm_amd.received_mask(nb, k, m) for _ in range(R)]
    state = norm_amd.tx_repair_state(nb, k, m, 0, device="cuda")
    pending = _dev(model[0]["pending"])
    nacks = 0
    for rec in model:
        assert np.array_equal(_np(pending, np.uint32), rec["pending"])
        off, blk, sym, ln, start = enc.list_pending(pending, gap=idlen)
        count, nbytes = (int(x) for x in _np(start, np.uint64)[nb])
        assert count == len(rec["keep"][0])
        wire = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        enc.emit_segments(src, wire, off, blk, sym, ln, count_dev=start[nb, :1], fec_id=fec[0], fec_m=fec[1],
                          first_block_id=first, pending=pending)
        enc.end_blocks(state, pending)
        h_off, h_ln = _np(off, np.uint64)[:count], _np(ln, np.uint16)[:count]
        for r in range(R):
            keep = rec["keep"][r]
            decs[r].ingest_messages(rxb[r], masks[r], wire, _dev(h_off[keep]), _dev(h_ln[keep]), fec[0], fec[1],
                                    first_block_id=first)
            decs[r].decode_received(rxb[r], masks[r])
        if "order" not in rec:
            break
        sent, adv_i = [], 0
        for r in rec["order"]:
            heard = list(sent)
            if heard:
                heard.append(device_content(*enc.repair_adv(state, None, fec[0], fec[1], obj, first)[::2]))
                assert bytes(heard[-1].cpu().numpy()) == rec["advs"][adv_i]
                adv_i += 1
            rx = decs[r].rx_repair_state(nb, device="cuda")
            if heard:
                lens = [int(c.numel()) for c in heard]
                decs[r].handle_repair_content(rx, masks[r], torch.cat(heard), _dev(np.cumsum([0] + lens[:-1]).astype(np.uint64)),
                                              _dev(np.array(lens, np.uint16)), None, fec[0], fec[1], obj, first)
            totals, words = decs[r].repair_pending(rx, masks[r])
            assert _np(totals, np.uint64).tolist() == rec["decisions"][r], (r, totals, rec["decisions"][r])
            assert np.array_equal(_np(words, np.uint32), rec["pending_words"][r])
            if rec["decisions"][r][0]:
                content = device_content(*decs[r].repair_requests(masks[r], None, fec[0], fec[1], obj, first)[::2])
                assert bytes(content.cpu().numpy()) == rec["nacks"][len(sent)]
                t = enc.handle_nacks(state, content, _dev(np.zeros(1, np.uint64)), _dev(np.array([content.numel()], np.uint16)),
                                     None, fec[0], fec[1], obj, first)
                assert _np(t, np.uint64)[4:].tolist() == [0, 0]
                sent.append(content)
        nacks += len(sent)
        assert len(sent) == len(rec["nacks"])
        enc.activate_repairs(state, pending)
        torch.cuda.synchronize()
        same_state(state.to_host(), rec["tx_state"])
    assert nacks == CYCLE_OBSERVED[1] and nacks < 3 * (len(model) - 1)
    for r in range(R):
        assert torch.equal(rxb[r][:, :k], src[:, :k])  # every source byte is the original
