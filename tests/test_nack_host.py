"""nfec_rx_repair_requests_host and nfec_repair_parse_host (norm_amd/csrc/nack_host.cpp, the rule of
nack_layout.hpp) against a serial walk written here the way the reference walks: first-pending /
next-pending iteration over one block (NormBlock::AppendRepairRequest, src/common/normSegment.cpp:
524-630), then over the blocks (NormObject::AppendRepairRequest, src/common/normObject.cpp:1179-1381,
flush form, NACK_NORMAL), with the items laid out by nfec_payload_id_write.  CPU only."""
import ctypes

import numpy as np
import pytest

import norm_amd
from norm_amd import _native as N

ITEMS, RANGES = 1, 2
SEGMENT, BLOCK, INFO = 1, 2, 4
SILENT, NEEDING, ABSENT = 0, 1, 2
PAIRS = [(5, 8), (2, 8), (2, 16), (129, 8), (129, 16)]


# ---- the serial walk ----

def item_bytes(fec_id, fec_m, object_id, block_id, symbol, nd):
    n = N.lib().nfec_payload_id_length(fec_id)
    buf = (ctypes.c_uint8 * n)()
    assert N.lib().nfec_payload_id_write(fec_id, fec_m, block_id & 0xFFFFFFFF, symbol, nd, buf) >= 0
    return bytes([fec_id, 0, object_id >> 8, object_id & 255]) + bytes(buf)


class Nack:
    """An unbounded NACK: AttachRepairRequest / AppendRepairItem / PackRepairRequest, plus the cut at
    max_units units.  units: what a parser has to yield, (flags, form, first, last)."""

    def __init__(self, fec_id, fec_m, object_id, first_block_id, info, max_units, nblocks):
        self.fec_id, self.fec_m, self.object_id, self.first = fec_id, fec_m, object_id, first_block_id
        self.info, self.max_units = INFO if info else 0, max_units
        self.out = bytearray()
        self.requests = 0
        self.at = np.zeros(nblocks + 1, np.uint64)  # bytes emitted at each block's position
        self.units = []
        self.bits = {5: 24, 129: 32}.get(fec_id, 24 if fec_m == 8 else 16)
        self.open = None  # [header offset, form, units]

    def pack(self):  # PackRepairRequest: the header's length field
        if self.open is not None:
            hdr = self.open[0]
            n = len(self.out) - hdr - 4
            self.out[hdr + 2:hdr + 4] = bytes([n >> 8, n & 255])
        self.open = None

    def unit(self, pos, flags, run, first, last):
        """first / last: (block of the call, symbol, nd)"""
        form = RANGES if run >= 3 else ITEMS
        before = len(self.out)
        if self.open is None or self.open[1] != form or self.open[2] == self.max_units:
            self.pack()
            self.open = [len(self.out), form, 0]
            self.out += bytes([form, flags | self.info, 0, 0])
            self.requests += 1
        self.open[2] += 1
        ends = [first] if run == 1 else [first, last]
        for b, s, nd in ends:
            self.out += item_bytes(self.fec_id, self.fec_m, self.object_id, self.first + b, s, nd)
        self.at[pos] += len(self.out) - before
        wire = [(self.object_id, (self.first + b) & ((1 << self.bits) - 1), nd if self.fec_id == 129 else 0, s)
                for b, s, nd in ends]
        if form == ITEMS:
            self.units += [(flags | self.info, form, w, w) for w in wire]
        else:
            self.units.append((flags | self.info, form, wire[0], wire[1]))


def block_stats(got, nd, m):
    e = int(np.count_nonzero(~got[:nd]))
    p = int(np.count_nonzero(got[nd:nd + m]))
    return e, p


def block_class(got, nd, k, m):
    if nd < 1 or nd > k:
        return SILENT
    if not got[:nd + m].any():
        return ABSENT
    e, p = block_stats(got, nd, m)
    return NEEDING if e > p else SILENT


def walk_block(nack, b, got, nd, m):
    """NormBlock::AppendRepairRequest (normSegment.cpp:524-630) with its own GetFirstPending /
    GetNextPending over the block's pending mask (pending = not received)."""
    n = nd + m

    def next_pending(s):  # the first pending slot at or behind s, or None
        while s < n and got[s]:
            s += 1
        return s if s < n else None

    erasure_count, _ = block_stats(got, nd, m)
    if erasure_count > m:  # :536-548: explicit repair, behind the first numParity pending ones
        nxt = next_pending(0)
        for _ in range(m):
            nxt = next_pending(nxt + 1)
        end = n
    else:  # :549-554
        nxt = next_pending(nd)
        end = nd + erasure_count
    if nxt is None:
        nxt = end
    count, first = 0, 0
    while nxt < end:  # :562-622
        cur = nxt
        nxt = next_pending(nxt + 1)
        if nxt is None:
            nxt = end
        if count == 0:
            first = cur
        count += 1
        if nxt - cur > 1 or nxt >= end:
            nack.unit(b, SEGMENT, count, (b, first, nd), (b, cur, nd))
            count = 0
    nack.pack()  # :623-629


def walk(k, m, got, nds, fec_id, fec_m, object_id, first_block_id, info, max_units):
    """NormObject::AppendRepairRequest (normObject.cpp:1179-1381), flush set: the object's pending
    blocks are the absent and the needing ones; a silent block is no longer pending."""
    nb = len(nds)
    cls = [block_class(got[b], nds[b], k, m) for b in range(nb)]
    nack = Nack(fec_id, fec_m, object_id, first_block_id, info, max_units, nb)
    pending = [b for b in range(nb) if cls[b] != SILENT]
    idx = 0
    iterating = idx < len(pending)
    nxt = pending[0] if iterating else 0
    prev, consecutive = nxt, 0
    while iterating or consecutive:  # :1194
        block = iterating and cls[nxt] == NEEDING  # block_buffer.Find (:1207)
        if block:
            append = True
        elif iterating and nxt - prev == consecutive:  # :1210
            consecutive += 1
            append = False
        else:
            append = True
        if append:
            if consecutive:  # :1216-1278: the run [prev, prev + consecutive)
                last = prev + consecutive - 1
                nack.unit(last, BLOCK, consecutive, (prev, 0, nds[prev]), (last, 0, nds[last]))
            if block:  # :1279-1335
                nack.pack()
                walk_block(nack, nxt, got[nxt], nds[nxt], m)
                consecutive = 0
            elif iterating:
                consecutive = 1
            else:
                consecutive = 0
            prev = nxt
        idx += 1  # :1347-1348
        iterating = idx < len(pending)
        nxt = pending[idx] if iterating else nxt + 1
    nack.pack()  # :1355-1364
    if not nack.out and info and nb:  # :1365-1379, the INFO-only request
        nack.out += bytes([ITEMS, INFO, 0, 0]) + item_bytes(fec_id, fec_m, object_id, 0, 0, 0)
        nack.pack_len = len(nack.out) - 4
        nack.out[2:4] = bytes([nack.pack_len >> 8, nack.pack_len & 255])
        nack.requests = 1
        nack.units.append((INFO, ITEMS, (object_id, 0, 0, 0), (object_id, 0, 0, 0)))
    start = np.zeros((nb + 1, 2), np.uint64)
    start[1:, 0] = np.cumsum(nack.at[:nb])
    start[:nb, 1] = cls
    start[nb] = (len(nack.out), nack.requests)
    totals = np.array([len(nack.out), nack.requests, cls.count(NEEDING), cls.count(ABSENT)], np.uint64)
    return np.frombuffer(bytes(nack.out), np.uint8), start, totals, nack.units


# ---- masks ----

def to_words(got, nds, m, stride=None, rng=None):
    """bool [nb, k + m] -> uint32 [nb, stride]; bits at or past nd + m are noise (they are ignored)"""
    nb, n = got.shape
    stride = (n + 31) // 32 if stride is None else stride
    bits = np.zeros((nb, stride * 32), bool)
    bits[:, :n] = got
    for b in range(nb):
        lim = nds[b] + m if 1 <= nds[b] else n
        if rng is not None and lim < stride * 32:
            bits[b, lim:] = rng.random(stride * 32 - lim) < 0.5
    return np.packbits(bits.reshape(nb, stride, 32), axis=2, bitorder="little").view(np.uint32).reshape(nb, stride)


def check(k, m, got, nds=None, fec=(5, 8), object_id=0x1234, first_block_id=0, info=False, max_units=None,
          stride=None, rng=None, capacity=None):
    got = np.asarray(got, bool)
    nb = got.shape[0]
    nds = [k] * nb if nds is None else list(nds)
    max_units = norm_amd.repair_max_units(fec[0]) if max_units is None else max_units
    want, w_start, w_totals, units = walk(k, m, got, nds, fec[0], fec[1], object_id, first_block_id, info, max_units)
    words = to_words(got, nds, m, stride, rng)
    keep = words.copy()
    content, start, totals = norm_amd.rx_repair_requests_host(
        k, m, words, np.array(nds, np.uint16), fec[0], fec[1], object_id, first_block_id,
        N.NFEC_NACK_INFO if info else 0, max_units, capacity)
    assert np.array_equal(words, keep)
    assert np.array_equal(totals, w_totals), (totals, w_totals)
    assert np.array_equal(start, w_start)
    n = min(len(want), len(content))
    assert np.array_equal(content[:n], want[:n])
    assert not content[n:].any()  # nothing behind the total (or the capacity)
    if capacity is None:
        fl, fm, first, last, consumed = norm_amd.repair_parse_host(fec[0], fec[1], content[:len(want)])
        assert consumed == len(want)
        have = [(int(fl[i]), int(fm[i]), tuple(int(x) for x in first[i]), tuple(int(x) for x in last[i]))
                for i in range(len(fl))]
        assert have == units
    return want, units, totals


def lossy(rng, nb, k, m, loss):
    return rng.random((nb, k + m)) >= loss


# ---- random masks ----

@pytest.mark.parametrize("k,m,nb", [(4, 2, 40), (8, 4, 40), (64, 32, 24), (200, 55, 12), (4096, 256, 3)])
@pytest.mark.parametrize("loss", [0.05, 0.3, 0.5, 0.7, 0.95])
def test_random_masks(k, m, nb, loss):
    rng = np.random.default_rng(1000 * k + int(loss * 100))
    fec = (5, 8) if k + m <= 256 else (2, 16)
    got = lossy(rng, nb, k, m, loss)
    nds = [k if rng.random() < 0.5 else k - 1 for _ in range(nb)]
    for b in range(nb):
        r = rng.random()
        if r < 0.15:
            got[b] = False  # absent
        elif r < 0.3:
            got[b, :nds[b]] = True  # silent: complete
        got[b, nds[b] + m:] = False
    nds[nb // 2] = 0  # invalid: silent
    for max_units in (None, 1, 2, 3):
        check(k, m, got, nds, fec=fec, max_units=max_units, rng=rng, first_block_id=77)
    check(k, m, got, nds, fec=fec, info=True, stride=(k + m + 31) // 32 + 2, rng=rng)


# ---- named corners ----

def block_with_runs(k, m, runs):
    """A needing block of (k, m) that asks for exactly `runs` = [(start, length)] of its source
    slots: m filler slots at the front are the pending ones the explicit-repair rule skips, and the
    parity has arrived (e = m + the runs > p = m)."""
    got = np.ones(k + m, bool)
    got[:m] = False
    for s, n in runs:
        got[s:s + n] = False
    return got


@pytest.mark.parametrize("edge", [32, 64])
@pytest.mark.parametrize("length", [1, 2, 3, 4])
def test_runs_straddling_word_edges(edge, length):
    k, m = 200, 20
    for back in range(length + 1):  # how many of the run's slots lie in front of the edge
        start = edge - back
        got = block_with_runs(k, m, [(start, length), (start + length + 1, 1), (start + length + 3, 5)])
        want, units, _ = check(k, m, got[None, :])
        seg = [u for u in units if u[0] & SEGMENT]
        assert seg[0][2][3] == start and seg[0][3][3] == (start if length <= 2 else start + length - 1)


@pytest.mark.parametrize("length", [1, 2, 3, 4])
def test_runs_straddling_the_64_word_round(length):
    k, m = 4096, 256
    for back in range(length + 1):
        start = 2048 - back
        got = block_with_runs(k, m, [(start, length), (start + length + 2, 2), (3000, 700)])
        check(k, m, got[None, :], fec=(2, 16))
        check(k, m, got[None, :], fec=(129, 16), max_units=1)


def test_erasures_against_m_and_p():
    k, m = 16, 4
    for e, p in [(m, 0), (m + 1, 0), (m + 1, m), (2, 2), (3, 2), (1, 0), (m, m - 1), (m, m), (k, 0), (k, m)]:
        got = np.ones(k + m, bool)
        got[1:1 + e] = False
        got[k:] = False
        got[k + m - p:] = True  # the received parity at the end: [nd, nd + e) starts pending
        want, units, totals = check(k, m, got[None, :])
        assert int(totals[2]) == (1 if e > p else 0)
        if e > p and e <= m:  # the pending slots of [nd, nd + e)
            asked = set()
            for u in units:
                asked |= set(range(u[2][3], u[3][3] + 1))
            assert asked == {s for s in range(k, k + e) if not got[s]} and asked


def test_request_set_ends_inside_a_run():
    k, m = 16, 8
    got = np.ones(k + m, bool)
    got[[2, 5, 9]] = False  # e = 3 <= m: parity [16, 19) of the pending run [16, 24)
    got[k:] = False
    want, units, _ = check(k, m, got[None, :])
    assert units == [(SEGMENT, RANGES, (0x1234, 0, 0, 16), (0x1234, 0, 0, 18))]
    got[17] = True  # [16], [18]: two single items in one request
    want, units, _ = check(k, m, got[None, :])
    assert [u[2][3] for u in units] == [16, 18] and len(want) == 4 + 2 * 8


def blocks_from_classes(k, m, classes):
    got = np.zeros((len(classes), k + m), bool)
    for b, c in enumerate(classes):
        if c == SILENT:
            got[b, :k] = True
        elif c == NEEDING:
            got[b, 0] = True  # e = k - 1 > m, p = 0
    return got


A, S, Nd = ABSENT, SILENT, NEEDING


@pytest.mark.parametrize("classes,requests", [
    ([A, S, A, A, S, A], 1),            # ITEMS, ITEMS, ITEMS share a request
    ([A, S, A, A, A, S, A], 3),         # ITEMS then RANGES then ITEMS do not
    ([A, A, A, S, A, A, A, A], 1),      # RANGES, RANGES
    ([A, A, Nd, A, A, A], 3),           # a needing block between two absent runs
    ([Nd, Nd, A], 3),
    ([S, A, S], 1),
    ([A] * 7, 1),                       # everything absent
    ([S] * 5, 0),                       # everything silent
    ([Nd], 1),
])
def test_block_level_chains(classes, requests):
    k, m = 8, 2
    got = blocks_from_classes(k, m, classes)
    for fec in PAIRS:
        want, units, totals = check(k, m, got, fec=fec)
        assert int(totals[1]) == requests
        want, units, totals = check(k, m, got, fec=fec, info=True)
        assert int(totals[1]) == max(requests, 1)  # the INFO-only request when nothing else is asked
        assert all(u[0] & INFO for u in units)
    for max_units in (1, 2):
        check(k, m, got, max_units=max_units)


def test_max_units_cuts_a_stretch():
    k, m = 64, 4
    got = block_with_runs(k, m, [(10 + 2 * i, 1) for i in range(9)])  # nine single items
    for max_units, requests in [(1, 9), (2, 5), (4, 3), (9, 1), (100, 1)]:
        want, units, totals = check(k, m, got[None, :], max_units=max_units)
        assert int(totals[1]) == requests and len(units) == 9


def test_capacity_below_the_total():
    rng = np.random.default_rng(5)
    k, m = 64, 32
    got = lossy(rng, 10, k, m, 0.6)
    want, _, totals = check(k, m, got)
    for cap in (0, 1, 3, 4, 5, len(want) // 2 + 1, len(want) - 1, len(want)):
        _, _, t = check(k, m, got, capacity=cap)
        assert np.array_equal(t, totals)


@pytest.mark.parametrize("fec,first", [((5, 8), 0xFFFFFD), ((2, 8), 0xFFFFFE), ((2, 16), 0xFFFE), ((129, 8), 0xFFFFFFFD),
                                       ((129, 16), 0xFFFFFFFF)])
def test_first_block_id_wraps_the_block_field(fec, first):
    k, m = 8, 2
    got = blocks_from_classes(k, m, [A, A, A, A, S, Nd, A, S, A, A])
    want, units, _ = check(k, m, got, fec=fec, first_block_id=first, nds=[8, 7, 8, 7, 8, 8, 7, 8, 8, 7])
    assert units[0][2][1] == first and units[0][3][1] == (first + 3) % (1 << {5: 24, 129: 32}.get(fec[0], 24 if fec[1] == 8 else 16))


def test_argument_checks():
    L = N.lib()
    k, m = 8, 2
    words = np.zeros((2, 1), np.uint32)
    content = np.zeros(256, np.uint8)
    start = np.zeros((3, 2), np.uint64)
    totals = np.ones(4, np.uint64)

    def call(fec_id=5, fec_m=8, flags=0, max_units=1, stride=1, nb=2, mask=words.ctypes.data, bs=start.ctypes.data,
             tot=totals.ctypes.data, cont=content.ctypes.data, kk=k):
        return L.nfec_rx_repair_requests_host(kk, m, mask, stride, None, nb, fec_id, fec_m, 1, 0, flags, max_units, cont,
                                              content.size, bs, tot)

    assert call() == N.NFEC_OK
    for bad in (dict(fec_id=0), dict(fec_id=2, fec_m=4), dict(fec_id=130), dict(flags=2), dict(max_units=0),
                dict(max_units=65535 // 16 + 1), dict(fec_id=129, max_units=65535 // 24 + 1), dict(stride=0),
                dict(mask=None), dict(bs=None), dict(tot=None), dict(cont=None), dict(kk=0)):
        assert call(**bad) == N.NFEC_EINVAL, bad
    assert call(max_units=65535 // 16) == N.NFEC_OK and call(fec_id=129, max_units=65535 // 24) == N.NFEC_OK
    assert call(nb=0, mask=None, flags=1) == N.NFEC_OK and not totals.any()


# ---- the parser ----

def test_parse_stops_where_the_rule_says():
    k, m = 64, 4
    got = np.stack([block_with_runs(k, m, [(10, 1), (12, 2), (20, 5), (30, 1)]),
                    block_with_runs(k, m, [(40, 3)])])
    want, units, _ = check(k, m, got, fec=(129, 8))
    # requests: b0 ITEMS(3 items) RANGES(1) ITEMS(1); b1 RANGES(1)
    L = 12
    sizes = [4 + 3 * L, 4 + 2 * L, 4 + L, 4 + 2 * L]
    assert len(want) == sum(sizes)

    def parse(buf, fec=(129, 8)):
        fl, fm, first, last, consumed = norm_amd.repair_parse_host(fec[0], fec[1], buf)
        return len(fl), consumed

    assert parse(want) == (6, len(want))
    assert parse(want[:0]) == (0, 0) and parse(want[:3]) == (0, 0)
    # truncated inside the second request: its length exceeds what is left
    assert parse(want[:sizes[0] + 4 + L]) == (3, sizes[0])
    assert parse(want[:sizes[0] + 3]) == (3, sizes[0])
    # a length field that claims more than there is
    big = want.copy()
    big[2:4] = (0xFF, 0xFF)
    assert parse(big) == (0, 0)
    # a foreign fec_id in the first request's third item, and in a range's second item
    bad = want.copy()
    bad[4 + 2 * L] = 5
    assert parse(bad) == (2, 4 + 2 * L)
    bad = want.copy()
    bad[sizes[0] + 4 + L] = 2
    assert parse(bad) == (3, sizes[0] + 4)
    # a RANGES request with an odd item count
    odd = want.copy()
    odd[sizes[0] + 2:sizes[0] + 4] = (0, L)
    assert parse(odd) == (3, sizes[0])
    # bytes behind a request's last whole item are skipped
    pad = np.concatenate([want[:sizes[0]], np.zeros(4, np.uint8), want[sizes[0]:]])
    pad[2:4] = ((3 * L + 4) >> 8, (3 * L + 4) & 255)
    assert parse(pad) == (6, len(pad))
    assert N.lib().nfec_repair_parse_host(3, 8, want.ctypes.data, want.size, None, None, None, None, 0, None) == N.NFEC_EINVAL
    # the arrays hold `capacity` units, the count is the full one
    fl = np.zeros(2, np.uint8)
    assert N.lib().nfec_repair_parse_host(129, 8, want.ctypes.data, want.size, fl.ctypes.data, None, None, None, 2, None) == 6


# ---- the scans' operator ----

def test_scan_operator_is_associative():
    rng = np.random.default_rng(11)

    def comb(a, b):
        x, y, out = np.array(a, np.uint64), np.array(b, np.uint64), np.zeros(2, np.uint64)
        N.lib().nfec_nack_scan_combine_host(x.ctypes.data, y.ctypes.data, out.ctypes.data)
        return tuple(int(v) for v in out)

    for _ in range(2000):
        a, b, c = [(int(rng.integers(0, 1 << 40)), int(rng.integers(0, 2))) for _ in range(3)]
        assert comb(comb(a, b), c) == comb(a, comb(b, c))
        assert comb((0, 0), a) == a and comb(a, (0, 0)) == a
    # a scan by the operator is the serial state: the run length of 1 1 0 1 1 1
    state = (0, 0)
    seen = []
    for absent in (1, 1, 0, 1, 1, 1):
        state = comb(state, (1, 0) if absent else (0, 1))
        seen.append(state[0])
    assert seen == [1, 2, 0, 1, 2, 3]
