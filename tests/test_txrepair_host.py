"""nfec_tx_handle_nacks_host, nfec_tx_activate_repairs_host and nfec_tx_end_blocks_host
(norm_amd/csrc/tx_repair_host.cpp, the rule of repair_layout.hpp) against a serial walk written here
the way the reference iterates: a Block with repair_mask, parity_offset and parity_count, the
SenderHandleNackMessage loop (src/common/normSession.cpp:3706-4300, the !holdoff arm) with its
freshObject / freshBlock / prevBlockId / numErasures variables, and NormBlock::HandleSegmentRequest
(src/common/normSegment.cpp:341-402), NormBlock::TxReset (:219-259), NormObject::ActivateRepairs
(src/common/normObject.cpp:472-537) and ResetParityCount line for line.  CPU only."""
import itertools

import numpy as np
import pytest

import norm_amd
from norm_amd import _native as N
from test_nack_host import item_bytes, to_words

ITEMS, RANGES = 1, 2
SEGMENT, BLOCK, INFO, OBJECT = 1, 2, 4, 8
R_OBJECT, R_INFO, P_INFO = N.NFEC_TX_REPAIR_OBJECT, N.NFEC_TX_REPAIR_INFO, N.NFEC_TX_PENDING_INFO
OBJ = 0xBEEF
BITS = {(5, 8): 24, (2, 8): 24, (2, 16): 16, (129, 8): 32, (129, 16): 32}


# ---- the serial walk ----

class Block:
    def __init__(self, nd, m, parity_offset=0, parity_count=0):
        self.nd = nd
        self.repair_mask = np.zeros(max(nd, 0) + m, bool)
        self.pending_mask = np.zeros(max(nd, 0) + m, bool)
        self.parity_offset, self.parity_count = parity_offset, parity_count

    def set_bits(self, first, count):  # ProtoBitmask::SetBits, clipped at the mask's size
        self.repair_mask[first:first + count] = True

    def handle_segment_request(self, next_id, last_id, num_data, num_parity, erasure_count):
        if next_id < num_data:
            self.parity_count = self.parity_offset = num_parity
            while next_id <= last_id:
                if next_id < len(self.repair_mask):
                    self.repair_mask[next_id] = True
                next_id += 1
        else:
            parity_available = num_parity - self.parity_offset
            if erasure_count <= parity_available:
                if erasure_count > self.parity_count:
                    self.set_bits(num_data + self.parity_offset + self.parity_count, erasure_count - self.parity_count)
                    self.parity_count = erasure_count
            else:
                if self.parity_count < parity_available:
                    count = parity_available - self.parity_count
                    self.set_bits(num_data + self.parity_offset + self.parity_count, count)
                    self.parity_count = parity_available
                    next_id += parity_available
                while next_id <= last_id:
                    if next_id < len(self.repair_mask):
                        self.repair_mask[next_id] = True
                    next_id += 1

    def tx_reset(self, num_data, num_parity, auto_parity):
        increased = False
        self.repair_mask[:] = False
        self.repair_mask[:num_data + auto_parity] = True
        self.repair_mask ^= self.pending_mask
        if self.repair_mask.any():
            increased = True
            self.repair_mask[:] = False
            self.pending_mask[:num_data + auto_parity] = True
            self.pending_mask[num_data + auto_parity:] = False
            self.parity_offset, self.parity_count = auto_parity, num_parity
        return increased

    def reset_parity_count(self, num_parity):
        self.parity_offset = min(self.parity_offset + self.parity_count, num_parity)
        self.parity_count = 0


class Sender:
    """One object's sender state.  nds: numData per block (outside [1, k]: no block is held)."""

    def __init__(self, k, m, nds, auto_parity=0, fec=(5, 8), first=0, object_id=OBJ, parity_offset=None):
        self.k, self.m, self.nds, self.auto = k, m, list(nds), auto_parity
        self.fec, self.first, self.object_id = fec, first, object_id
        self.blocks = [Block(nd if 1 <= nd <= k else 0, m, auto_parity if parity_offset is None else parity_offset)
                       for nd in nds]
        for blk in self.blocks:
            blk.pending_mask[:blk.nd + auto_parity] = blk.nd > 0
        self.repair_mask = set()  # NormObject::repair_mask
        self.word = 0

    def held(self, b):
        return b < len(self.nds) and 1 <= self.nds[b] <= self.k

    def block_of(self, block_id):
        return (block_id - self.first) & ((1 << BITS[self.fec]) - 1)

    def handle_nack(self, units, extra_parity):
        """units: (flags, (obj, block id, block len, symbol) first, the same last).  Returns
        (SEGMENT units applied, units not applied or ignored, block bits newly set)."""
        applied = ignored = newly = 0
        fresh_object, fresh_block, prev_block_id, num_erasures = True, True, None, extra_parity
        for flags, first, last in units:
            if flags & SEGMENT:
                level = SEGMENT
            elif flags & BLOCK:
                level = BLOCK
            elif flags & OBJECT:
                level = OBJECT
            elif flags & INFO:
                level = INFO
            else:
                ignored += 1
                continue
            if level in (OBJECT, INFO):
                own = ((self.object_id - first[0]) & 0xFFFF) <= ((last[0] - first[0]) & 0xFFFF)
            else:
                own = first[0] == self.object_id
            if not own:
                fresh_object = True
                ignored += 1
                continue
            if fresh_object:
                fresh_block, fresh_object = True, False
            if flags & INFO:
                self.word |= R_INFO
            if level == OBJECT:
                self.word |= R_OBJECT
            elif level == BLOCK:
                b0, b1 = self.block_of(first[1]), self.block_of(last[1])
                if b0 <= b1 and b0 < len(self.nds):
                    for b in range(b0, min(b1, len(self.nds) - 1) + 1):
                        newly += b not in self.repair_mask
                        self.repair_mask.add(b)
            elif level == SEGMENT:
                b = self.block_of(first[1])
                if b != prev_block_id:
                    fresh_block = True
                if not self.held(b) or last[3] < first[3]:
                    fresh_block = True
                    ignored += 1
                    continue
                if fresh_block:
                    if b in self.repair_mask:  # IsRepairSet
                        ignored += 1
                        continue
                    fresh_block, num_erasures, prev_block_id = False, extra_parity, b
                num_erasures = (num_erasures + last[3] - first[3] + 1) & 0xFFFFFFFF
                self.blocks[b].handle_segment_request(first[3], last[3], self.nds[b], self.m, num_erasures)
                applied += 1
        return applied, ignored, newly

    def activate(self):
        """OnRepairTimeout for the object.  Returns (blocks reset with a change, blocks activated, pending bits)."""
        changed = activated = 0
        if self.word & R_OBJECT:  # NormObject::TxReset
            for b, blk in enumerate(self.blocks):
                if self.held(b):
                    changed += blk.tx_reset(self.nds[b], self.m, self.auto)
        else:  # NormObject::ActivateRepairs
            for b in sorted(self.repair_mask):
                if self.held(b):
                    changed += self.blocks[b].tx_reset(self.nds[b], self.m, self.auto)
            for b, blk in enumerate(self.blocks):
                if self.held(b) and blk.repair_mask.any():
                    blk.pending_mask |= blk.repair_mask
                    blk.repair_mask[:] = False
                    activated += 1
        self.repair_mask.clear()
        word = self.word & ~(R_OBJECT | R_INFO)
        if (self.word & R_INFO) or changed:
            word |= P_INFO
        self.word = word
        return changed, activated, sum(int(blk.pending_mask.sum()) for b, blk in enumerate(self.blocks) if self.held(b))

    def end_blocks(self):
        for b, blk in enumerate(self.blocks):
            if self.held(b) and not blk.pending_mask.any():
                blk.reset_parity_count(self.m)

    # the state as the library's arrays
    def masks(self, which, stride):
        out = np.zeros((len(self.blocks), stride * 32), bool)
        for b, blk in enumerate(self.blocks):
            out[b, :len(getattr(blk, which))] = getattr(blk, which) if self.held(b) else False
        return np.packbits(out.reshape(len(self.blocks), stride, 32), axis=2, bitorder="little").view(np.uint32).reshape(
            len(self.blocks), stride)

    def state(self, stride=None):
        stride = (self.k + self.m + 31) // 32 if stride is None else stride
        nb = len(self.blocks)
        parity = np.array([[blk.parity_offset, blk.parity_count] for blk in self.blocks], np.uint16).reshape(nb, 2)
        br = np.zeros(max(1, (nb + 31) // 32), np.uint32)
        for b in self.repair_mask:
            br[b >> 5] |= np.uint32(1 << (b & 31))
        return norm_amd.TxRepairState(self.masks("repair_mask", stride), parity, br, np.array([self.word], np.uint32))

    def pending(self, stride=None):
        return self.masks("pending_mask", (self.k + self.m + 31) // 32 if stride is None else stride)


# ---- content ----

def parse(fec, content):
    """NormRepairRequest::Unpack and ::Iterator over one message, in Python: (units, cut short)"""
    L = 4 + N.lib().nfec_payload_id_length(fec[0])
    at, units = 0, []

    def item(o):
        raw = content[o + 4:o + L]
        if fec[0] == 129:
            return (content[o + 2] << 8 | content[o + 3], int.from_bytes(raw[:4], "big"), int.from_bytes(raw[4:6], "big"),
                    int.from_bytes(raw[6:8], "big"))
        v = int.from_bytes(raw, "big")
        if BITS[fec] == 24:
            return (content[o + 2] << 8 | content[o + 3], v >> 8, 0, v & 0xFF)
        return (content[o + 2] << 8 | content[o + 3], v >> 16, 0, v & 0xFFFF)

    while len(content) - at >= 4:
        form, flags, ln = content[at], content[at + 1], content[at + 2] << 8 | content[at + 3]
        if ln > len(content) - at - 4:
            break
        count, step = ln // L, 2 if form == RANGES else 1
        if form == RANGES and count & 1:
            break
        o, foreign = at + 4, False
        for _ in range(0, count, step):
            if content[o] != fec[0] or (step == 2 and content[o + L] != fec[0]):
                foreign = True
                break
            units.append((flags, item(o), item(o + (step - 1) * L)))
            o += step * L
        if foreign:
            at = o
            break
        at += 4 + ln
    return units, at != len(content)


def request(form, flags, items, fec=(5, 8), object_id=OBJ, first=0, nd=0):
    """one request; items: (block of the batch, symbol) or (object id, block, symbol)"""
    body = b""
    for it in items:
        obj, b, s = it if len(it) == 3 else (object_id,) + tuple(it)
        body += item_bytes(fec[0], fec[1], obj, first + b, s, nd)
    return bytes([form, flags, len(body) >> 8, len(body) & 255]) + body


def seg_items(b, *symbols, **kw):
    return request(ITEMS, SEGMENT, [(b, s) for s in symbols], **kw)


def seg_range(b, lo, hi, **kw):
    return request(RANGES, SEGMENT, [(b, lo), (b, hi)], **kw)


def block_range(b0, b1, **kw):
    return request(RANGES, BLOCK, [(b0, 0), (b1, 0)], **kw)


class Case:
    """A sender state in front of a handle call, and the call's messages in a wire buffer."""

    def __init__(self, k, m, nds, messages, fec=(5, 8), first=0, extra=0, parity_offset=None, auto=0, align=0, gap=0,
                 block_repair=(), word=0, stride=None, name=""):
        self.k, self.m, self.nds, self.fec, self.first, self.extra = k, m, list(nds), fec, first, extra
        self.auto, self.parity_offset, self.block_repair, self.word, self.stride = auto, parity_offset, block_repair, word, stride
        self.name = name
        self.messages = [bytes(x) for x in messages]
        wire, off = bytearray(b"\xA5" * align), []
        for x in self.messages:
            off.append(len(wire))
            wire += x + b"\xA5" * gap
        self.wire = np.frombuffer(bytes(wire[:len(wire) - gap if gap and self.messages else len(wire)]), np.uint8).copy()
        self.offsets = np.array(off, np.uint64)
        self.lengths = np.array([len(x) for x in self.messages], np.uint16)
        self.payload_bytes = None
        self.count = None

    def sender(self):
        s = Sender(self.k, self.m, self.nds, self.auto, self.fec, self.first, OBJ, self.parity_offset)
        s.repair_mask, s.word = set(self.block_repair), self.word
        return s

    def readable(self, i):
        size = self.wire.size if self.payload_bytes is None else self.payload_bytes
        return int(self.offsets[i]) <= size and int(self.lengths[i]) <= size - int(self.offsets[i])

    def expected(self):
        """the serial walk: (sender behind the call, totals)"""
        s = self.sender()
        totals = np.zeros(6, np.uint64)
        n = len(self.messages) if self.count is None else min(self.count, len(self.messages))
        for i in range(n):
            if not self.readable(i):
                totals[5] += 1
                continue
            o, ln = int(self.offsets[i]), int(self.lengths[i])
            units, cut = parse(self.fec, bytes(self.wire[o:o + ln]))
            a, g, w = s.handle_nack(units, self.extra)
            totals += np.array([len(units), a, g, w, cut, 0], np.uint64)
        return s, totals

    def host(self, unit_capacity=None, state=None):
        """the host entry: (state behind the call, totals)"""
        state = self.sender().state(self.stride) if state is None else state
        totals = norm_amd.tx_handle_nacks_host(self.k, self.m, state, self.wire, self.offsets, self.lengths,
                                               np.array(self.nds, np.uint16), self.fec[0], self.fec[1], OBJ, self.first,
                                               self.extra, unit_capacity, self.count, self.payload_bytes)
        return state, totals


def same_state(a, b):
    for f in norm_amd.TxRepairState.FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        assert np.array_equal(x, y), (f, np.argwhere(x != y)[:4].tolist(), x.ravel()[:8], y.ravel()[:8])


def check(case):
    want, want_totals = case.expected()
    got, totals = case.host()
    assert np.array_equal(totals, want_totals), (case.name, totals, want_totals)
    same_state(got, want.state(case.stride))
    return want, want_totals


def bits_of(state, b):
    return [int(s) for s in np.flatnonzero(np.unpackbits(state.repair[b].view(np.uint8), bitorder="little"))]


# ---- the corner contents (tests/test_gpu_txrepair.py runs them on the device too) ----

def order_pair(order):
    """k = 8, m = 4, parity {1, 0}: 3 parity segments are available.  A = RANGES (8, 12), E 5;
    B = RANGES (8, 10), E 3."""
    a, b = seg_range(0, 8, 12), seg_range(0, 8, 10)
    return Case(8, 4, [8], [a, b] if order == "AB" else [b, a], parity_offset=1, name="order " + order)


def stretch_cases():
    k, m, nds = 8, 4, [8, 8, 8]
    foreign = request(ITEMS, SEGMENT, [(OBJ + 1, 0, 9)])
    return [
        Case(k, m, nds, [seg_items(1, 8) + seg_range(1, 9, 11)], name="E accumulates over ITEMS and RANGES"),
        Case(k, m, nds, [seg_items(1, 8, 9) + foreign + seg_range(1, 9, 11)], name="a foreign unit restarts E"),
        Case(k, m, nds, [seg_items(1, 8) + block_range(1, 1) + seg_range(1, 9, 10)],
             name="a BLOCK-level request does not restart E, and the stretch goes on over the bit it set"),
        Case(k, m, nds, [seg_items(1, 8) + block_range(1, 1) + seg_range(1, 9, 10), seg_range(1, 9, 10) + seg_items(2, 8)],
             name="the same unit in a later message is skipped"),
        Case(k, m, nds, [seg_items(1, 8) + seg_items(2, 8) + seg_items(1, 9)], name="another block in between opens a stretch"),
        Case(k, m, nds, [seg_items(1, 8) + request(RANGES, SEGMENT, [(1, 9), (1, 8)]) + seg_items(1, 10)],
             name="a backwards range is not applied and ends the stretch"),
        Case(k, m, nds, [seg_items(1, 8) + request(ITEMS, 0, [(1, 9)]) + request(ITEMS, OBJECT, [(0, 0)])
                         + request(ITEMS, INFO, [(0, 0)]) + seg_items(1, 9)], extra=1,
             name="requests without a level and OBJECT / INFO requests are transparent"),
        Case(k, m, nds, [request(RANGES, OBJECT, [(OBJ - 2, 0, 0), (OBJ + 2, 0, 0)]),
                         request(RANGES, INFO | OBJECT, [(OBJ + 1, 0, 0), (OBJ + 2, 0, 0)]),
                         request(ITEMS, SEGMENT | INFO, [(2, 3)])], name="object ranges and the INFO flag"),
        Case(k, m, nds, [request(RANGES, BLOCK, [(1, 0), (7, 0)]) + request(RANGES, BLOCK, [(2, 0), (1, 0)])
                         + request(ITEMS, BLOCK, [(3, 0), (0, 0)]) + seg_items(7, 1)], block_repair={0},
             name="block ranges are clipped at the batch"),
    ]


def id_form_cases():
    out = []
    for fec in BITS:
        first = (1 << BITS[fec]) - 2  # the window wraps the block field behind block 1
        kw = dict(fec=fec, first=first, nd=8)
        body = (seg_items(0, 8, 9, **kw) + seg_range(3, 2, 9, **kw) + block_range(1, 2, **kw)
                + request(ITEMS, SEGMENT, [(OBJ ^ 1, 0, 1)], **kw) + seg_items(2, 8, **kw) + seg_range(4, 9, 11, **kw))
        for align in range(4):
            out.append(Case(8, 4, [8] * 5, [body, seg_items(3, 10, **kw)], fec=fec, first=first, align=align, gap=align ^ 1,
                            name=f"fec {fec} align {align}"))
    return out


def shortened_cases():
    k, m, nds = 8, 4, [5, 8, 1, 0, 9]
    return [Case(k, m, nds, [seg_range(0, 3, 11) + seg_range(2, 1, 4) + seg_items(3, 0) + seg_items(4, 0) + seg_items(1, 11, 12)
                             + seg_range(2, 5, 200) + seg_range(0, 6, 8)], stride=2, name="shortened blocks")]


def damaged_case():
    good = seg_items(0, 8) + seg_range(1, 8, 9)
    cut_item = good + seg_items(1, 10, 11)[:-3]
    long_header = good + bytes([ITEMS, SEGMENT, 0, 64]) + item_bytes(5, 8, OBJ, 1, 10, 0)
    odd_ranges = good + request(RANGES, SEGMENT, [(1, 9), (1, 10), (1, 11)])
    foreign_fec = bytearray(good + seg_items(1, 10, 11))
    foreign_fec[-8] = 2  # the last item's fec_id
    tail = good + b"\x01\x01\x00"
    # a request whose length leaves bytes behind its last whole item: they are skipped
    slack = bytes([ITEMS, SEGMENT, 0, 11]) + item_bytes(5, 8, OBJ, 2, 8, 0) + b"\x05\x00\x00" + seg_items(2, 9)
    c = Case(8, 4, [8, 8, 8], [cut_item, long_header, odd_ranges, bytes(foreign_fec), tail, slack, good], name="damaged")
    return c


def unreadable_case():
    c = Case(8, 4, [8, 8], [seg_items(0, 8), seg_items(1, 8, 9), seg_items(0, 9)], name="unreadable")
    c.offsets = np.array([c.offsets[0], c.wire.size - 4, 1 << 40], np.uint64)  # the second reaches past the end
    return c


def count_dev_case():
    c = Case(8, 4, [8, 8], [seg_items(0, 8), seg_items(1, 8, 9), seg_range(0, 0, 3)], name="count_dev below count")
    c.count = 2
    return c


def corner_cases():
    return ([order_pair("AB"), order_pair("BA")] + stretch_cases() + id_form_cases() + shortened_cases()
            + [damaged_case(), unreadable_case(), count_dev_case()])


# ---- tests ----

def test_exhaustive_small_shape():
    """(k, m) = (3, 2), two blocks, every starting parity_offset 0..2 and extra_parity 0..1, every
    sequence of up to three units.  The alphabet is thinned from 43 letters to 14 so that 6 * (14 +
    14^2 + 14^3) = 17,724 one-message runs stay, plus, for extra_parity 0, the 8,862 runs with every
    unit in a message of its own: of the 21 (first, last) pairs at block 0 the nine that differ in
    which of {source, parity, past the end} they start and end in and in their width ((0,0), (0,2),
    (2,3), (2,4), (0,5), (3,3), (3,4), (4,4), (3,5)), at block 1 four ((0,1), (3,3), (3,4), (4,5)), and
    the BLOCK unit over block 0."""
    k, m, nds = 3, 2, [3, 3]
    letters = [(0, p) for p in ((0, 0), (0, 2), (2, 3), (2, 4), (0, 5), (3, 3), (3, 4), (4, 4), (3, 5))]
    letters += [(1, p) for p in ((0, 1), (3, 3), (3, 4), (4, 5))] + [None]
    assert len(letters) == 14

    def content(letter):
        if letter is None:
            return request(ITEMS, BLOCK, [(0, 0)])
        b, (lo, hi) = letter
        return seg_items(b, lo) if lo == hi else seg_range(b, lo, hi)

    contents = [content(x) for x in letters]
    runs = 0
    for n in (1, 2, 3):
        for seq in itertools.product(range(len(letters)), repeat=n):
            for offset0 in range(3):
                for extra in range(2):
                    check(Case(k, m, nds, [b"".join(contents[i] for i in seq)], extra=extra, parity_offset=offset0, name=str(seq)))
                    runs += 1
                    if extra == 0:
                        check(Case(k, m, nds, [contents[i] for i in seq], parity_offset=offset0, name=str(seq) + " split"))
                        runs += 1
    assert runs == 17724 + 8862


def test_order_decides():
    """A then B leaves the repair bits {9..11}, B then A {8..11} (slot 12 of the ranges lies past
    nd + m and is never set): derived from the reference's lines; the serial walk is the judge."""
    ab, _ = check(order_pair("AB"))
    ba, _ = check(order_pair("BA"))
    got_ab, got_ba = bits_of(order_pair("AB").host()[0], 0), bits_of(order_pair("BA").host()[0], 0)
    assert got_ab == bits_of(ab.state(), 0) and got_ba == bits_of(ba.state(), 0)
    assert got_ab == [9, 10, 11] and got_ba == [8, 9, 10, 11]
    assert got_ab != got_ba


@pytest.mark.parametrize("case", stretch_cases(), ids=lambda c: c.name)
def test_stretch_and_fresh_rules(case):
    want, totals = check(case)
    if case.name.startswith("E accumulates"):
        assert bits_of(want.state(), 1) == [8, 9, 10, 11]  # E = 1, then 1 + 3
    if case.name.startswith("a foreign unit"):
        assert bits_of(want.state(), 1) == [8, 9, 10]  # E = 2, then 3 again
    if case.name.startswith("a BLOCK-level request"):
        assert bits_of(want.state(), 1) == [8, 9, 10] and totals[1] == 2 and totals[3] == 1
    if case.name.startswith("the same unit"):
        assert bits_of(want.state(), 1) == [8, 9, 10] and totals[1] == 3 and totals[2] == 1


@pytest.mark.parametrize("case", id_form_cases(), ids=lambda c: c.name)
def test_id_forms_and_alignment(case):
    _, totals = check(case)
    assert totals[1] == 5 and totals[2] == 2 and totals[3] == 2 and totals[4] == 0  # (block 2's unit meets the BLOCK range's bit)


def test_shortened_blocks():
    (case,) = shortened_cases()
    want, _ = check(case)
    assert bits_of(want.state(2), 0) == [3, 4, 5, 6, 7, 8]  # nd + m = 9: clipped
    assert bits_of(want.state(2), 2) == [1, 2, 3, 4]


def test_damaged_and_unreadable_messages():
    want, totals = check(damaged_case())
    assert totals[4] == 5 and totals[5] == 0  # all but the one with slack behind an item, and the good one
    _, totals = check(unreadable_case())
    assert totals[5] == 2 and totals[0] == 1
    check(count_dev_case())


def test_capacity():
    """one unit too few changes no byte of the state; totals[0], [4] and [5] are the full ones"""
    case = damaged_case()
    _, full = case.expected()
    units = int(full[0])
    before = case.sender().state()
    before.repair[0, 0] = 0x0F00
    state, totals = case.host(units - 1, before.clone())
    same_state(state, before)
    assert totals.tolist() == [units, 0, 0, 0, int(full[4]), int(full[5])]
    state, totals = case.host(units, case.sender().state())
    assert np.array_equal(totals, full)


def test_activation():
    k, m, nds, auto = 8, 4, [8, 6, 8, 0, 8], 1
    for word, block_repair in ((0, set()), (0, {1, 2, 3}), (R_INFO, {0}), (R_OBJECT, {2}), (R_OBJECT | R_INFO | P_INFO, set())):
        s = Sender(k, m, nds, auto)
        s.word, s.repair_mask = word, set(block_repair)
        s.blocks[0].pending_mask[:] = False                # sent out: a reset changes it
        s.blocks[1].pending_mask[:] = False
        s.blocks[1].repair_mask[[2, 7, 9]] = True          # segment repairs on a block that is also block-requested
        s.blocks[1].parity_offset, s.blocks[1].parity_count = 1, 2
        s.blocks[4].pending_mask[:] = False
        s.blocks[4].repair_mask[[0, 11]] = True
        state, pending = s.state(), s.pending()            # (block 2 still holds TxInit's bits: a reset without a change)
        totals = norm_amd.tx_activate_repairs_host(k, m, state, pending, np.array(nds, np.uint16), auto)
        want = s.activate()
        assert totals.tolist() == list(want), (word, block_repair, totals, want)
        same_state(state, s.state())
        assert np.array_equal(pending, s.pending())
    # the last state: the object bit resets every block, and nothing of the repair masks is activated
    assert s.word == P_INFO and not any(blk.repair_mask.any() for blk in s.blocks)
    assert s.blocks[4].pending_mask.tolist() == [True] * 9 + [False] * 3


def test_end_blocks():
    k, m, nds = 8, 4, [8, 8, 8, 9]
    s = Sender(k, m, nds)
    for blk, pair in zip(s.blocks, ((1, 2), (3, 3), (2, 1), (1, 1))):
        blk.pending_mask[:] = False
        blk.parity_offset, blk.parity_count = pair
    s.blocks[2].pending_mask[11] = True  # still pending: left alone
    state, pending = s.state(), s.pending()
    pending[0, 0] |= np.uint32(1 << 12)  # a bit past nd + m is ignored
    norm_amd.tx_end_blocks_host(k, m, state, pending, np.array(nds, np.uint16))
    s.end_blocks()
    same_state(state, s.state())
    assert state.parity.tolist() == [[3, 0], [4, 0], [2, 1], [1, 1]]  # clamped at m; nd outside [1, k] left alone
    again = state.clone()
    norm_amd.tx_end_blocks_host(k, m, again, pending, np.array(nds, np.uint16))
    same_state(again, state)


def test_parity_on_demand():
    """Three receivers miss 3, 5 and 2 different sources of one block: what becomes pending is five
    fresh parity segments, not the union of the ten named sources."""
    k, m, nb = 16, 8, 3
    rng = np.random.default_rng(5)
    lost = rng.permutation(k)[:10]
    missing = [lost[:3], lost[3:8], lost[8:]]
    messages = []
    for miss in missing:
        got = np.ones((nb, k + m), bool)
        got[1, miss] = False
        got[1, k:] = False  # the auto_parity is 0: no parity was sent
        content, _, totals = norm_amd.rx_repair_requests_host(k, m, to_words(got, [k] * nb, m), None, 5, 8, OBJ, 0)
        messages.append(bytes(content[:int(totals[0])]))
    case = Case(k, m, [k] * nb, messages)
    want, totals = check(case)
    state, _ = case.host()
    pending = np.zeros_like(state.repair)
    t = norm_amd.tx_activate_repairs_host(k, m, state, pending)
    assert t.tolist() == [0, 1, 5]
    bits = np.flatnonzero(np.unpackbits(pending[1].view(np.uint8), bitorder="little")).tolist()
    assert bits == list(range(k, k + 5)) and not pending[0].any() and not pending[2].any()
    assert state.parity.tolist() == [[0, 0], [0, 5], [0, 0]]


def test_argument_checks():
    L = N.lib()
    state = norm_amd.tx_repair_state(2, 8, 4)
    wire = np.frombuffer(seg_items(0, 8), np.uint8).copy()
    off, ln = np.zeros(1, np.uint64), np.array([wire.size], np.uint16)

    def handle(fec_id=5, fec_m=8, extra=0, k=8, m=4):
        try:
            norm_amd.tx_handle_nacks_host(k, m, state, wire, off, ln, None, fec_id, fec_m, OBJ, 0, extra)
        except norm_amd.NfecError as e:
            return e.code
        return 0

    assert handle() == 0
    assert handle(fec_id=0) == N.NFEC_EINVAL and handle(fec_id=2, fec_m=12) == N.NFEC_EINVAL
    assert handle(extra=65536) == N.NFEC_EINVAL and handle(extra=65535) == 0
    assert handle(k=40, m=30) == N.NFEC_EINVAL  # the stride of one word is too small
    assert handle(k=0) == N.NFEC_EINVAL
    with pytest.raises(norm_amd.NfecError):
        norm_amd.tx_activate_repairs_host(8, 4, state, np.zeros((2, 1), np.uint32), auto_parity=5)
    empty = norm_amd.tx_repair_state(0, 8, 4)
    assert norm_amd.tx_handle_nacks_host(8, 4, empty, wire, off, ln).tolist() == [0] * 6
    assert norm_amd.tx_handle_nacks_host(8, 4, state, wire, off[:0], ln[:0]).tolist() == [0] * 6
    assert all(name in N.declared_symbols() for name in (
        "nfec_tx_handle_nacks", "nfec_tx_nack_workspace_bytes", "nfec_tx_handle_nacks_host", "nfec_tx_activate_repairs",
        "nfec_tx_activate_repairs_host", "nfec_tx_end_blocks", "nfec_tx_end_blocks_host"))
    assert L.nfec_tx_nack_workspace_bytes(10, 1, 3) >= 10 * 16
