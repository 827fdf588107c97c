"""nfec_rx_handle_repair_content_host, nfec_rx_repair_pending_host (norm_amd/csrc/suppress_host.cpp) and
nfec_tx_repair_adv_host (norm_amd/csrc/nack_host.cpp), the rule of suppress_layout.hpp, against serial
walks written here the way the reference iterates: a receiver object whose held blocks carry
repair_mask / pending_mask / erasure_count, NormSenderNode::HandleRepairContent's loop
(src/common/normNode.cpp:1069-1187) with its freshObject / freshBlock caches, NormObject::
IsRepairPending (src/common/normObject.cpp:1137-1177) and NormBlock::IsRepairPending
(src/common/normSegment.cpp:174-216) with their preset-then-XCopy steps done literally, and
NormObject::AppendRepairAdv (normObject.cpp:540-683) / NormBlock::AppendRepairAdv
(normSegment.cpp:405-493) with their blockCount / segmentCount loops.  Then identities that a shared
misreading could not satisfy, and a model of the whole repair cycle on masks.  CPU only."""
import copy

import numpy as np
import pytest

import norm_amd
from norm_amd import _native as N
from test_nack_host import ABSENT, NEEDING, SILENT, Nack, block_class, block_with_runs, item_bytes, lossy, to_words
from test_txrepair_host import (BITS, BLOCK, INFO, ITEMS, OBJ, OBJECT, RANGES, SEGMENT, Case, block_range, corner_cases,
                                damaged_case, parse, request, seg_items, seg_range)

RX_OBJECT, RX_INFO = N.NFEC_RX_REPAIR_OBJECT, N.NFEC_RX_REPAIR_INFO
TX_OBJECT, TX_INFO = N.NFEC_TX_REPAIR_OBJECT, N.NFEC_TX_REPAIR_INFO
FECS = [(5, 8), (2, 8), (2, 16), (129, 8)]


# ---- the serial walk: the receiver ----

class RxBlock:
    """A NormBlock the receiver holds: pending = not received, over the block's nd + m slots."""

    def __init__(self, got, nd, m):
        self.nd, self.size = nd, nd + m
        self.pending_mask = ~np.asarray(got[:nd + m], bool)
        self.repair_mask = np.zeros(nd + m, bool)
        self.erasure_count = int(self.pending_mask[:nd].sum())

    def set_repairs(self, first, last):  # normSegment.h:216-222; the bits are clipped at the mask's size
        self.repair_mask[first:last + 1] = True

    def next_pending(self, s):
        while s < self.size and not self.pending_mask[s]:
            s += 1
        return s

    def is_repair_pending(self, num_data, num_parity):  # normSegment.cpp:174-216; destroys repair_mask
        if self.erasure_count > num_parity:
            if num_parity:
                i, next_id = num_parity, self.next_pending(0)
                while i:
                    i -= 1
                    self.repair_mask[next_id] = True  # a bit a parity segment can fill
                    next_id = self.next_pending(next_id + 1)
            elif self.size > num_data:
                self.repair_mask[num_data:self.size] = True
        else:
            self.repair_mask[:num_data] = True
            self.repair_mask[num_data + self.erasure_count:num_data + num_parity] = True
        self.repair_mask = self.pending_mask & ~self.repair_mask  # XCopy: pending_mask - repair_mask
        return bool(self.repair_mask.any())


class RxObject:
    """One object on a receiver.  A block is held exactly when it is needing: an absent block has no
    NormBlock, a complete or decodable one was decoded and released."""

    def __init__(self, k, m, got, nds, fec=(5, 8), first=0, object_id=OBJ):
        self.k, self.m, self.nds, self.fec, self.first, self.object_id = k, m, list(nds), fec, first, object_id
        self.cls = [block_class(got[b], nds[b], k, m) for b in range(len(nds))]
        self.blocks = {b: RxBlock(got[b], nds[b], m) for b, c in enumerate(self.cls) if c == NEEDING}
        self.pending_mask = {b for b, c in enumerate(self.cls) if c != SILENT}
        self.repair_mask = set()
        self.repair_info = False
        self.named = False  # rx_repair_mask.Test(object id)

    def block_of(self, block_id):
        return (block_id - self.first) & ((1 << BITS[self.fec]) - 1)

    def in_range(self, first, last):  # is this object one of first_obj .. last_obj (16-bit ids)?
        return ((self.object_id - first) & 0xFFFF) <= ((last - first) & 0xFFFF)

    def set_repairs(self, b0, b1):  # normObject.h:275-279, over the blocks of the call
        newly = 0
        if b0 <= b1 and b0 < len(self.nds):
            for b in range(b0, min(b1, len(self.nds) - 1) + 1):
                newly += b not in self.repair_mask
                self.repair_mask.add(b)
        return newly

    def handle_repair_content(self, units):
        """normNode.cpp:1069-1187 over the units of one message: (flags, first, last) with first / last
        = (obj, block id, block len, symbol).  Returns (SEGMENT units applied, units not applied or
        ignored, block bits newly set)."""
        applied = ignored = newly = 0
        fresh_object, prev_object_id, obj = True, 0, None
        fresh_block, prev_block_id, block = True, 0, None
        for flags, nxt, last in units:
            if flags & SEGMENT:
                level = SEGMENT
            elif flags & BLOCK:
                level = BLOCK
            elif flags & OBJECT:
                level = OBJECT
            elif flags & INFO:
                level = INFO
            else:
                ignored += 1  # (the reference asserts INFO here; a request without a level is skipped)
                continue
            repair_info = bool(flags & INFO)
            if level == INFO:  # :1131-1140
                if self.in_range(nxt[0], last[0]):
                    self.repair_info = True
                else:
                    ignored += 1
            elif level == OBJECT:  # :1141-1146
                if self.in_range(nxt[0], last[0]):
                    self.named = True
                else:
                    ignored += 1
            else:
                if nxt[0] != prev_object_id:
                    fresh_object = True
                if fresh_object:  # (the reference never clears the flag: a cache that always looks up)
                    obj = self if nxt[0] == self.object_id else None  # rx_table.Find
                    prev_object_id = nxt[0]
                if obj is None:
                    ignored += 1
                    continue
                if repair_info:
                    self.repair_info = True
                if level == BLOCK:  # :1147-1161
                    newly += self.set_repairs(self.block_of(nxt[1]), self.block_of(last[1]))
                    continue
                if nxt[1] != prev_block_id:  # :1173
                    fresh_block = True
                if fresh_block:
                    block = self.blocks.get(self.block_of(nxt[1]))  # FindBlock
                    prev_block_id = nxt[1]
                if block is not None and last[3] >= nxt[3]:
                    block.set_repairs(nxt[3], last[3])
                    applied += 1
                else:
                    ignored += 1
        return applied, ignored, newly

    def is_repair_pending(self, pending_info):  # normObject.cpp:1137-1177, flush; destroys the masks
        if pending_info and not self.repair_info:
            return True
        self.repair_mask = self.pending_mask - self.repair_mask  # XCopy
        for next_id in sorted(self.repair_mask):
            block = self.blocks.get(next_id)
            if block is not None:
                if block.is_repair_pending(self.nds[next_id], self.m):
                    return True
            else:
                return True  # the whole block is needed
        return False

    def decision(self, pending_info):
        """OnRepairTimeout (normNode.cpp:2362-2390) on copies: (send, the blocks that are pending,
        needing blocks suppressed, absent blocks suppressed)"""
        send = 0 if self.named else int(copy.deepcopy(self).is_repair_pending(pending_info))
        pending = []
        for b in sorted(self.pending_mask - self.repair_mask):
            block = copy.deepcopy(self.blocks.get(b))
            if block is None or block.is_repair_pending(self.nds[b], self.m):
                pending.append(b)
        needing = sum(1 for b in self.blocks if b not in pending)
        absent = sum(1 for b in self.pending_mask if b not in self.blocks and b not in pending)
        return send, pending, needing, absent

    def state(self, stride=None):
        stride = (self.k + self.m + 31) // 32 if stride is None else stride
        nb = len(self.nds)
        bits = np.zeros((nb, stride * 32), bool)
        for b, blk in self.blocks.items():
            bits[b, :blk.size] = blk.repair_mask
        rep = np.packbits(bits.reshape(nb, stride, 32), axis=2, bitorder="little").view(np.uint32).reshape(nb, stride)
        br = np.zeros(max(1, (nb + 31) // 32), np.uint32)
        for b in self.repair_mask:
            br[b >> 5] |= np.uint32(1 << (b & 31))
        word = (RX_OBJECT if self.named else 0) | (RX_INFO if self.repair_info else 0)
        return norm_amd.RxRepairState(rep, br, np.array([word], np.uint32))


def same_rx_state(a, b):
    for f in norm_amd.RxRepairState.FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        assert np.array_equal(x, y), (f, np.argwhere(x != y)[:4].tolist(), x.ravel()[:8], y.ravel()[:8])


def words_of(blocks, nb):
    out = np.zeros(max(1, (nb + 31) // 32), np.uint32)
    for b in blocks:
        out[b >> 5] |= np.uint32(1 << (b & 31))
    return out


class RxCase:
    """A receiver (reception mask `got`, bool [nb, k + m]) in front of a handle call whose messages are
    `case`'s (a test_txrepair_host.Case: the wire buffer, offsets, lengths, count, payload_bytes)."""

    def __init__(self, case, got, stride=None, rng=None):
        self.case, self.got, self.stride = case, np.asarray(got, bool), stride
        self.words = to_words(self.got, case.nds, case.m, stride, rng)

    def receiver(self):
        c = self.case
        return RxObject(c.k, c.m, self.got, c.nds, c.fec, c.first, OBJ)

    def expected(self):
        c, rx = self.case, self.receiver()
        totals = np.zeros(6, np.uint64)
        n = len(c.messages) if c.count is None else min(c.count, len(c.messages))
        for i in range(n):
            if not c.readable(i):
                totals[5] += 1
                continue
            o, ln = int(c.offsets[i]), int(c.lengths[i])
            units, cut = parse(c.fec, bytes(c.wire[o:o + ln]))
            a, g, w = rx.handle_repair_content(units)
            totals += np.array([len(units), a, g, w, cut, 0], np.uint64)
        return rx, totals

    def host(self, state=None):
        c = self.case
        state = norm_amd.rx_repair_state(len(c.nds), c.k, c.m, mask_stride=self.stride) if state is None else state
        keep = self.words.copy()
        totals = norm_amd.rx_handle_repair_content_host(c.k, c.m, state, self.words, c.wire, c.offsets, c.lengths,
                                                        np.array(c.nds, np.uint16), c.fec[0], c.fec[1], OBJ, c.first, c.count,
                                                        c.payload_bytes)
        assert np.array_equal(self.words, keep)
        return state, totals


def check_handle(rc):
    want, want_totals = rc.expected()
    got, totals = rc.host()
    assert np.array_equal(totals, want_totals), (rc.case.name, totals, want_totals)
    same_rx_state(got, want.state(rc.stride))
    return want, totals


def check_pending(k, m, got, nds, state, flags=0, stride=None, rng=None):
    """the host decision on (got, state) against the literal IsRepairPending on a receiver that holds
    the state's bits.  Returns (totals, the pending blocks)."""
    nb = len(nds)
    rx = RxObject(k, m, got, nds)
    bits = np.unpackbits(state.repair.view(np.uint8), axis=1, bitorder="little").astype(bool)
    for b, blk in rx.blocks.items():
        blk.repair_mask = bits[b, :blk.size].copy()
    rx.repair_mask = {b for b in range(nb) if (int(state.block_repair[b >> 5]) >> (b & 31)) & 1}
    rx.named, rx.repair_info = bool(state.object[0] & RX_OBJECT), bool(state.object[0] & RX_INFO)
    send, pending, needing, absent = rx.decision(bool(flags & N.NFEC_NACK_INFO))
    before = state.clone()
    totals, words = norm_amd.rx_repair_pending_host(k, m, state, to_words(got, nds, m, stride, rng), np.array(nds, np.uint16), flags)
    same_rx_state(state, before)  # only read
    assert totals.tolist() == [send, len(pending), needing, absent], (totals, send, pending, needing, absent)
    assert np.array_equal(words, words_of(pending, nb))
    return totals, pending


# ---- the serial walk: the sender's advertisement ----

def walk_adv(k, m, nds, repair, block_bits, word, fec, object_id, first, max_units):
    """repair: bool [nb, k + m], the blocks' repair masks; block_bits: NormObject::repair_mask.  The
    request bookkeeping (prevForm, AttachRepairRequest, PackRepairRequest) is test_nack_host.Nack's."""
    nb = len(nds)
    L = 4 + N.lib().nfec_payload_id_length(fec[0])
    start = np.zeros((nb + 1, 2), np.uint64)
    if word & TX_OBJECT:  # normSession.cpp:4602, :4662: one OBJECT request, never with INFO
        out = bytes([ITEMS, OBJECT, 0, L]) + item_bytes(fec[0], fec[1], object_id, 0, 0, k)
        start[nb] = (len(out), 1)
        return np.frombuffer(out, np.uint8), start, np.array([len(out), 1, 0, 0], np.uint64)
    held = [1 <= nd <= k for nd in nds]
    nack = Nack(fec[0], fec[1], object_id, first, bool(word & TX_INFO), max_units, nb)
    cls = [SILENT] * nb
    block_count, first_id = 0, 0
    for current in range(nb):  # normObject.cpp:577-660
        repair_entire_block = held[current] and current in block_bits
        if repair_entire_block:
            if not block_count:
                first_id = current
            block_count += 1
            cls[current] = ABSENT
        if block_count and (not repair_entire_block or current + 1 >= nb):  # a break in continuity, or the end
            last_id = current if repair_entire_block else current - 1
            nack.unit(last_id, BLOCK, block_count, (first_id, 0, nds[first_id]), (last_id, 0, nds[last_id]))
            block_count = 0
        if not repair_entire_block and held[current] and repair[current, :nds[current] + m].any():  # :640-658
            nack.pack()
            cls[current] = NEEDING
            bits, size, nd = repair[current], nds[current] + m, nds[current]

            def next_repair(s):
                while s < size and not bits[s]:
                    s += 1
                return s

            next_id, segment_count, first_seg = next_repair(0), 0, 0  # normSegment.cpp:418-483
            while next_id < size:
                current_id = next_id
                next_id = next_repair(next_id + 1)
                if not segment_count:
                    first_seg = current_id
                segment_count += 1
                if next_id - current_id > 1 or next_id >= size:
                    nack.unit(current, SEGMENT, segment_count, (current, first_seg, nd), (current, current_id, nd))
                    segment_count = 0
            nack.pack()
    nack.pack()
    if not nack.out and (word & TX_INFO) and nb:  # :670-681
        nack.out += bytes([ITEMS, INFO, 0, L]) + item_bytes(fec[0], fec[1], object_id, 0, 0, 0)
        nack.requests = 1
    start[1:, 0] = np.cumsum(nack.at[:nb])
    start[:nb, 1] = cls
    start[nb] = (len(nack.out), nack.requests)
    return (np.frombuffer(bytes(nack.out), np.uint8), start,
            np.array([len(nack.out), nack.requests, cls.count(NEEDING), cls.count(ABSENT)], np.uint64))


def tx_state(k, m, nds, repair, block_bits, word, stride=None, rng=None):
    st = norm_amd.tx_repair_state(len(nds), k, m, mask_stride=stride)
    st.repair[:] = to_words(repair, nds, m, stride, rng)
    st.block_repair[:] = words_of(block_bits, len(nds))
    st.object[0] = word
    return st


def check_adv(k, m, nds, repair, block_bits=(), word=0, fec=(5, 8), first=0, max_units=None, capacity=None, stride=None,
              rng=None):
    max_units = norm_amd.repair_max_units(fec[0]) if max_units is None else max_units
    want, w_start, w_totals = walk_adv(k, m, nds, np.asarray(repair, bool), set(block_bits), word, fec, OBJ, first, max_units)
    st = tx_state(k, m, nds, np.asarray(repair, bool), block_bits, word, stride, rng)
    before = st.clone()
    content, start, totals = norm_amd.tx_repair_adv_host(k, m, st, np.array(nds, np.uint16), fec[0], fec[1], OBJ, first,
                                                         max_units, capacity)
    for f in st.FIELDS:
        assert np.array_equal(getattr(st, f), getattr(before, f))
    assert np.array_equal(totals, w_totals), (totals, w_totals)
    assert np.array_equal(start, w_start)
    n = min(len(want), len(content))
    assert np.array_equal(content[:n], want[:n])
    assert not content[n:].any()
    return want, totals


# ---- content ----

def random_content(rng, nb, k, m, fec, first, messages):
    """requests of every level and form, own and foreign, some of them damaged"""
    kw = dict(fec=fec, first=first, nd=k)
    out = []
    for _ in range(messages):
        msg = b""
        for _ in range(int(rng.integers(0, 6))):
            r = rng.random()
            b = int(rng.integers(0, nb + 2))
            lo = int(rng.integers(0, k + m + 2))
            hi = lo + int(rng.integers(0, 5))
            flags = INFO if rng.random() < 0.2 else 0
            obj = OBJ if rng.random() < 0.85 else OBJ + 1
            if r < 0.45:
                msg += (request(ITEMS, SEGMENT | flags, [(obj, b, lo), (obj, (b + 1) % nb, hi % (k + m))], **kw) if rng.random() < 0.5
                        else request(RANGES, SEGMENT | flags, [(obj, b, lo), (obj, b, hi)], **kw))
            elif r < 0.7:
                msg += request(RANGES, BLOCK | flags, [(obj, b, 0), (obj, b + int(rng.integers(-1, 4)), 0)], **kw)
            elif r < 0.8:
                msg += request(ITEMS, BLOCK | flags, [(obj, b, 0)], **kw)
            elif r < 0.87:
                msg += request(RANGES, OBJECT | flags, [(obj - 1, 0, 0), (obj + int(rng.integers(0, 2)), 0, 0)], **kw)
            elif r < 0.94:
                msg += request(ITEMS, INFO, [(obj, 0, 0)], **kw)
            else:
                msg += request(ITEMS, 0, [(obj, b, lo)], **kw)
        d = rng.random()
        if d < 0.1 and len(msg) > 4:
            msg = msg[:-int(rng.integers(1, 4))]
        elif d < 0.15 and len(msg) > 4:
            msg = msg[:2] + b"\xff" + msg[3:]
        out.append(msg)
    return out


def random_reception(rng, nb, k, m, loss):
    got = lossy(rng, nb, k, m, loss)
    nds = [k if rng.random() < 0.5 else k - 1 for _ in range(nb)]
    for b in range(nb):
        r = rng.random()
        if r < 0.15:
            got[b] = False
        elif r < 0.3:
            got[b, :nds[b]] = True
        got[b, nds[b] + m:] = False
    nds[nb // 2] = 0 if nb > 2 else nds[nb // 2]
    if nb > 4:
        nds[nb // 3] = k + 1
    return got, nds


# ---- tests: the handler ----

@pytest.mark.parametrize("fec", FECS)
@pytest.mark.parametrize("k,m,nb", [(8, 4, 40), (62, 34, 9), (3, 2, 5)])
def test_handler_random_content(fec, k, m, nb):
    rng = np.random.default_rng(k * 100 + fec[0] + fec[1])
    first = (1 << BITS[fec]) - 3  # the window wraps the block field
    for trial in range(12):
        got, nds = random_reception(rng, nb, k, m, [0.2, 0.45, 0.7][trial % 3])
        case = Case(k, m, nds, random_content(rng, nb, k, m, fec, first, 6), fec=fec, first=first, align=trial % 4,
                    gap=(trial + 1) % 3, name=f"random {trial}")
        check_handle(RxCase(case, got, stride=(k + m + 31) // 32 + trial % 2, rng=rng))


@pytest.mark.parametrize("case", corner_cases(), ids=lambda c: c.name)
def test_handler_on_the_sender_tests_corner_contents(case):
    """the contents tests/test_txrepair_host.py feeds the sender, overheard by a receiver that needs
    every other block (e = 5 > m or e = 2) and holds nothing of block 0"""
    nb = len(case.nds)
    got = np.ones((nb, case.k + case.m), bool)
    for b in range(nb):
        got[b, :5 if b % 2 else 2] = False
        got[b, case.k:] = False
    got[0] = False
    check_handle(RxCase(case, got, stride=case.stride))


def test_handler_damaged_unreadable_and_count():
    want, totals = check_handle(RxCase(damaged_case(), np.zeros((3, 12), bool) | (np.arange(12) == 11)))
    assert totals[4] == 5 and totals[5] == 0
    c = Case(8, 4, [8, 8], [seg_items(0, 8), seg_items(1, 8, 9), seg_items(0, 9)], name="unreadable")
    c.offsets = np.array([c.offsets[0], c.wire.size - 4, 1 << 40], np.uint64)
    _, totals = check_handle(RxCase(c, np.zeros((2, 12), bool) | (np.arange(12) == 0)))
    assert totals[5] == 2 and totals[0] == 1 and totals[1] == 1
    c = Case(8, 4, [8, 8], [seg_items(0, 8), seg_items(1, 8, 9), seg_range(0, 0, 3)], name="count below count")
    c.count = 2
    _, totals = check_handle(RxCase(c, np.zeros((2, 12), bool) | (np.arange(12) == 0)))
    assert totals[0] == 3
    # a foreign fec_id and a foreign object: nothing is set
    c = Case(8, 4, [8], [request(ITEMS, SEGMENT, [(OBJ + 1, 0, 9)]), seg_items(0, 9, fec=(2, 8))], name="foreign")
    want, totals = check_handle(RxCase(c, np.zeros((1, 12), bool) | (np.arange(12) == 0)))
    assert totals.tolist() == [1, 0, 1, 0, 1, 0] and not want.state().repair.any()


def test_handler_levels_and_the_held_rule():
    k, m = 8, 4
    got = np.ones((5, k + m), bool)
    got[:, k:] = False
    got[0, :3] = False          # needing (e = 3)
    got[1] = False              # absent
    got[2, :1] = False          # needing (e = 1)
    got[3, 0] = False
    got[3, k] = True            # decodable: silent
    nds = [8, 8, 8, 8, 8]       # block 4 complete
    body = (request(RANGES, SEGMENT | INFO, [(1, 8), (1, 10)])     # absent: not applied, INFO still set
            + seg_range(0, 6, 200) + seg_items(3, 9) + seg_items(4, 9) + seg_items(2, 11)
            + request(RANGES, SEGMENT, [(0, 9), (0, 8)])           # backwards
            + request(ITEMS, OBJECT | INFO, [(OBJ + 1, 0, 0)]))    # another object
    want, totals = check_handle(RxCase(Case(k, m, nds, [body]), got))
    st = want.state()
    assert totals.tolist() == [7, 2, 5, 0, 0, 0]
    assert st.object[0] == RX_INFO and st.repair[:, 0].tolist() == [0xFC0, 0, 0x800, 0, 0]
    want, _ = check_handle(RxCase(Case(k, m, nds, [request(ITEMS, OBJECT | INFO, [(OBJ, 0, 0)])]), got))
    assert want.state().object[0] == RX_OBJECT  # the INFO flag of an OBJECT-level request is not looked at
    want, totals = check_handle(RxCase(Case(k, m, nds, [request(RANGES, BLOCK | INFO, [(3, 0), (900, 0)]) + block_range(4, 2)
                                                         + block_range(7, 9)]), got))
    assert want.state().block_repair[0] == 0x18 and totals[3] == 2 and want.state().object[0] == RX_INFO


def test_handler_order_and_splitting_do_not_matter():
    rng = np.random.default_rng(77)
    k, m, nb = 8, 4, 30
    got, nds = random_reception(rng, nb, k, m, 0.5)
    msgs = random_content(rng, nb, k, m, (5, 8), 0, 14)
    a, _ = RxCase(Case(k, m, nds, msgs), got).host()
    b, _ = RxCase(Case(k, m, nds, msgs[::-1], align=3), got).host()
    same_rx_state(a, b)
    c, _ = RxCase(Case(k, m, nds, msgs[5:]), got).host()
    c, _ = RxCase(Case(k, m, nds, msgs[:5]), got).host(c)
    same_rx_state(a, c)


# ---- tests: the decision ----

@pytest.mark.parametrize("k,m,nb", [(8, 4, 70), (60, 8, 12), (28, 8, 12), (3, 2, 33)])
def test_pending_random_states(k, m, nb):
    rng = np.random.default_rng(k + m)
    for trial in range(25):
        got, nds = random_reception(rng, nb, k, m, [0.15, 0.4, 0.6, 0.9][trial % 4])
        stride = (k + m + 31) // 32 + trial % 2
        st = norm_amd.rx_repair_state(nb, k, m, mask_stride=stride)
        rep = rng.random((nb, k + m)) < [0.1, 0.5, 0.9][trial % 3]
        if trial % 5 == 0:
            rep |= ~got  # everything that is missing was asked for
        st.repair[:] = to_words(rep, nds, m, stride, rng)
        st.block_repair[:] = words_of([b for b in range(nb) if rng.random() < 0.3], nb)
        st.object[0] = [0, RX_INFO, RX_OBJECT, RX_OBJECT | RX_INFO][trial % 4]
        check_pending(k, m, got, nds, st, flags=trial % 2, stride=stride, rng=rng)


def test_pending_e_against_m():
    """e < m, e == m and e > m: what has to be named for the block to fall silent"""
    k, m = 16, 4
    for e in (1, m - 1, m, m + 1, k):
        got = np.ones((1, k + m), bool)
        got[0, k:] = False
        got[0, 1:1 + e] = False
        want = set(range(k, k + e)) if e <= m else set(range(1 + m, 1 + e)) | set(range(k, k + m))
        for drop in [None] + sorted(want):
            rep = np.zeros((1, k + m), bool)
            rep[0, sorted(want - {drop})] = True
            st = norm_amd.rx_repair_state(1, k, m)
            st.repair[:] = to_words(rep, [k], m)
            totals, pending = check_pending(k, m, got, [k], st)
            assert pending == ([] if drop is None else [0]) and totals[2] == (drop is None)


def test_pending_slots_at_a_word_edge():
    k, m = 60, 8
    for slots in ([31], [32], [31, 32], [30, 31, 32], [31, 32, 33], [63], [64], [63, 64, 65]):
        got = block_with_runs(k, m, [(s, 1) for s in slots])[None, :]  # asks for exactly `slots`
        for missing in [None] + slots:
            rep = np.zeros((1, k + m), bool)
            rep[0, [s for s in slots if s != missing]] = True
            st = norm_amd.rx_repair_state(1, k, m)
            st.repair[:] = to_words(rep, [k], m)
            _, pending = check_pending(k, m, got, [k], st)
            assert pending == ([] if missing is None else [0])


# ---- tests: the advertisement ----

@pytest.mark.parametrize("fec", FECS)
@pytest.mark.parametrize("k,m,nb", [(8, 4, 40), (62, 34, 9), (200, 55, 5)])
def test_adv_random_states(fec, k, m, nb):
    if k + m > 256 and fec[1] == 8 and fec[0] != 129:
        fec = (2, 16)
    rng = np.random.default_rng(k + fec[0] * 7 + fec[1])
    first = (1 << BITS[fec]) - 3
    for trial in range(10):
        nds = [k if rng.random() < 0.5 else k - 1 for _ in range(nb)]
        nds[nb // 2] = [0, k + 1][trial % 2]
        repair = rng.random((nb, k + m)) < [0.02, 0.3, 0.7][trial % 3]
        repair[rng.random(nb) < 0.4] = False
        bits = [b for b in range(nb) if rng.random() < [0.1, 0.5][trial % 2]]
        word = [0, TX_INFO, N.NFEC_TX_PENDING_INFO, TX_INFO | N.NFEC_TX_PENDING_INFO][trial % 4]
        for max_units in (None, 1, 2):
            check_adv(k, m, nds, repair, bits, word, fec, first, max_units, stride=(k + m + 31) // 32 + trial % 2, rng=rng)


@pytest.mark.parametrize("length", [1, 2, 3])
def test_adv_runs_across_a_word_edge(length):
    k, m = 72, 8
    for edge in (32, 64):
        for back in range(length + 1):
            repair = np.zeros((2, k + m), bool)
            start = edge - back
            repair[0, start:start + length] = True
            repair[0, start + length + 1] = True
            repair[1, 79] = True  # the last slot of the block
            want, totals = check_adv(k, m, [k, k], repair)
            assert totals[2] == 2
    for bits in ([31], [31, 32], [30, 31, 32], [31, 32, 33, 35]):  # whole blocks across a block_repair word
        check_adv(8, 4, [8] * 40, np.zeros((40, 12), bool), bits)


def test_adv_object_info_and_capacity():
    k, m, nds = 8, 4, [8, 7, 8]
    repair = np.zeros((3, 12), bool)
    repair[1, [2, 9, 10]] = True
    for fec in FECS:
        want, totals = check_adv(k, m, nds, repair, [2], TX_OBJECT | TX_INFO, fec)
        L = 4 + N.lib().nfec_payload_id_length(fec[0])
        assert totals.tolist() == [4 + L, 1, 0, 0] and want[0] == ITEMS and want[1] == OBJECT
        units, cut = parse(fec, bytes(want))
        assert not cut and units == [(OBJECT, (OBJ, 0, k if fec[0] == 129 else 0, 0), (OBJ, 0, k if fec[0] == 129 else 0, 0))]
        want, totals = check_adv(k, m, nds, np.zeros((3, 12), bool), [], TX_INFO, fec)  # the INFO-only request
        assert totals.tolist() == [4 + L, 1, 0, 0] and want[1] == INFO
        want, totals = check_adv(k, m, nds, np.zeros((3, 12), bool), [], 0, fec)
        assert totals.tolist() == [0, 0, 0, 0]
    want, totals = check_adv(k, m, nds, repair, [2], TX_INFO)
    assert all(u[0] & INFO for u in parse((5, 8), bytes(want))[0])
    for cap in (0, 1, 3, 4, 5, len(want) // 2 + 1, len(want) - 1, len(want)):
        _, t = check_adv(k, m, nds, repair, [2], TX_INFO, capacity=cap)
        assert np.array_equal(t, totals)
    _, t = check_adv(k, m, nds, repair, [2], TX_OBJECT, capacity=5)
    assert t[0] == 12


# ---- identities ----

def nack_of(k, m, got, nds, flags=0, fec=(5, 8), first=0):
    content, _, totals = norm_amd.rx_repair_requests_host(k, m, to_words(got, nds, m), np.array(nds, np.uint16), fec[0], fec[1],
                                                          OBJ, first, flags)
    return bytes(content[:int(totals[0])]), totals


def overhear(k, m, got, nds, messages, fec=(5, 8), first=0, flags=0, state=None):
    """a receiver with reception `got` handles `messages` and decides: (totals, pending words, state)"""
    rc = RxCase(Case(k, m, nds, messages, fec=fec, first=first), got)
    state, _ = rc.host(state)
    totals, words = norm_amd.rx_repair_pending_host(k, m, state, rc.words, np.array(nds, np.uint16), flags)
    return totals, words, state


@pytest.mark.parametrize("fec", FECS)
@pytest.mark.parametrize("loss", [0.2, 0.45, 0.8])
def test_self_suppression(fec, loss):
    """B with A's reception handles A's NACK: it stays silent, and every needing and every absent
    block counts as suppressed (e <= m, e > m, absent runs; with and without NFEC_NACK_INFO)"""
    k, m, nb = 8, 4, 48
    rng = np.random.default_rng(int(loss * 100) + fec[0])
    first = (1 << BITS[fec]) - 5
    got, nds = random_reception(rng, nb, k, m, loss)
    for flags in (0, N.NFEC_NACK_INFO):
        content, t = nack_of(k, m, got, nds, flags, fec, first)
        assert t[2] > 0 and t[3] > 0
        totals, words, _ = overhear(k, m, got, nds, [content], fec, first, flags)
        assert totals.tolist() == [0, 0, int(t[2]), int(t[3])] and not words.any()
        # without having heard anything it sends, and for all of them
        totals, words, _ = overhear(k, m, got, nds, [], fec, first, flags)
        assert totals.tolist() == [1, int(t[2] + t[3]), 0, 0]


def test_no_false_suppression():
    """B misses one more source segment than A in one block: B sends, for exactly that block.  (One
    case is left out because the rule itself suppresses B there: both need at most m segments and
    the parity slot B would add to A's request, nd + e_A, has arrived, so B asks for what A asked.)"""
    k, m, nb = 8, 4, 48
    rng = np.random.default_rng(9)
    got, nds = random_reception(rng, nb, k, m, 0.45)
    content, t = nack_of(k, m, got, nds)
    rx = RxObject(k, m, got, nds)
    tried = 0
    for b in range(nb):
        nd = nds[b]
        have = [s for s in range(nd) if got[b, s]] if 1 <= nd <= k else []
        if not have:
            continue
        mine = got.copy()
        mine[b, have[-1]] = False
        if block_class(mine[b], nd, k, m) != NEEDING:
            continue
        e_b = int((~mine[b, :nd]).sum())
        if rx.cls[b] == NEEDING and e_b <= m and got[b, nd + e_b - 1]:
            continue
        totals, words, _ = overhear(k, m, mine, nds, [content])
        assert totals[0] == 1 and totals[1] == 1 and np.array_equal(words, words_of([b], nb)), (b, totals)
        tried += 1
    assert tried >= 10


@pytest.mark.parametrize("fec", FECS)
def test_adv_round_trip(fec):
    """a receiver that holds every block as needing handles the sender's advertisement: its repair
    and block_repair are the sender's over [0, nd + m), and INFO / OBJECT carry over"""
    k, m, nb = 8, 4, 70
    rng = np.random.default_rng(fec[0] + fec[1])
    first = (1 << BITS[fec]) - 33
    nds = [k if rng.random() < 0.5 else k - 1 for _ in range(nb)]
    got = np.zeros((nb, k + m), bool)
    got[:, 0] = True  # e = nd - 1 > p = 0: needing
    for word in (0, TX_INFO, TX_OBJECT, TX_OBJECT | TX_INFO):
        repair = rng.random((nb, k + m)) < 0.3
        repair[rng.random(nb) < 0.3] = False
        for b in range(nb):
            repair[b, nds[b] + m:] = False
        bits = [b for b in range(nb) if rng.random() < 0.3]
        st = tx_state(k, m, nds, repair, bits, word)
        content, _, totals = norm_amd.tx_repair_adv_host(k, m, st, np.array(nds, np.uint16), fec[0], fec[1], OBJ, first)
        _, _, rx = overhear(k, m, got, nds, [bytes(content[:int(totals[0])])], fec, first)
        if word & TX_OBJECT:
            assert rx.object[0] == RX_OBJECT and not rx.repair.any() and not rx.block_repair.any()
            continue
        assert rx.object[0] == (RX_INFO if word & TX_INFO else 0)
        assert np.array_equal(rx.block_repair, st.block_repair)
        want = st.repair.copy()
        want[bits] = 0  # a whole block's segment bits are not advertised
        assert np.array_equal(rx.repair, want)


# ---- the full cycle on masks ----

CYCLE = dict(k=8, m=4, nb=40, receivers=3, loss=0.45, seed=40, cap=60, fec=(5, 8), first=0xFFFFF0, object_id=7)


def cycle_model(k, m, nb, receivers, loss, seed, cap, fec, first, object_id, on_round=None):
    """One sender and `receivers` receivers on masks alone.  Each round: the sender lists and sends
    its pending slots, every receiver loses `loss` of them; decodable blocks are complete; then the
    receivers act in a drawn back-off order, each zeroing its state, handling the NACKs sent so far
    in the round and the sender's advertisement built behind them, deciding, and sending or not;
    then the sender activates.  Returns the rounds, each a dict of what a device run must repeat."""
    rng = np.random.default_rng(seed)
    nds = np.full(nb, k, np.uint16)
    tx = norm_amd.tx_repair_state(nb, k, m)
    pending = to_words(np.arange(k + m)[None, :].repeat(nb, 0) < k, [k] * nb, m)  # TxInit
    masks = [np.zeros((nb, (k + m + 31) // 32), np.uint32) for _ in range(receivers)]
    rounds = []
    while True:
        assert len(rounds) < cap, "the cycle is stuck"
        rec = dict(pending=pending.copy())
        _, blk, sym, _, start = norm_amd.tx_list_host(k, m, 64, pending)
        count = int(start[nb, 0])
        pending[:] = 0
        norm_amd.tx_end_blocks_host(k, m, tx, pending)
        rec["keep"] = [rng.random(count) >= loss for _ in range(receivers)]
        for r in range(receivers):
            for b, s in zip(blk[:count][rec["keep"][r]], sym[:count][rec["keep"][r]]):
                masks[r][b, s >> 5] |= np.uint32(1 << (s & 31))
            bits = np.unpackbits(masks[r].view(np.uint8), axis=1, bitorder="little")[:, :k + m].astype(int)
            done = (bits.sum(1) > 0) & (k - bits[:, :k].sum(1) <= bits[:, k:].sum(1))  # decodable: every source is there now
            masks[r][done, 0] |= np.uint32((1 << k) - 1)
        rec["masks"] = [x.copy() for x in masks]
        if all((x[:, 0] & ((1 << k) - 1) == (1 << k) - 1).all() for x in masks):
            rounds.append(rec)
            break
        rec["order"] = [int(r) for r in rng.permutation(receivers)]
        rec["decisions"], rec["pending_words"], rec["nacks"], rec["advs"] = {}, {}, [], []
        for r in rec["order"]:
            state = norm_amd.rx_repair_state(nb, k, m)
            heard = list(rec["nacks"])
            if heard:
                adv, _, t = norm_amd.tx_repair_adv_host(k, m, tx, nds, fec[0], fec[1], object_id, first)
                heard.append(bytes(adv[:int(t[0])]))
                rec["advs"].append(heard[-1])
            off = np.cumsum([0] + [len(x) for x in heard[:-1]]).astype(np.uint64) if heard else np.zeros(0, np.uint64)
            wire = np.frombuffer(b"".join(heard), np.uint8)
            norm_amd.rx_handle_repair_content_host(k, m, state, masks[r], wire, off, np.array([len(x) for x in heard], np.uint16),
                                                   nds, fec[0], fec[1], object_id, first)
            totals, words = norm_amd.rx_repair_pending_host(k, m, state, masks[r], nds)
            rec["decisions"][r], rec["pending_words"][r] = [int(x) for x in totals], words
            assert totals[0] == (totals[1] > 0)  # a receiver with a pending block sends
            if totals[0]:
                content, _, t = norm_amd.rx_repair_requests_host(k, m, masks[r], nds, fec[0], fec[1], object_id, first)
                content = bytes(content[:int(t[0])])
                rec["nacks"].append(content)
                ht = norm_amd.tx_handle_nacks_host(k, m, tx, np.frombuffer(content, np.uint8), np.zeros(1, np.uint64),
                                                   np.array([len(content)], np.uint16), nds, fec[0], fec[1], object_id, first)
                assert ht[4] == 0 and ht[5] == 0
        norm_amd.tx_activate_repairs_host(k, m, tx, pending, nds)
        rec["tx_state"] = tx.clone()
        rounds.append(rec)
        if on_round:
            on_round(rec)
    return rounds


def cycle_summary(rounds):
    nacks = sum(len(r.get("nacks", ())) for r in rounds)
    suppressed = sum(1 for r in rounds for d in r.get("decisions", {}).values() if d[0] == 0 and (d[2] or d[3]))
    return len(rounds), nacks, suppressed


def test_cycle_model_finishes_with_suppression():
    """Seed 40, chosen on the CPU so that the conditions below hold (a whole NACK is suppressed only
    when every block a receiver needs was asked for, which at 45 % independent loss is rare: 5 of
    the seeds 40 .. 298 have one).  Observed: 12 rounds (11 with a NACK phase), 24 NACKs sent of the
    33 three receivers could send, 3 NACKs suppressed."""
    rounds = cycle_model(**CYCLE)
    n, nacks, suppressed = cycle_summary(rounds)
    print(f"rounds {n}, NACKs {nacks}, suppressed {suppressed}")
    assert n <= CYCLE["cap"] and suppressed >= 1
    assert nacks < 3 * (n - 1)
    for r in rounds[:-1]:
        for d in r["decisions"].values():
            assert d[0] == 1 or d[1] == 0  # nobody with a pending block stayed silent
    assert (n, nacks, suppressed) == CYCLE_OBSERVED


CYCLE_OBSERVED = (12, 24, 3)  # rounds, NACKs sent, NACKs suppressed


# ---- arguments ----

def test_argument_checks():
    k, m = 8, 4
    got = np.zeros((2, 12), bool)
    wire = np.frombuffer(seg_items(0, 8), np.uint8).copy()
    off, ln = np.zeros(1, np.uint64), np.array([wire.size], np.uint16)
    words = to_words(got, [k, k], m)

    def code(fn, *a, **kw):
        try:
            fn(*a, **kw)
        except norm_amd.NfecError as e:
            return e.code
        return 0

    st = norm_amd.rx_repair_state(2, k, m)
    assert code(norm_amd.rx_handle_repair_content_host, k, m, st, words, wire, off, ln) == 0
    assert code(norm_amd.rx_handle_repair_content_host, k, m, st, words, wire, off, ln, fec_id=0) == N.NFEC_EINVAL
    assert code(norm_amd.rx_handle_repair_content_host, k, m, st, words, wire, off, ln, fec_id=2, fec_m=12) == N.NFEC_EINVAL
    assert code(norm_amd.rx_handle_repair_content_host, 0, m, st, words, wire, off, ln) == N.NFEC_EINVAL
    assert code(norm_amd.rx_handle_repair_content_host, 40, 30, st, words, wire, off, ln) == N.NFEC_EINVAL  # the stride
    assert code(norm_amd.rx_repair_pending_host, k, m, st, words, flags=2) == N.NFEC_EINVAL
    assert code(norm_amd.rx_repair_pending_host, 40, 30, st, words) == N.NFEC_EINVAL
    tx = norm_amd.tx_repair_state(2, k, m)
    assert code(norm_amd.tx_repair_adv_host, k, m, tx) == 0
    assert code(norm_amd.tx_repair_adv_host, k, m, tx, fec_id=0) == N.NFEC_EINVAL
    assert code(norm_amd.tx_repair_adv_host, k, m, tx, max_units=0) == N.NFEC_EINVAL
    assert code(norm_amd.tx_repair_adv_host, k, m, tx, max_units=65535 // 16 + 1) == N.NFEC_EINVAL
    assert code(norm_amd.tx_repair_adv_host, 40, 30, tx) == N.NFEC_EINVAL
    L = N.lib()
    s = st.struct()
    s.block_repair = None
    t = np.zeros(6, np.uint64)
    assert L.nfec_rx_repair_pending_host(k, m, words.ctypes.data, 1, None, 2, s, 0, None, t.ctypes.data) == N.NFEC_EINVAL
    assert L.nfec_rx_repair_pending_host(k, m, words.ctypes.data, 1, None, 2, st.struct(), 0, None, None) == N.NFEC_EINVAL
    assert L.nfec_rx_repair_pending_host(k, m, words.ctypes.data, 1, None, 2, st.struct(), 0, None, t.ctypes.data) == 0
    # nothing to do: zero totals
    empty = norm_amd.rx_repair_state(0, k, m)
    assert norm_amd.rx_handle_repair_content_host(k, m, empty, words[:0], wire, off, ln).tolist() == [0] * 6
    assert norm_amd.rx_handle_repair_content_host(k, m, st, words, wire, off[:0], ln[:0]).tolist() == [0] * 6
    assert norm_amd.rx_repair_pending_host(k, m, empty, words[:0], flags=1)[0].tolist() == [0] * 4
    assert norm_amd.tx_repair_adv_host(k, m, norm_amd.tx_repair_state(0, k, m))[2].tolist() == [0] * 4
    assert all(name in N.declared_symbols() for name in (
        "nfec_rx_handle_repair_content", "nfec_rx_handle_repair_content_host", "nfec_rx_repair_pending",
        "nfec_rx_repair_pending_host", "nfec_tx_repair_adv", "nfec_tx_repair_adv_host"))
