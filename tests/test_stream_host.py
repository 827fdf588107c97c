"""Framing a NORM stream's writes into segments on the host: nfec_stream_frame_host.

The entry computes NormStreamObject::Write's segmentation (reference src/common/normObject.cpp:
4039-4232) in closed form (norm_amd/csrc/stream_layout.hpp, shared with the kernels).  It is held
here to a restatement of the reference's loop itself, line for line (:4166-4217): one open segment
with the three header fields, filled write by write, closed when full or flushed.  No GPU."""
import ctypes

import numpy as np
import pytest

import norm_amd
from norm_amd import _native as N
from norm_amd import NFEC_STREAM_EOM as EOM, NFEC_STREAM_FLUSH as FLUSH, StreamState, stream_frame_host

M32 = 0xFFFFFFFF


class RefStream:
    """NormStreamObject::Write's state and loop; closed segments are (payload_offset, payload_len,
    payload_msg_start) in the order their pending bits are set"""

    def __init__(self, segment_size, write_offset=0):
        self.segment_size = segment_size
        self.msg_start = True             # :2788
        self.write_offset = write_offset  # :2798 (0 there)
        self.segment = None               # the segment at write_index, once attached
        self.closed = []

    def write(self, length, eom, flush):
        n_bytes = 0
        while True:
            if self.segment is None:      # :4166-4169
                self.segment = {"msg_start": 0, "len": 0, "offset": self.write_offset}
            seg = self.segment
            index = seg["len"]            # :4172
            if self.msg_start and length != 0:  # :4175-4180
                if seg["msg_start"] == 0:
                    seg["msg_start"] = index + 1
                self.msg_start = False
            count = length - n_bytes      # :4182-4184
            space = self.segment_size - index
            count = min(count, space)
            seg["len"] = index + count    # :4193-4195
            n_bytes += count
            self.write_offset = (self.write_offset + count) & M32
            if count == space or (flush and n_bytes == length and (index != 0 or length != 0)):  # :4198-4199
                self.closed.append((seg["offset"], seg["len"], seg["msg_start"]))
                self.segment = None       # ++write_index.segment
            if not n_bytes < length:      # :4211
                break
        if eom:                           # :4214-4217
            self.msg_start = True

    def carry(self):
        seg = self.segment
        return (seg["len"], seg["msg_start"]) if seg else (0, 0)


def reference(S, lens, flags, write_offset=0):
    ref = RefStream(S, write_offset)
    for ln, fl in zip(lens, flags):
        ref.write(int(ln), bool(fl & EOM), bool(fl & FLUSH))
    return ref


def framed(S, lens, flags, state, capacity=None):
    """the entry's segments with the headers' absolute offsets, and its totals"""
    wo = state.write_offset
    start, ln, ms, totals = stream_frame_host(S, lens, flags, state, capacity)
    n = min(int(totals[0]), len(start))
    segs = [((wo + int(start[i])) & M32, int(ln[i]), int(ms[i])) for i in range(n)]
    return segs, totals, start


def check_against_reference(S, lens, flags, write_offset=0):
    ref = reference(S, lens, flags, write_offset)
    state = StreamState(write_offset=write_offset)
    segs, totals, start = framed(S, lens, flags, state)
    assert segs == ref.closed, (S, list(lens), list(flags))
    carry_len, carry_ms = ref.carry()
    assert totals.tolist() == [len(ref.closed), sum(s[1] for s in ref.closed), carry_len, carry_ms]
    assert state.as_tuple() == ((ref.write_offset - carry_len) & M32, int(ref.msg_start), carry_len, carry_ms,
                                len(ref.closed))
    # the segments tile the consumed bytes, and none is empty
    at = 0
    for i, (_, ln, ms) in enumerate(segs):
        assert int(start[i]) == at and 1 <= ln <= S and ms <= ln
        at += ln
    return segs


def random_writes(rng, S, n):
    kind = rng.integers(0, 6, n)
    lens = np.where(kind == 0, 0, np.where(kind == 1, S, np.where(kind == 2, rng.integers(0, 3 * S + 2, n),
                                                                   rng.integers(0, S + 2, n)))).astype(np.uint32)
    # (also lengths that complete the open segment exactly: kind 5, set below)
    flags = rng.choice([0, 0, 0, EOM, FLUSH, EOM | FLUSH], n).astype(np.uint8)
    fill = 0
    for i in range(n):
        if kind[i] == 5:
            lens[i] = (S - fill % S) % S or S
        fill += int(lens[i])
        if flags[i] & FLUSH:
            fill = 0
    return lens, flags


@pytest.mark.parametrize("S", [1, 2, 3, 7, 16])
def test_random_sequences_equal_the_reference_loop(S):
    rng = np.random.default_rng(100 + S)
    for _ in range(1500):
        n = int(rng.integers(0, 24))
        lens, flags = random_writes(rng, S, n)
        check_against_reference(S, lens, flags)


def test_named_corners():
    S = 7
    # zero-length writes with and without flush: on an empty and on an open segment
    assert check_against_reference(S, [0, 0, 3, 0, 0, 2], [0, FLUSH, 0, 0, FLUSH, 0]) == [(0, 3, 1)]
    assert check_against_reference(S, [0], [FLUSH]) == []
    assert check_against_reference(S, [3, 0, 0], [0, FLUSH, FLUSH]) == [(0, 3, 1)]
    # a write that ends exactly on a segment boundary, then a flush: no empty segment
    assert check_against_reference(S, [7, 0, 7, 1], [0, FLUSH, FLUSH, FLUSH]) == [(0, 7, 1), (7, 7, 0), (14, 1, 0)]
    assert check_against_reference(S, [4, 3, 0, 5], [0, 0, FLUSH, FLUSH]) == [(0, 7, 1), (7, 5, 0)]
    # EOM on a zero-length write starts a message at the next nonzero write; zero-length writes
    # between them leave the flag as it is
    assert check_against_reference(S, [2, 0, 0, 3, 9], [0, EOM, 0, 0, FLUSH]) == [(0, 7, 1), (7, 7, 0)]
    assert check_against_reference(S, [2, 0, 0, 3, 2], [0, EOM, 0, 0, FLUSH])[0] == (0, 7, 1)
    assert check_against_reference(S, [2, 2, 0, 3, 3], [FLUSH, 0, EOM | FLUSH, 0, FLUSH]) == [(0, 2, 1), (2, 2, 0), (4, 6, 1)]
    # only the first message start of a segment is recorded
    assert check_against_reference(S, [1, 2, 2, 9], [EOM, EOM, EOM, 0]) == [(0, 7, 1), (7, 7, 0)]
    assert check_against_reference(S, [9, 2, 2, 5], [EOM, EOM, EOM, FLUSH]) == [(0, 7, 1), (7, 7, 3), (14, 4, 0)]
    # segment_size 1
    assert check_against_reference(1, [3, 0, 1], [EOM, FLUSH, 0]) == [(0, 1, 1), (1, 1, 0), (2, 1, 0), (3, 1, 1)]
    # the largest segment_size
    top = 65535 - 8
    assert check_against_reference(top, [top + 1, top - 1], [EOM, 0]) == [(0, top, 1), (top, top, 2)]


def test_capacity_smaller_than_the_total():
    S = 5
    rng = np.random.default_rng(7)
    lens, flags = random_writes(rng, S, 40)
    ref = reference(S, lens, flags)
    total = len(ref.closed)
    assert total > 12
    for cap in (0, 1, total - 1, total, total + 3):
        state = StreamState()
        segs, totals, start = framed(S, lens, flags, state, cap)
        assert int(totals[0]) == total and len(start) == cap
        assert segs == ref.closed[:cap]
        assert state.next_slot == total  # the state moves by the full totals
        assert not start[total:].any()


def test_one_call_equals_any_split():
    rng = np.random.default_rng(11)
    for S in (1, 3, 7, 16):
        for _ in range(300):
            n = int(rng.integers(1, 30))
            lens, flags = random_writes(rng, S, n)
            whole_state = StreamState()
            whole, _, _ = framed(S, lens, flags, whole_state)
            cuts = sorted(set(rng.integers(0, n + 1, int(rng.integers(1, 5))).tolist()) | {0, n})
            state, parts = StreamState(), []
            for a, b in zip(cuts[:-1], cuts[1:]):
                before = state.next_slot
                segs, totals, _ = framed(S, lens[a:b], flags[a:b], state)
                assert state.next_slot == before + len(segs)
                parts += segs
            assert parts == whole, (S, lens.tolist(), flags.tolist(), cuts)
            assert state.as_tuple() == whole_state.as_tuple()


def test_offset_wraps_at_2_to_32():
    S = 16
    lens, flags = [10, 30, 0, 5, 40], [0, EOM, FLUSH, 0, EOM | FLUSH]
    base = (1 << 32) - 37
    segs = check_against_reference(S, lens, flags, write_offset=base)
    assert [s[0] for s in segs] == [(base + o) & M32 for o in (0, 16, 32, 40, 56, 72)]
    assert segs[-1][0] < 64 < base  # wrapped
    # and across calls: the state's offset wraps too
    state = StreamState(write_offset=base)
    a, _, _ = framed(S, lens[:2], flags[:2], state)
    assert state.write_offset == (base + 32) & M32 and state.carry_bytes == 8
    b, _, _ = framed(S, lens[2:], flags[2:], state)
    assert a + b == segs and state.write_offset == (base + 85) & M32


def test_invalid_arguments():
    L = N.lib()
    lens = np.array([3, 4], np.uint32)
    flags = np.array([0, FLUSH], np.uint8)
    out = (np.zeros(4, np.uint64), np.zeros(4, np.uint16), np.zeros(4, np.uint16))
    totals = np.zeros(4, np.uint64)

    def call(S=8, wl=lens.ctypes.data, wf=flags.ctypes.data, n=2, state=None, o0=out[0].ctypes.data,
             o1=out[1].ctypes.data, o2=out[2].ctypes.data, cap=4, t=totals.ctypes.data, null_state=False):
        st = state or StreamState()
        return L.nfec_stream_frame_host(S, wl, wf, n, None if null_state else ctypes.byref(st), o0, o1, o2, cap, t)

    E = N.NFEC_EINVAL
    assert call() == N.NFEC_OK
    assert call(S=0) == E and call(S=65535 - 7) == E and call(S=65535 - 8) == N.NFEC_OK
    assert call(wl=None) == E and call(wf=None) == E and call(null_state=True) == E and call(t=None) == E
    assert call(o0=None) == E and call(o1=None) == E and call(o2=None) == E
    assert call(o0=None, o1=None, o2=None, cap=0) == N.NFEC_OK      # a counting call
    assert call(wl=None, wf=None, n=0) == N.NFEC_OK                 # no writes
    assert call(state=StreamState(carry_bytes=8)) == E              # a carry is an open segment
    assert call(state=StreamState(carry_bytes=3, carry_msg_start=5)) == E
    assert call(state=StreamState(carry_bytes=7, carry_msg_start=7)) == N.NFEC_OK


def test_symbols_are_declared_and_bound():
    names = ["nfec_stream_frame_host", "nfec_stream_frame", "nfec_stream_pack", "nfec_stream_unpack"]
    declared = N.declared_symbols()
    for name in names:
        assert name in declared and name in N._SIGS
        assert getattr(N.lib(), name) is not None
    for cls in (norm_amd.NormEncoderRS8, norm_amd.NormDecoderRS16):
        for method in ("frame_stream", "pack_stream", "unpack_stream"):
            assert callable(getattr(cls, method))
    assert ctypes.sizeof(N.StreamState) == 24 and ctypes.sizeof(N.StreamSegments) == 56
    assert (N.NFEC_STREAM_EOM, N.NFEC_STREAM_FLUSH, N.NFEC_STREAM_END) == (1, 2, 1)
    assert StreamState().as_tuple() == (0, 1, 0, 0, 0)
