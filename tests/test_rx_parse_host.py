"""Receiver intake, the part that needs no GPU: nfec_rx_parse_host, the parse half of nfec_rx_ingest's
rule (include/nfec.h, "receiver assembly on the device") on host arrays.  It runs the code the kernel
runs (norm_amd/csrc/rx_parse.hpp), so what is held here against oracle/wire_ref.py's restatement of
NormPayloadId (reference include/normMessage.h:396-567) and against nfec_payload_id_read holds for
the device path's decode too."""
import ctypes

import numpy as np
import pytest

import norm_amd
from norm_amd import NormDecoderRS8
from norm_amd import _native as N
from oracle import wire_ref as R

NEW = ("nfec_rx_ingest", "nfec_rx_parse_host")
FORMS = [(5, 8), (2, 8), (2, 16), (129, 8)]
BITS = {(5, 8): 24, (2, 8): 24, (2, 16): 16, (129, 8): 32}
SYMBOL_BITS = {(5, 8): 8, (2, 8): 8, (2, 16): 16, (129, 8): 16}
WRAPS = (0xFFFFFE, 0xFFFE, 0xFFFFFFFE)  # two below the wrap of the 24-, 16- and 32-bit block fields


def test_rx_intake_symbols_declared_exported_and_bound():
    declared = N.declared_symbols()
    L = N.lib()
    for name in NEW:
        assert name in declared, f"{name} not declared in include/nfec.h"
        assert hasattr(L, name), f"{name} not exported"
        assert name in N._SIGS, f"{name} missing from _SIGS"
    assert [f[0] for f in N.RxMessages._fields_] == ["payloads", "payload_bytes", "offsets", "length", "count",
                                                      "count_dev"]
    assert ctypes.sizeof(N.RxMessages) == 48 and N.RxMessages.count_dev.offset == 40
    assert hasattr(norm_amd, "rx_parse_host")
    assert hasattr(NormDecoderRS8, "ingest_messages") and hasattr(norm_amd.NormEncoderRS8, "ingest_messages")
    assert L.nfec_abi_version() == 1


def _read(fec_id, fec_m, raw):
    bid, sid, blen = ctypes.c_uint32(), ctypes.c_uint16(), ctypes.c_uint16()
    buf = np.frombuffer(bytes(raw), np.uint8)
    n = N.lib().nfec_payload_id_read(fec_id, fec_m, buf.ctypes.data, ctypes.byref(bid), ctypes.byref(sid),
                                     ctypes.byref(blen))
    assert n == len(raw)
    return bid.value, sid.value, blen.value


@pytest.mark.parametrize("fec_id,fec_m", FORMS)
@pytest.mark.parametrize("first", WRAPS)
def test_ids_at_every_alignment(fec_id, fec_m, first):
    """IDs that start at every residue of a 16-byte chunk (so every way an ID can straddle two
    chunks), block IDs on both sides of the block field's wrap"""
    rng = np.random.default_rng(fec_id * 7 + fec_m + first % 1000)
    bits, sbits = BITS[(fec_id, fec_m)], SYMBOL_BITS[(fec_id, fec_m)]
    field = (1 << bits) - 1
    idlen = N.lib().nfec_payload_id_length(fec_id)
    wire = rng.integers(1, 256, 64 * (15 + 8 + 8) + 16, dtype=np.uint8)  # 64 messages: gap, ID, payload
    offs, lens, sent = [], [], []
    at = 16
    for rep in range(4):
        for res in range(16):
            b = (rep * 16 + res) % 6  # blocks 0-5: block IDs first, first + 1 | wrap | first + 2 ...
            if rep == 3:
                b = int(rng.integers(0, min(field, 1 << 20)))  # and anywhere in the field
            s = int(rng.integers(0, 1 << sbits))
            bl = int(rng.integers(1, 1 << 16)) if fec_id == 129 else 0
            start = at + (res - at) % 16
            raw = R.payload_id(fec_id, fec_m, (first + b) & field, s, bl)
            assert len(raw) == idlen
            wire[start:start + idlen] = np.frombuffer(raw, np.uint8)
            offs.append(start + idlen)
            lens.append(int(rng.integers(0, 9)))
            sent.append((b, s, bl, raw))
            at = start + idlen + lens[-1]
    assert at <= wire.size and {(o - idlen) % 16 for o in offs} == set(range(16))
    blk, sym, blen = norm_amd.rx_parse_host(fec_id, fec_m, first, wire, np.array(offs, np.uint64),
                                            np.array(lens, np.uint16))
    assert blk.dtype == np.uint32 and sym.dtype == np.uint16 and blen.dtype == np.uint16
    for i, (b, s, bl, raw) in enumerate(sent):
        got = (int(blk[i]), int(sym[i]), int(blen[i]))
        assert got == (b, s, bl), (i, got, (b, s, bl))
        # the restatement's encoding of what was parsed is the bytes on the wire ...
        assert R.payload_id(fec_id, fec_m, (first + got[0]) & field, got[1], got[2]) == raw
        # ... and nfec_payload_id_read of the same bytes says the same
        bid, sid, rlen = _read(fec_id, fec_m, wire[offs[i] - idlen:offs[i]])
        assert ((bid - first) & field, sid, rlen) == got
    if first & field == field - 1:  # the window starts two below this field's wrap: both sides were sent
        assert {field - 1, field, 0, 1} <= {(first + b) & field for b, _, _, _ in sent}


def test_unreadable_messages():
    L = N.lib()
    wire = np.arange(1, 101, dtype=np.uint8)
    P = wire.size
    for fec_id, fec_m in FORMS:
        idlen = L.nfec_payload_id_length(fec_id)
        cases = [
            (idlen - 1, 0, False),      # off < idlen
            (0, 0, False),
            (idlen, 0, True),           # the first message a buffer can hold
            (idlen, P - idlen, True),   # ... filling it: off + len == wire_bytes
            (P - 10, 11, False),        # off + len one past wire_bytes
            (P - 10, 10, True),         # off + len == wire_bytes
            (P, 0, True),               # an empty payload at the very end
            (P + 1, 0, False),
            (1 << 63, 5, False),        # no sum that wraps
            ((1 << 64) - 1, 65535, False),
        ]
        off = np.array([c[0] for c in cases], np.uint64)
        ln = np.array([c[1] for c in cases], np.uint16)
        blk = np.full(len(cases), 7, np.uint32)
        sym = np.full(len(cases), 7, np.uint16)
        bl = np.full(len(cases), 7, np.uint16)
        n = L.nfec_rx_parse_host(fec_id, fec_m, 0, wire.ctypes.data, P, off.ctypes.data, ln.ctypes.data, len(cases),
                                 blk.ctypes.data, sym.ctypes.data, bl.ctypes.data)
        assert n == sum(c[2] for c in cases)
        for i, (o, _, ok) in enumerate(cases):
            if ok:
                bid, sid, rlen = _read(fec_id, fec_m, wire[o - idlen:o])
                assert (int(blk[i]), int(sym[i]), int(bl[i])) == (bid, sid, rlen), (fec_id, i)
            else:
                assert (int(blk[i]), int(sym[i]), int(bl[i])) == (0xFFFFFFFF, 0xFFFF, 0xFFFF), (fec_id, i)
        # every output may be NULL; the count is the same
        assert L.nfec_rx_parse_host(fec_id, fec_m, 0, wire.ctypes.data, P, off.ctypes.data, ln.ctypes.data, len(cases),
                                    None, None, None) == n


def test_refused_arguments():
    L = N.lib()
    wire = np.zeros(64, np.uint8)
    off = np.full(2, 16, np.uint64)
    ln = np.full(2, 4, np.uint16)
    blk = np.zeros(2, np.uint32)
    E = N.NFEC_EINVAL

    def call(fec_id=5, fec_m=8, w=wire.ctypes.data, o=off.ctypes.data, le=ln.ctypes.data, count=2):
        return L.nfec_rx_parse_host(fec_id, fec_m, 0, w, 64, o, le, count, blk.ctypes.data, None, None)

    assert call() == 2
    assert call(fec_id=0) == E and "fec_id" in N.last_error()   # a message without an ID names no slot
    assert call(fec_id=0, fec_m=0) == E
    assert call(fec_id=2, fec_m=12) == E and "fec_id" in N.last_error()
    assert call(fec_id=7) == E
    assert call(fec_id=2, fec_m=8) == 2 and call(fec_id=2, fec_m=16) == 2 and call(fec_id=129) == 2
    assert call(w=None) == E and "wire" in N.last_error()
    assert call(o=None) == E and "offsets" in N.last_error()
    assert call(le=None) == E and "length" in N.last_error()
    assert call(w=None, o=None, le=None, count=0) == 0
    assert call(fec_id=0, count=0) == E
    with pytest.raises(N.NfecError):
        norm_amd.rx_parse_host(2, 12, 0, wire, off, ln)
    with pytest.raises(ValueError):
        norm_amd.rx_parse_host(5, 8, 0, wire, off, ln[:1])


def test_device_entry_argument_checks_and_host_only_codec():
    """nfec_rx_ingest: null arrays, a short mask and a refused fec_id / fec_m pair are NFEC_EINVAL before
    the codec's device is looked at; a host-only codec answers NFEC_EDEVICE to well-formed calls"""
    dec = NormDecoderRS8(options=N.NFEC_OPT_HOST_ONLY)
    assert dec.Init(64, 32, 64)  # 96 slots: mask_stride >= 3
    L = N.lib()
    blk = np.zeros((2, 96, 64), np.uint8)
    b = N.BlockBatch()
    b.blocks, b.block_stride, b.seg_stride, b.nblocks = blk.ctypes.data, 96 * 64, 64, 2
    pay = np.zeros(256, np.uint8)
    off = np.full(2, 16, np.uint64)
    ln = np.full(2, 64, np.uint16)
    msg = N.RxMessages()
    msg.payloads, msg.payload_bytes = pay.ctypes.data, 256
    msg.offsets, msg.length, msg.count = off.ctypes.data, ln.ctypes.data, 2
    mask = np.zeros((2, 3), np.uint32)
    E, D = N.NFEC_EINVAL, N.NFEC_EDEVICE
    bb, mg, mp = ctypes.byref(b), ctypes.byref(msg), mask.ctypes.data

    def ingest(codec=dec._h, batch=bb, msgs=mg, fec_id=5, fec_m=8, received=mp, stride=3):
        return L.nfec_rx_ingest(codec, batch, msgs, fec_id, fec_m, 0, received, stride, None, None, None, None)

    assert ingest() == D and ingest(fec_id=2, fec_m=16) == D and ingest(fec_id=129) == D
    assert ingest(codec=None) == E and ingest(batch=None) == E and ingest(msgs=None) == E
    assert ingest(received=None) == E and "mask" in N.last_error()
    assert ingest(stride=2) == E and "mask_stride" in N.last_error()
    assert ingest(fec_id=0) == E and "fec_id" in N.last_error()
    assert ingest(fec_id=2, fec_m=12) == E and ingest(fec_id=7) == E
    for field in ("payloads", "offsets", "length"):
        saved = getattr(msg, field)
        setattr(msg, field, None)
        assert ingest() == E and field in N.last_error()
        setattr(msg, field, saved)
    assert not mask.any() and not blk.any()
