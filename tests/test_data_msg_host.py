"""Whole NORM_DATA messages: the header nfec_tx_emit_data writes and the parse nfec_rx_ingest_data
runs, through their host twins (nfec_data_header_write_host, nfec_rx_parse_data_host; the kernels run
the same code, norm_amd/csrc/data_msg.hpp).  CPU only.

The expected bytes come from a model written here from the reference's offsets:
  NormMsg        include/normMessage.h:688-696    byte 0 version << 4 | type (version 1, :26; DATA = 2,
                                                  :578), 1 hdr_len in words, 2-3 sequence, 4-7 source_id
  NormObjectMsg  :769-779                         8-9 instance_id, 10 grtt, 11 backoff << 4 | gsize,
                                                  12 flags (:727-737), 13 fec_id, 14-15 object id
  NormDataMsg    :1183-1186                       16 ... the FEC payload ID; extensions up to 4 hdr_len
                                                  (:612-616); then the payload (:636-637, :1127-1130)
and from oracle/wire_ref.py's payload_id / fti for the two fields it pins.  The classes follow
NormMsg::InitFromBuffer (src/common/normMessage.cpp:17-92): false for an unknown fec_id byte, for
msgLength < header_length and for header_length < 16 + idlen; a header_length equal to 16 + idlen and
a datagram that ends with its header (no payload) pass it, and are held here as the passing side of
those two bounds."""
import struct

import numpy as np
import pytest

import norm_amd
from norm_amd import _native as N
from oracle import wire_ref as R

FORMS = [(5, 8), (2, 8), (2, 16), (129, 8)]
IDLEN = {5: 4, 2: 4, 129: 8}
FTILEN = {5: 12, 2: 16, 129: 16}
BITS = {(5, 8): 24, (2, 8): 24, (2, 16): 16, (129, 8): 32}
SRC, INST, OBJ = 0xC0A80107, 0xBEEF, 0x8123
ONES = (0xFFFFFFFF, 0xFFFF, 0xFFFF)


def model_header(fec_id, fec_m, seq, block, symbol, block_len, ext=b"", source=SRC, instance=INST, obj=OBJ, grtt=0x9C,
                 backoff=5, gsize=3, flags=0x1A, mtype=2, hdr_len=None):
    pid = R.payload_id(fec_id, fec_m, block, symbol, block_len) if fec_id in IDLEN else b""
    n = 16 + len(pid) + len(ext)
    return struct.pack(">BBHIHBBBBH", (1 << 4) | mtype, n // 4 if hdr_len is None else hdr_len, seq & 0xFFFF, source,
                       instance, grtt, (backoff << 4) | gsize, flags, fec_id, obj) + pid + ext


def _fti(fec_id, fec_m, size=0x123456789A):
    return R.fti(fec_id, 1392, 64, 32, object_size=size, fec_m=fec_m)


def _filter(fec_id, fec_m, **kw):
    return norm_amd.data_filter(kw.get("source", SRC), kw.get("instance", INST), kw.get("obj", OBJ), fec_id, fec_m)


def _parse(fec_id, fec_m, datagrams, first=0, gap=3, tail=0, **kw):
    """the datagrams laid into one buffer, `gap` junk bytes in front of each, `tail` behind the last"""
    off, pos, parts = [], 0, []
    for d in datagrams:
        parts.append(b"\xEE" * gap)
        pos += gap
        off.append(pos)
        parts.append(d)
        pos += len(d)
    wire = np.frombuffer(b"".join(parts) + b"\xEE" * tail, np.uint8)
    ln = [len(d) for d in datagrams]
    return norm_amd.rx_parse_data_host(_filter(fec_id, fec_m, **kw), first, wire, np.array(off, np.uint64),
                                       np.array(ln, np.uint16)), off


def test_header_bytes_and_refusals():
    want = {(5, 0): 20, (2, 0): 20, (129, 0): 24, (5, 12): 32, (2, 16): 36, (129, 16): 40}
    for (fec_id, ext), n in want.items():
        assert norm_amd.data_header_bytes(fec_id, ext) == n
    for fec_id, ext in ((0, 0), (3, 0), (128, 0), (5, 16), (2, 12), (129, 12), (5, 4), (2, 8), (5, 13)):
        assert N.lib().nfec_data_header_bytes(fec_id, ext) == N.NFEC_EINVAL, (fec_id, ext)


@pytest.mark.parametrize("fec_id,fec_m", FORMS)
@pytest.mark.parametrize("with_fti", [False, True])
def test_header_equals_the_model(fec_id, fec_m, with_fti):
    ext = _fti(fec_id, fec_m) if with_fti else b""
    assert len(ext) == (FTILEN[fec_id] if with_fti else 0)
    cases = [  # first_sequence, i, grtt, backoff, gsize, flags, block, symbol, block_len
        (0, 0, 0, 0, 0, 0, 0, 0, 1),
        (65530, 5, 0x9C, 5, 3, 0x1A, 0xABCDEF, 0x7F, 64),    # sequence 65535
        (65530, 6, 0xFF, 15, 15, 0xFF, 0x123456, 200, 255),  # ... wraps to 0
        (65535, 65537, 1, 15, 0, 0x01, 0xFFFFFF, 0, 64),     # i itself past 2^16
        (7, 0xFFFFFFFF, 2, 0, 15, 0x80, 0x89ABCDEF, 0x1234 if fec_m == 16 or fec_id == 129 else 0x34, 0x0102),
    ]
    for first_seq, i, grtt, backoff, gsize, flags, block, symbol, block_len in cases:
        h = norm_amd.data_header(SRC, INST, OBJ, fec_id, fec_m, first_sequence=first_seq, grtt=grtt, backoff=backoff,
                                 gsize=gsize, flags=flags, fti=ext or None)
        got = norm_amd.data_header_write_host(h, i, block, symbol, block_len)
        field = (1 << BITS[(fec_id, fec_m)]) - 1
        want = model_header(fec_id, fec_m, first_seq + i, block & field, symbol, block_len, ext, grtt=grtt,
                            backoff=backoff, gsize=gsize, flags=flags)
        assert got == want, (first_seq, i, got.hex(), want.hex())
        assert len(got) == norm_amd.data_header_bytes(fec_id, len(ext)) and got[1] == len(got) // 4
        assert got[0] == 0x12 and got[11] == (backoff << 4 | gsize) and got[12] == flags
    seqs = [struct.unpack(">H", norm_amd.data_header_write_host(
        norm_amd.data_header(SRC, INST, OBJ, fec_id, fec_m, first_sequence=65534, fti=ext or None), i, 0, 0, 1)[2:4])[0]
        for i in range(4)]
    assert seqs == [65534, 65535, 0, 1]


def test_header_refusals():
    lib = N.lib()
    out = np.zeros(40, np.uint8)

    def rc(h, cap=40):
        return lib.nfec_data_header_write_host(h, 0, 0, 0, 1, out.ctypes.data, cap)

    good = norm_amd.data_header(SRC, INST, OBJ, 5, 8, fti=_fti(5, 8))
    assert rc(good) == 32 and rc(good, 31) == N.NFEC_EINVAL
    assert rc(norm_amd.data_header(SRC, INST, OBJ, 3, 8)) == N.NFEC_EINVAL
    assert rc(norm_amd.data_header(SRC, INST, OBJ, 2, 12)) == N.NFEC_EINVAL
    assert rc(norm_amd.data_header(SRC, INST, OBJ, 5, 8, fti=_fti(2, 8))) == N.NFEC_EINVAL  # 16 bytes on fec_id 5
    assert rc(norm_amd.data_header(SRC, INST, OBJ, 5, 8, backoff=16)) == N.NFEC_EINVAL
    assert rc(norm_amd.data_header(SRC, INST, OBJ, 5, 8, gsize=16)) == N.NFEC_EINVAL
    assert lib.nfec_data_header_write_host(None, 0, 0, 0, 1, out.ctypes.data, 40) == N.NFEC_EINVAL


@pytest.mark.parametrize("fec_id,fec_m", FORMS)
def test_one_datagram_per_class(fec_id, fec_m):
    idlen = IDLEN[fec_id]
    base = 16 + idlen
    pay = bytes(range(1, 12))
    ok = model_header(fec_id, fec_m, 77, 9, 3, 8) + pay
    other_code = 2 if fec_id != 2 else 5
    grams = [
        ok,                                                                    # 0 parsed
        ok[:7],                                                                # 1 unreadable: length < 8
        model_header(fec_id, fec_m, 78, 9, 3, 8, mtype=1) + pay,               # 2 INFO
        model_header(fec_id, fec_m, 79, 9, 3, 8, mtype=4)[:8],                 # 3 NACK, eight bytes
        model_header(fec_id, fec_m, 80, 9, 3, 8, source=SRC + 1) + pay,        # 4 other source
        model_header(fec_id, fec_m, 81, 9, 3, 8, instance=INST ^ 1) + pay,     # 5 other instance
        model_header(other_code, 8, 82, 9, 3, 8) + pay + b"\0" * 4,            # 6 other code (its own idlen)
        model_header(fec_id, fec_m, 83, 9, 3, 8, obj=OBJ + 1) + pay,           # 7 other object
        model_header(fec_id, fec_m, 84, 9, 3, 8, ext=_fti(fec_id, fec_m)),     # 8 parsed, FTI, no payload
    ]
    (cls, seq, blk, sym, blen, poff, plen, fti), off = _parse(fec_id, fec_m, grams)
    U, T, S, C, O, P = (N.NFEC_DGRAM_UNREADABLE, N.NFEC_DGRAM_OTHER_TYPE, N.NFEC_DGRAM_OTHER_SENDER,
                        N.NFEC_DGRAM_OTHER_CODE, N.NFEC_DGRAM_OTHER_OBJECT, N.NFEC_DGRAM_PARSED)
    assert cls.tolist() == [P, U, T, T, S, S, C, O, P]
    assert seq.tolist() == [77, 0, 78, 79, 80, 81, 82, 83, 84]
    for i in range(len(grams)):
        if cls[i] == P:
            assert (blk[i], sym[i]) == (9, 3) and blen[i] == (8 if fec_id == 129 else 0)
        else:
            assert (blk[i], sym[i], blen[i]) == ONES and (poff[i], plen[i]) == (0, 0)
    assert (poff[0], plen[0]) == (off[0] + base, len(pay))
    assert (poff[8], plen[8]) == (off[8] + len(grams[8]), 0)
    assert fti == 8
    # a datagram that ends one byte past the buffer is unreadable, whatever its bytes say
    (cls, *_), _ = _parse(fec_id, fec_m, [ok], tail=0)
    assert cls.tolist() == [P]
    wire = np.frombuffer(b"\xEE" * 3 + ok, np.uint8)
    cls2 = norm_amd.rx_parse_data_host(_filter(fec_id, fec_m), 0, wire[:-1], np.array([3], np.uint64),
                                       np.array([len(ok)], np.uint16))[0]
    assert cls2.tolist() == [U]
    cls3 = norm_amd.rx_parse_data_host(_filter(fec_id, fec_m), 0, wire, np.array([1 << 40], np.uint64),
                                       np.array([8], np.uint16))[0]
    assert cls3.tolist() == [U]


@pytest.mark.parametrize("fec_id,fec_m", FORMS)
def test_malformed_table(fec_id, fec_m):
    """InitFromBuffer's two bounds from both sides, and the fec_id bytes it does not know."""
    idlen = IDLEN[fec_id]
    base = 16 + idlen
    words = base // 4
    pay = bytes(range(1, 9))
    hdr = lambda **kw: model_header(fec_id, fec_m, 5, 2, 1, 8, **kw)  # noqa: E731
    grams = [
        hdr(hdr_len=words - 1) + pay,             # 0: 4 hdr_len one word below the base header
        hdr(hdr_len=words) + pay,                 # 1: equal to the base header: passes
        hdr(hdr_len=words + 3) + pay,             # 2: one word past the datagram (base + 8 bytes)
        hdr(hdr_len=words + 2) + pay,             # 3: ... and exactly the datagram: passes, no payload
        hdr(),                                    # 4: a datagram of exactly 16 + idlen bytes: passes, no payload
        hdr()[:base - 1],                         # 5: one byte short of its base header
        hdr()[:16],                               # 6: the base header without its ID
        hdr()[:12],                               # 7: byte 13 is not there
        model_header(0, 8, 5, 0, 0, 0) + b"\0" * 12,  # 8: fec_id byte 0
        model_header(3, 8, 5, 0, 0, 0) + b"\0" * 12,  # 9: fec_id byte 3
        hdr(hdr_len=0) + pay,                     # 10
        hdr(hdr_len=255) + pay,                   # 11
    ]
    (cls, seq, blk, sym, blen, poff, plen, fti), off = _parse(fec_id, fec_m, grams)
    M, P = N.NFEC_DGRAM_MALFORMED, N.NFEC_DGRAM_PARSED
    assert cls.tolist() == [M, P, M, P, P, M, M, M, M, M, M, M]
    assert (seq == 5).all()
    assert [int(x) for x in plen] == [0, 8, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]
    assert int(poff[1]) == off[1] + base and int(poff[3]) == off[3] + base + 8 and int(poff[4]) == off[4] + base
    assert fti is None


def test_class_order_when_several_conditions_hold():
    fec_id, fec_m = 5, 8
    pay = b"\x55" * 6
    U, T, M, S, C, O = (N.NFEC_DGRAM_UNREADABLE, N.NFEC_DGRAM_OTHER_TYPE, N.NFEC_DGRAM_MALFORMED,
                        N.NFEC_DGRAM_OTHER_SENDER, N.NFEC_DGRAM_OTHER_CODE, N.NFEC_DGRAM_OTHER_OBJECT)
    bad = dict(source=SRC ^ 7, obj=OBJ ^ 7)
    grams = [
        model_header(3, 8, 1, 0, 0, 0, mtype=3, hdr_len=1, **bad)[:7],        # everything wrong, and too short
        model_header(3, 8, 2, 0, 0, 0, mtype=3, hdr_len=1, **bad) + pay,      # other type before malformed
        model_header(3, 8, 3, 0, 0, 0, hdr_len=1, **bad) + pay,               # malformed before other sender
        model_header(2, 8, 4, 0, 0, 0, hdr_len=4, **bad) + pay,               # (a known code, a short header)
        model_header(2, 8, 5, 0, 0, 0, **bad) + pay,                          # other sender before other code
        model_header(2, 8, 6, 0, 0, 0, obj=OBJ ^ 7) + pay,                    # other code before other object
        model_header(129, 8, 7, 0, 0, 0, obj=OBJ ^ 7) + pay,                  # ... with the longer ID too
        model_header(5, 8, 8, 0, 0, 0, obj=OBJ ^ 7) + pay,
    ]
    (cls, seq, *_), _ = _parse(fec_id, fec_m, grams)
    assert cls.tolist() == [U, T, M, M, S, C, C, O]
    assert seq.tolist() == [0, 2, 3, 4, 5, 6, 7, 8]


@pytest.mark.parametrize("fec_id,fec_m", FORMS)
def test_first_extension_and_fti_index(fec_id, fec_m):
    idlen = IDLEN[fec_id]
    fti = _fti(fec_id, fec_m)
    unknown = bytes([1, 2]) + b"\xAA" * 6            # type 1, two words
    zero_len = bytes([64, 0]) + fti[2:]              # an FTI whose length byte is 0
    pay = b"\x33" * 5
    hdr = lambda ext, **kw: model_header(fec_id, fec_m, 9, 4, 2, 8, ext=ext, **kw)  # noqa: E731
    n_fti = (16 + idlen + len(fti)) // 4
    grams = [
        hdr(b"") + pay,                                         # 0 no extension
        hdr(unknown + fti) + pay,                               # 1 an unknown extension in front of an FTI
        hdr(zero_len) + pay,                                    # 2 length byte 0
        hdr(fti, hdr_len=n_fti - 1) + pay,                      # 3 the FTI runs past 4 hdr_len
        hdr(fti, obj=OBJ + 1) + pay,                            # 4 an FTI, but another object's
        hdr(fti) + pay,                                         # 5 the first that counts
        hdr(fti) + pay,                                         # 6
    ]
    (cls, seq, blk, sym, blen, poff, plen, idx), off = _parse(fec_id, fec_m, grams)
    P = N.NFEC_DGRAM_PARSED
    assert cls.tolist() == [P, P, P, P, N.NFEC_DGRAM_OTHER_OBJECT, P, P]
    assert idx == 5
    # the payload starts at 4 hdr_len whatever the extensions are
    assert int(poff[1]) == off[1] + 16 + idlen + 8 + len(fti) and plen[1] == len(pay)
    assert int(poff[3]) == off[3] + 4 * (n_fti - 1) and plen[3] == len(pay) + 4
    assert int(poff[5]) == off[5] + 16 + idlen + len(fti)
    # and nfec_fti_read finds the object's size where the index points
    out = N.Fti()
    at = off[idx] + 16 + idlen
    wire = b"".join(b"\xEE" * 3 + g for g in grams)
    ext = np.frombuffer(wire[at:at + len(fti)], np.uint8).copy()
    assert N.lib().nfec_fti_read(fec_id, ext.ctypes.data, ext.size, out) == len(fti)
    assert out.object_size == 0x123456789A
    # without datagrams 5 and 6 there is none
    assert _parse(fec_id, fec_m, grams[:5])[0][7] is None


@pytest.mark.parametrize("fec_id,fec_m", FORMS)
def test_block_field_wraps_against_first_block_id(fec_id, fec_m):
    bits = BITS[(fec_id, fec_m)]
    field = (1 << bits) - 1
    first = field - 1                      # block IDs field - 1, field, 0, 1, 2
    sym = 300 if bits != 24 else 200
    grams = [model_header(fec_id, fec_m, b, (first + b) & field, sym, 64) + b"\x01" for b in range(5)]
    for f in (first, first | (0xAB << bits if bits < 32 else 0)):  # only the field's bits of first_block_id count
        (cls, _, blk, s, blen, *_), _ = _parse(fec_id, fec_m, grams, first=f & 0xFFFFFFFF)
        assert (cls == N.NFEC_DGRAM_PARSED).all()
        assert blk.tolist() == [0, 1, 2, 3, 4] and (s == sym).all()
        assert (blen == (64 if fec_id == 129 else 0)).all()
    # a block in front of the window lands at the field's far end
    (_, _, blk, *_), _ = _parse(fec_id, fec_m, [model_header(fec_id, fec_m, 0, 4, 0, 64) + b"\x01"], first=5)
    assert blk.tolist() == [field]


def test_parse_refusals_and_empty():
    lib = N.lib()
    f = norm_amd.data_filter(SRC, INST, OBJ, 5, 8)
    assert norm_amd.rx_parse_data_host(f, 0, np.zeros(0, np.uint8), [], [])[7] is None
    one = np.zeros(1, np.uint64)
    ln = np.zeros(1, np.uint16)
    w = np.zeros(8, np.uint8)
    args = (0, w.ctypes.data, 8, one.ctypes.data, ln.ctypes.data, 1) + (None,) * 8
    assert lib.nfec_rx_parse_data_host(f, *args) == 0  # every output may be NULL
    assert lib.nfec_rx_parse_data_host(norm_amd.data_filter(SRC, INST, OBJ, 3, 8), *args) == N.NFEC_EINVAL
    assert lib.nfec_rx_parse_data_host(norm_amd.data_filter(SRC, INST, OBJ, 2, 12), *args) == N.NFEC_EINVAL
    assert lib.nfec_rx_parse_data_host(None, *args) == N.NFEC_EINVAL
    assert lib.nfec_rx_parse_data_host(f, 0, None, 8, one.ctypes.data, ln.ctypes.data, 1, *(None,) * 8) == N.NFEC_EINVAL
    assert lib.nfec_rx_parse_data_host(f, 0, w.ctypes.data, 8, None, ln.ctypes.data, 1, *(None,) * 8) == N.NFEC_EINVAL
    assert lib.nfec_rx_parse_data_host(f, 0, w.ctypes.data, 8, one.ctypes.data, None, 1, *(None,) * 8) == N.NFEC_EINVAL
    assert lib.nfec_rx_parse_data_host(f, 0, w.ctypes.data, 8, one.ctypes.data, ln.ctypes.data, 1 << 31,
                                       *(None,) * 8) == N.NFEC_ERANGE


@pytest.mark.parametrize("length", [8, 20, 24, 32, 40, 41, 56])
def test_chunk_rule(length):
    """Every load the intake makes of a datagram before it knows its class is an aligned 16-byte chunk
    that holds a byte of the datagram, and together they hold its first min(length, 28) bytes: the
    base header, the longest ID and the first word of the first extension."""
    for res in range(16):
        for base in (0, 4096, (1 << 40) + 4096 - 16):  # ... the last: a datagram that crosses a page
            at = base + res
            chunks = norm_amd.rx_data_chunks_host(at, length)
            assert 1 <= len(chunks) <= 3
            for c in chunks:
                assert c % 16 == 0
                assert c < at + length and c + 16 > at, (res, length, c)   # intersects [at, at + length)
            need = range(at, at + min(length, 28))
            assert all(any(c <= x < c + 16 for c in chunks) for x in need)
            assert chunks == sorted(set(chunks)) and chunks[-1] - chunks[0] == 16 * (len(chunks) - 1)
    for short in range(8):
        assert norm_amd.rx_data_chunks_host(5, short) == []
