"""The host twins of the NORM_NACK / REPAIR_ADV message calls (norm_amd/csrc/ctl_msg_host.cpp, the
rule of ctl_msg.hpp): nfec_nack_fragment_host against two serial walks written here the way
NormSenderNode::FragmentNack is (reference src/common/normNode.cpp:2676-2772), one verbatim and one
with the two departures nfec.h states; the two headers field by field; nfec_adv_message_host against
the first message of the cut; nfec_ctl_parse_host on a table of datagrams.  CPU only."""
import ctypes
import struct

import numpy as np
import pytest

import norm_amd
from norm_amd import _native as N
from test_nack_host import PAIRS

ITEMS, RANGES = 1, 2
SIZES = (40, 44, 64, 104, 1400)
NACK = dict(source_id=0x0A0B0C0D, sender_id=0x11223344, instance_id=0x5566, first_sequence=65530, sequence_step=3,
            grtt_response=(0x01020304, 0x000F4241))
EXT = bytes(range(0xE0, 0xEC))


def item_length(fec_id):
    return 4 + N.lib().nfec_payload_id_length(fec_id)


def item(fec_id, fec_m, rng):
    n = N.lib().nfec_payload_id_length(fec_id)
    buf = (ctypes.c_uint8 * n)()
    assert N.lib().nfec_payload_id_write(fec_id, fec_m, int(rng.integers(0, 1 << 16)), int(rng.integers(0, 200)),
                                         int(rng.integers(1, 200)), buf) >= 0
    obj = int(rng.integers(0, 1 << 16))
    return bytes([fec_id, 0, obj >> 8, obj & 255]) + bytes(buf)


def build(table, fec_id, fec_m, rng):
    """table: (form, flags, units) per request -> the content's bytes and its requests as
    (form, flags, [unit bytes])."""
    out, reqs = bytearray(), []
    for form, flags, units in table:
        per = 2 if form == RANGES else 1
        us = [b"".join(item(fec_id, fec_m, rng) for _ in range(per)) for _ in range(units)]
        body = b"".join(us)
        out += bytes([form, flags]) + struct.pack(">H", len(body)) + body
        reqs.append((form, flags, us))
    return bytes(out), reqs


def pack(form, flags, units):
    body = b"".join(units)
    return bytes([form, flags]) + struct.pack(">H", len(body)) + body


def walk_verbatim(reqs, S):
    """FragmentNack as written: (messages, requests lost in its last arm, requests packed empty)."""
    msgs, cur, P, lost, empty = [], bytearray(), 0, 0, 0
    for form, flags, units in reqs:
        whole = pack(form, flags, units)
        if P + len(whole) <= S:
            cur += whole
            P += len(whole)
        elif P + 4 < S:
            P += 4
            mine = []
            for u in units:
                if P + len(u) > S:
                    empty += not mine
                    cur += pack(form, flags, mine)
                    msgs.append(bytes(cur))
                    cur, mine, P = bytearray(), [], 4
                mine.append(u)
                P += len(u)
            empty += not mine
            cur += pack(form, flags, mine)
        else:
            msgs.append(bytes(cur))
            cur, P = bytearray(), 0
            lost += 1
    if P:
        msgs.append(bytes(cur))
    return msgs, lost, empty


def walk_departed(reqs, S):
    """The rule of nfec.h: (messages, splits, times each arm was taken)."""
    msgs, cur, P, splits = [], bytearray(), 0, 0
    arms = {"A": 0, "B": 0, "C": 0}
    i = 0
    while i < len(reqs):
        form, flags, units = reqs[i]
        whole = pack(form, flags, units)
        U = len(units[0]) if units else 0
        if P + len(whole) <= S:
            arms["A"] += 1
            cur += whole
            P += len(whole)
        elif units and P + 4 + U <= S:
            arms["B"] += 1
            splits += 1
            P += 4
            mine = []
            for u in units:
                if P + len(u) > S:
                    cur += pack(form, flags, mine)
                    msgs.append(bytes(cur))
                    cur, mine, P = bytearray(), [], 4
                mine.append(u)
                P += len(u)
            cur += pack(form, flags, mine)
        else:
            arms["C"] += 1
            assert P, "arm C on an empty message would not advance"
            msgs.append(bytes(cur))
            cur, P = bytearray(), 0
            continue
        i += 1
    if P:
        msgs.append(bytes(cur))
    return msgs, splits, arms


def twin(content, S, fec_id, header=None, **kw):
    header = norm_amd.nack_header(**NACK) if header is None else header
    H = norm_amd.nack_header_bytes(header.ext_bytes)
    wire, offs, lens, totals = norm_amd.nack_fragment_host(np.frombuffer(content, np.uint8), header, S, fec_id=fec_id, **kw)
    n = min(int(totals[0]), offs.size)
    msgs = [bytes(wire[int(offs[i]) + H:int(offs[i]) + int(lens[i])]) for i in range(n)]
    heads = [bytes(wire[int(offs[i]):int(offs[i]) + H]) for i in range(n)]
    return msgs, heads, totals


def random_table(rng, S):
    n = int(rng.integers(1, 14))
    most = 5 if S <= 104 else 60
    return [(int(rng.choice((ITEMS, RANGES))), int(rng.integers(0, 8)), int(rng.integers(0, most + 1)) if rng.random() < 0.9 else 0)
            for _ in range(n)]


def units_of(fec_id, fec_m, content):
    flags, form, first, last, consumed = norm_amd.repair_parse_host(fec_id, fec_m, np.frombuffer(content, np.uint8))
    return list(zip(flags.tolist(), form.tolist(), map(tuple, first.tolist()), map(tuple, last.tolist()))), consumed


@pytest.mark.parametrize("fec_id,fec_m", PAIRS)
@pytest.mark.parametrize("S", SIZES)
def test_twin_equals_the_departed_walk_on_random_tables(fec_id, fec_m, S):
    rng = np.random.default_rng(1000 * S + 10 * fec_id + fec_m)
    L = item_length(fec_id)
    if S < 4 + 2 * L:
        with pytest.raises(norm_amd.NfecError):
            twin(b"", S, fec_id)
        return
    arms = {"A": 0, "B": 0, "C": 0}
    same_as_verbatim = 0
    for _ in range(150):
        content, reqs = build(random_table(rng, S), fec_id, fec_m, rng)
        want, splits, took = walk_departed(reqs, S)
        for a in arms:
            arms[a] += took[a]
        got, heads, totals = twin(content, S, fec_id)
        assert got == want
        assert totals.tolist() == [len(want), sum(map(len, want)), len(reqs), splits, len(content), 0]
        assert all(len(m) <= S and len(m) % 4 == 0 for m in got)
        # the messages, parsed one after the other, name the units of the content in its order
        assert units_of(fec_id, fec_m, b"".join(got))[0] == units_of(fec_id, fec_m, content)[0]
        verb, lost, empty = walk_verbatim(reqs, S)
        if not lost and not empty:
            same_as_verbatim += 1
            assert want == verb
    assert same_as_verbatim >= 10
    if S <= 104:
        assert min(arms.values()) >= 1, arms


def test_departure_1_the_request_that_did_not_fit_is_sent():
    rng = np.random.default_rng(1)
    content, reqs = build([(ITEMS, 1, 1)] * 4, 5, 8, rng)  # L = 8: three requests of 12 bytes, P = 36, S = 40
    verb, lost, empty = walk_verbatim(reqs, 40)
    assert lost == 1 and verb == [content[:36]]
    want, splits, arms = walk_departed(reqs, 40)
    assert want == [content[:36], content[36:]] and arms == {"A": 4, "B": 0, "C": 1}
    got, heads, totals = twin(content, 40, 5)
    assert got == want and totals.tolist() == [2, 48, 4, 0, 48, 0]


def test_departure_2_no_message_ends_with_an_empty_request():
    rng = np.random.default_rng(2)
    content, reqs = build([(ITEMS, 1, 1), (ITEMS, 1, 2), (ITEMS, 1, 2)], 5, 8, rng)  # P = 12 + 20 = 32, S = 40
    verb, lost, empty = walk_verbatim(reqs, 40)
    assert empty == 1 and verb[0] == content[:32] + bytes([ITEMS, 1, 0, 0])
    want, splits, arms = walk_departed(reqs, 40)
    assert want == [content[:32], content[32:]] and arms == {"A": 3, "B": 0, "C": 1}
    got, heads, totals = twin(content, 40, 5)
    assert got == want


def test_edges_exact_fit_long_ranges_and_zero_items():
    rng = np.random.default_rng(3)
    # exact fit: 12 + 28 = 40
    content, reqs = build([(ITEMS, 1, 1), (ITEMS, 2, 3)], 5, 8, rng)
    assert twin(content, 40, 5)[0] == [content]
    # one RANGES request longer than S: 4 + 5 * 16 = 84 bytes, two units a message
    content, reqs = build([(RANGES, 1, 5)], 5, 8, rng)
    got, heads, totals = twin(content, 40, 5)
    u = reqs[0][2]
    assert got == [pack(RANGES, 1, u[0:2]), pack(RANGES, 1, u[2:4]), pack(RANGES, 1, u[4:5])]
    assert totals.tolist() == [3, 92, 1, 1, 84, 0]
    # a request without items: copied where it fits, else the message is closed in front of it
    content, reqs = build([(ITEMS, 1, 0)], 5, 8, rng)
    assert twin(content, 40, 5)[0] == [content]
    content, reqs = build([(ITEMS, 1, 4), (ITEMS, 2, 0), (ITEMS, 4, 1)], 5, 8, rng)  # 36, then 4 fits: 40
    assert twin(content, 40, 5)[0] == [content[:40], content[40:]]
    content, reqs = build([(ITEMS, 1, 2), (ITEMS, 1, 2), (ITEMS, 2, 0), (ITEMS, 4, 1)], 5, 8, rng)  # P = 40, then arm C
    got, heads, totals = twin(content, 40, 5)
    assert got == walk_departed(reqs, 40)[0] == [content[:40], content[40:]]
    # nothing
    got, heads, totals = twin(b"", 40, 5)
    assert got == [] and totals.tolist() == [0, 0, 0, 0, 0, 0]


@pytest.mark.parametrize("tail,what", [(bytes([ITEMS, 1, 0, 16]) + bytes(8), "a length past the content"),
                                       (bytes([ITEMS, 1, 0, 12]) + bytes(12), "item bytes that are no multiple of L"),
                                       (bytes([RANGES, 1, 0, 24]) + bytes(24), "an odd item count in RANGES"),
                                       (bytes([ITEMS, 1]), "a header that does not fit")],
                         ids=["length", "multiple", "odd", "header"])
def test_the_walk_stops_at_a_malformed_tail_and_keeps_what_precedes_it(tail, what):
    rng = np.random.default_rng(4)
    good, reqs = build([(ITEMS, 1, 3), (RANGES, 1, 2), (ITEMS, 2, 2)], 5, 8, rng)
    want, splits, arms = walk_departed(reqs, 40)
    got, heads, totals = twin(good + tail, 40, 5)
    assert got == want, what
    assert totals.tolist() == [len(want), sum(map(len, want)), 3, splits, len(good), 1]
    if what[0] == "i" or what.startswith("an odd"):  # (bytes behind the other two tails would complete them)
        behind, reqs2 = build([(ITEMS, 1, 1)], 5, 8, rng)
        assert twin(good + tail + behind, 40, 5)[0] == want  # nothing behind the stop is read as a request


def test_arguments_capacity_and_pitch():
    rng = np.random.default_rng(5)
    content, reqs = build([(ITEMS, 1, 9), (RANGES, 1, 7)], 5, 8, rng)
    want = walk_departed(reqs, 40)[0]
    h = norm_amd.nack_header(**NACK)
    for S in (42, 16, 65512):  # no multiple of 4; below 4 + 2 L; S + H above 65535
        with pytest.raises(norm_amd.NfecError):
            norm_amd.nack_fragment_host(np.frombuffer(content, np.uint8), h, S)
    for pitch in (60, 66):  # below H + S; no multiple of 4
        with pytest.raises(norm_amd.NfecError):
            norm_amd.nack_fragment_host(np.frombuffer(content, np.uint8), h, 40, pitch=pitch)
    for bad in (1, 8, 16):
        with pytest.raises(norm_amd.NfecError):
            norm_amd.nack_header_bytes(bad)
        with pytest.raises(norm_amd.NfecError):
            norm_amd.adv_header_bytes(bad)
    assert (norm_amd.nack_header_bytes(0), norm_amd.nack_header_bytes(12)) == (24, 36)
    assert (norm_amd.adv_header_bytes(0), norm_amd.adv_header_bytes(12)) == (16, 28)
    # past capacity: the full totals, the first messages alone
    got, heads, totals = twin(content, 40, 5, capacity=2, pitch=76)
    assert got == want[:2] and int(totals[0]) == len(want) > 2 and int(totals[1]) == sum(map(len, want))


@pytest.mark.parametrize("ext", [None, EXT], ids=["base", "extension"])
def test_nack_header_fields(ext):
    rng = np.random.default_rng(6)
    content, reqs = build([(ITEMS, 1, 9), (RANGES, 1, 7)], 5, 8, rng)
    h = norm_amd.nack_header(ext=ext, **NACK)
    got, heads, totals = twin(content, 40, 5, header=h)
    H = 36 if ext else 24
    assert len(heads) > 3
    for i, b in enumerate(heads):
        assert len(b) == H and b == norm_amd.nack_header_write_host(h, i)
        assert b[0] == 0x14 and b[1] == H // 4
        assert struct.unpack(">H", b[2:4])[0] == (65530 + 3 * i) & 0xFFFF
        assert struct.unpack(">IIHH", b[4:16]) == (0x0A0B0C0D, 0x11223344, 0x5566, 0)
        assert struct.unpack(">II", b[16:24]) == (0x01020304, 0x000F4241)
        assert b[24:] == (ext or b"")
    # the reference's sequence: every NACK carries the same
    h0 = norm_amd.nack_header(1, 2, 3)
    assert all(b[2:4] == b"\0\0" for b in twin(content, 40, 5, header=h0)[1])


@pytest.mark.parametrize("ext", [None, EXT], ids=["base", "extension"])
def test_adv_message_is_the_header_and_the_first_message_of_the_cut(ext):
    rng = np.random.default_rng(7)
    h = norm_amd.adv_header(0x0A0B0C0D, 0x5566, sequence=0xBEEF, grtt=0x7A, backoff=4, gsize=3, ext=ext)
    H = 28 if ext else 16
    for table in ([(ITEMS, 1, 2)], [(ITEMS, 1, 2), (RANGES, 2, 1)], [(ITEMS, 1, 1), (ITEMS, 1, 2), (ITEMS, 1, 2)],
                  [(RANGES, 1, 5)], [(ITEMS, 1, 9), (RANGES, 1, 7)]):
        content, reqs = build(table, 5, 8, rng)
        first = walk_departed(reqs, 40)[0][0]
        fits = first == content
        msg, totals = norm_amd.adv_message_host(np.frombuffer(content, np.uint8), h, 40)
        assert msg[H:] == first == twin(content, 40, 5)[0][0]
        b = msg[:H]
        assert b[0] == 0x13 and b[1] == H // 4 and struct.unpack(">HIH", b[2:10]) == (0xBEEF, 0x0A0B0C0D, 0x5566)
        assert b[10] == 0x7A and b[11] == 0x43 and b[12] == 5 and b[13] == (0 if fits else 1) and b[14:16] == b"\0\0"
        assert b[16:] == (ext or b"")
        assert totals.tolist()[0] == len(first) and totals.tolist()[2] == (0 if fits else 1)
        assert (totals.tolist()[1] == 0) == fits
    msg, totals = norm_amd.adv_message_host(np.zeros(0, np.uint8), h, 40)
    assert msg == b"" and totals.tolist() == [0, 0, 0]


# ---- the intake's parse ----

SENDER, INSTANCE, LOCAL = 0x11223344, 0x5566, 0x0A0B0C0D


def nack_dgram(source=0x01010101, sender=SENDER, instance=INSTANCE, hdr_len=6, content=b"\1\1\0\0", ext=b"", sec=7, usec=9,
               vt=0x14):
    return bytes([vt, hdr_len]) + struct.pack(">HIIHHII", 5, source, sender, instance, 0, sec, usec) + ext + content


def adv_dgram(source=SENDER, instance=INSTANCE, hdr_len=4, flavor=5, content=b"\1\1\0\0", ext=b""):
    return bytes([0x13, hdr_len]) + struct.pack(">HIHBBBBH", 5, source, instance, 1, 2, flavor, 0, 0) + ext + content


def control_table():
    """(datagram bytes, class) for every class, both messages, with and without the extension."""
    C = N
    t = [(nack_dgram(), C.NFEC_CTL_NACK), (adv_dgram(), C.NFEC_CTL_REPAIR_ADV),
         (nack_dgram(hdr_len=9, ext=EXT), C.NFEC_CTL_NACK | C.NFEC_CTL_EXTENDED),
         (adv_dgram(hdr_len=7, ext=EXT), C.NFEC_CTL_REPAIR_ADV | C.NFEC_CTL_EXTENDED),
         (nack_dgram(content=b""), C.NFEC_CTL_NACK), (adv_dgram(content=b""), C.NFEC_CTL_REPAIR_ADV),
         (nack_dgram(vt=0x12), C.NFEC_CTL_OTHER_TYPE), (nack_dgram(vt=0x15), C.NFEC_CTL_OTHER_TYPE),
         (nack_dgram(hdr_len=5), C.NFEC_CTL_MALFORMED), (nack_dgram(hdr_len=8), C.NFEC_CTL_MALFORMED),
         (adv_dgram(hdr_len=3), C.NFEC_CTL_MALFORMED), (adv_dgram(hdr_len=6), C.NFEC_CTL_MALFORMED),
         (adv_dgram(hdr_len=3, flavor=4), C.NFEC_CTL_MALFORMED),
         (adv_dgram(flavor=4), C.NFEC_CTL_OTHER_FLAVOR), (adv_dgram(flavor=1), C.NFEC_CTL_OTHER_FLAVOR),
         (nack_dgram(source=LOCAL), C.NFEC_CTL_OWN), (adv_dgram(source=LOCAL), C.NFEC_CTL_OWN),
         (nack_dgram(sender=SENDER + 1), C.NFEC_CTL_OTHER_SENDER), (adv_dgram(source=SENDER + 1), C.NFEC_CTL_OTHER_SENDER),
         (nack_dgram(instance=INSTANCE + 1), C.NFEC_CTL_OTHER_INSTANCE),
         (adv_dgram(instance=INSTANCE + 1), C.NFEC_CTL_OTHER_INSTANCE)]
    # every length 0 .. 40 of a NACK with the extension and of an advertisement with it
    full_n, full_a = nack_dgram(hdr_len=9, ext=EXT), adv_dgram(hdr_len=7, ext=EXT)
    for n in range(41):
        cn = C.NFEC_CTL_UNREADABLE if n < 8 else C.NFEC_CTL_MALFORMED if n < 36 else C.NFEC_CTL_NACK | C.NFEC_CTL_EXTENDED
        ca = C.NFEC_CTL_UNREADABLE if n < 8 else C.NFEC_CTL_MALFORMED if n < 28 else C.NFEC_CTL_REPAIR_ADV | C.NFEC_CTL_EXTENDED
        t.append((full_n[:n], cn))
        t.append((full_a[:n], ca))
    return t


def lay_out(table, lead=0):
    """The datagrams back to back behind `lead` bytes: (wire, offsets, length)."""
    wire = bytearray(b"\xA5" * lead)
    offs, lens = [], []
    for d, _ in table:
        offs.append(len(wire))
        lens.append(len(d))
        wire += d
    return np.frombuffer(bytes(wire), np.uint8), np.array(offs, np.uint64), np.array(lens, np.uint16)


def expected_entries(table, offs, take):
    """content (offset, length) per datagram for the classes in `take`."""
    out = []
    for (d, cls), off in zip(table, offs.tolist()):
        out.append((off + 4 * d[1], len(d) - 4 * d[1]) if (cls & 0x7F) in take else (0, 0))
    return out


def test_ctl_parse_classes_entries_and_stats():
    table = control_table()
    wire, offs, lens = lay_out(table)
    f = norm_amd.ctl_filter(SENDER, INSTANCE, local_id=LOCAL, flags=N.NFEC_CTL_TAKE_NACK)
    cls, coff, clen, src, grtt, stats = norm_amd.ctl_parse_host(f, wire, offs, lens)
    assert cls.tolist() == [c for _, c in table]
    assert list(zip(coff.tolist(), clen.tolist())) == expected_entries(table, offs, {N.NFEC_CTL_NACK})
    assert stats.tolist() == [sum((c & 0x7F) == j for _, c in table) for j in range(9)] and min(stats.tolist()) >= 1
    for (d, c), s, g in zip(table, src.tolist(), grtt.tolist()):
        assert s == (struct.unpack(">I", d[4:8])[0] if len(d) >= 8 else 0)
        assert g == ([7, 9] if (c & 0x7F) == N.NFEC_CTL_NACK else [0, 0])
    # a receiver's intake takes the advertisements; both flags take both; none takes none
    for flags, take in ((N.NFEC_CTL_TAKE_ADV, {N.NFEC_CTL_REPAIR_ADV}),
                        (N.NFEC_CTL_TAKE_ADV | N.NFEC_CTL_TAKE_NACK, {N.NFEC_CTL_NACK, N.NFEC_CTL_REPAIR_ADV}), (0, set())):
        f = norm_amd.ctl_filter(SENDER, INSTANCE, local_id=LOCAL, flags=flags)
        cls2, coff, clen, _, _, _ = norm_amd.ctl_parse_host(f, wire, offs, lens)
        assert cls2.tolist() == cls.tolist()
        assert list(zip(coff.tolist(), clen.tolist())) == expected_entries(table, offs, take)
    # local_id 0 disables the own test; ANY_INSTANCE the instance test
    f = norm_amd.ctl_filter(SENDER, INSTANCE, local_id=0, flags=N.NFEC_CTL_ANY_INSTANCE)
    cls3 = norm_amd.ctl_parse_host(f, wire, offs, lens)[0].tolist()
    for (d, c), c3 in zip(table, cls3):
        if c == N.NFEC_CTL_OTHER_INSTANCE:
            assert c3 in (N.NFEC_CTL_NACK, N.NFEC_CTL_REPAIR_ADV)
        elif c == N.NFEC_CTL_OWN:
            # (the table's own NACK is for the filter's sender; its own advertisement is from LOCAL, not from it)
            assert c3 == (N.NFEC_CTL_NACK if d[0] == 0x14 else N.NFEC_CTL_OTHER_SENDER)
        else:
            assert c3 == c
    # an entry past the buffer is unreadable
    cls4 = norm_amd.ctl_parse_host(f, wire, np.array([wire.size - 10], np.uint64), np.array([11], np.uint16))[0]
    assert cls4.tolist() == [N.NFEC_CTL_UNREADABLE]
    with pytest.raises(norm_amd.NfecError):
        norm_amd.ctl_parse_host(norm_amd.ctl_filter(1, 2, flags=8), wire, offs, lens)


def test_an_entry_of_0_0_is_a_readable_empty_message_to_the_consumers():
    k, m, nb = 8, 4, 3
    st = norm_amd.tx_repair_state(nb, k, m)
    totals = norm_amd.tx_handle_nacks_host(k, m, st, np.zeros(16, np.uint8), np.zeros(3, np.uint64), np.zeros(3, np.uint16))
    assert totals.tolist() == [0, 0, 0, 0, 0, 0]  # [4] cut short, [5] unreadable
