"""NORM_NACK and NORM_CMD(REPAIR_ADV) messages on the device: nfec_nack_fragment,
nfec_tx_repair_adv_message and nfec_rx_ingest_control (norm_amd/csrc/kernels_ctlmsg.hip) against the
host twins on the same bytes (themselves held to two serial walks of FragmentNack and to the header
layouts in tests/test_ctl_msg_host.py): every byte of the wire buffer, canaries included, the datagram
tables and the totals.  Then the closed loop of test_gpu_txrepair.py with the NACK leg in HBM:
repair_requests -> nack_messages -> ingest_control -> handle_nacks, three receivers' datagrams
interleaved in one buffer, the host route alongside on host state.

Shapes: S in {40, 44, 64} puts a cut every few requests (every arm of the rule, messages of one to
five units); 300 blocks at 45 % loss give some 2,000 requests in 300 stretches of the hint, more rows
than one 256-lane workgroup of the walk and several anchors of 64 messages at S = 104; 5,000
alternating blocks give one stretch that a single lane walks."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import norm_amd  # noqa: E402
from norm_amd import _native as N  # noqa: E402
from norm_amd import NormDecoderRS8, NormEncoderRS8  # noqa: E402
from test_ctl_msg_host import (EXT, INSTANCE, ITEMS, LOCAL, NACK, RANGES, SENDER, build, control_table, lay_out,  # noqa: E402
                               random_table, walk_departed)
from test_gpu_tx import _dev, _np  # noqa: E402
from test_suppress_host import same_rx_state  # noqa: E402
from test_txrepair_host import Sender, same_state  # noqa: E402

CANARY = 0xA5
_CODEC = {}


def codec():
    if "enc" not in _CODEC:
        enc, dec = NormEncoderRS8(), NormDecoderRS8()
        assert enc.Init(64, 32, 1400) and dec.Init(64, 32, 1400)
        _CODEC["enc"], _CODEC["dec"] = enc, dec
    return _CODEC["enc"], _CODEC["dec"]


def bytes_dev(content):
    """content bytes as (uint8 tensor of at least 4 bytes, its length as the int64 tensor a producer leaves)"""
    c = np.frombuffer(bytes(content), np.uint8)
    t = torch.zeros(max(c.size, 4), dtype=torch.uint8, device="cuda")
    t[:c.size] = torch.from_numpy(c.copy()).cuda()
    return t, torch.tensor([c.size], dtype=torch.int64, device="cuda")


def fragment_both(content, S, fec_id, header, capacity, pitch, block_start=None, content_dev=None):
    """(device wire, offsets, lengths, totals) and the host twin's, both on a canary-filled wire buffer
    that holds capacity + 1 messages' room"""
    dec = codec()[1]
    cd, nbytes = bytes_dev(content) if content_dev is None else content_dev
    wire = torch.full(((capacity + 1) * pitch,), CANARY, dtype=torch.uint8, device="cuda")
    _, offs, lens, totals = dec.nack_messages(cd, nbytes, header, S, fec_id=fec_id, block_start=block_start, wire=wire,
                                              pitch=pitch, capacity=capacity)
    h_wire, h_offs, h_lens, h_totals = norm_amd.nack_fragment_host(np.frombuffer(bytes(content), np.uint8), header, S,
                                                                   fec_id=fec_id, pitch=pitch, capacity=capacity)
    want = np.full((capacity + 1) * pitch, CANARY, np.uint8)
    for i in range(min(int(h_totals[0]), capacity)):
        o, n = int(h_offs[i]), int(h_lens[i])
        want[o:o + n] = h_wire[o:o + n]
    torch.cuda.synchronize()
    return (wire.cpu().numpy(), _np(offs, np.uint64), _np(lens, np.uint16), _np(totals, np.uint64)), (want, h_offs, h_lens, h_totals)


def assert_same(got, want, what=None):
    for g, w, name in zip(got, want, ("wire", "offsets", "lengths", "totals")):
        assert np.array_equal(g, w), (what, name, np.argwhere(g != w)[:4].tolist(), g[:8], w[:8])


HAND = [[(ITEMS, 1, 1)] * 4, [(ITEMS, 1, 1), (ITEMS, 1, 2), (ITEMS, 1, 2)], [(ITEMS, 1, 1), (ITEMS, 2, 3)], [(RANGES, 1, 5)],
        [(ITEMS, 1, 0)], [(ITEMS, 1, 4), (ITEMS, 2, 0), (ITEMS, 4, 1)], [(ITEMS, 1, 2), (ITEMS, 1, 2), (ITEMS, 2, 0), (ITEMS, 4, 1)], []]


@pytest.mark.parametrize("fec_id,fec_m", [(5, 8), (129, 16)])
@pytest.mark.parametrize("S", [40, 44, 64])
def test_hand_cases_and_random_tables_equal_the_host_twin(fec_id, fec_m, S):
    rng = np.random.default_rng(77 * S + fec_id)
    header = norm_amd.nack_header(ext=EXT if S == 44 else None, **NACK)
    H = norm_amd.nack_header_bytes(header.ext_bytes)
    pitch = H + S + 12
    tables = HAND + [random_table(rng, S) for _ in range(34)]  # 6 * 34 = 204 random tables over the cases
    short = 0
    for t, table in enumerate(tables):
        content, reqs = build(table, fec_id, fec_m, rng)
        messages = len(walk_departed(reqs, S)[0])
        got, want = fragment_both(content, S, fec_id, header, messages + 1, pitch)
        assert_same(got, want, table)
        assert int(got[3][0]) == messages
        if messages >= 2 and t % 3 == 0:  # a capacity below the message count: the full totals, nothing past it
            short += 1
            got, want = fragment_both(content, S, fec_id, header, messages - 1, pitch)
            assert_same(got, want, table)
            assert int(got[3][0]) == messages and (got[0][(messages - 1) * pitch:] == CANARY).all()
    assert short >= 5


def malformed_tails():
    return [bytes([ITEMS, 1, 0, 16]) + bytes(8), bytes([ITEMS, 1, 0, 12]) + bytes(12), bytes([RANGES, 1, 0, 24]) + bytes(24),
            bytes([ITEMS, 1]), bytes([ITEMS, 1, 0, 8])]


def test_malformed_content_stops_the_walk_as_on_the_host():
    rng = np.random.default_rng(5)
    header = norm_amd.nack_header(**NACK)
    good, reqs = build([(ITEMS, 1, 3), (RANGES, 1, 2), (ITEMS, 2, 2)], 5, 8, rng)
    for tail in malformed_tails():
        got, want = fragment_both(good + tail, 40, 5, header, 8, 76)
        assert_same(got, want, tail)
        assert got[3].tolist()[4:] == [len(good), 1]
    # content cut at content_capacity: what the buffer holds is cut, and the call says so
    dec = codec()[1]
    cd, _ = bytes_dev(good)
    more = torch.tensor([len(good) + 40], dtype=torch.int64, device="cuda")
    _, _, _, totals = dec.nack_messages(cd, more, header, 40, capacity=8)
    want = walk_departed(reqs, 40)
    assert _np(totals, np.uint64).tolist() == [len(want[0]), sum(map(len, want[0])), 3, want[1], len(good), 1]


def random_masks(rng, nb, k, m, loss):
    bits = rng.random((nb, 32 * ((k + m + 31) // 32))) >= loss
    bits[:, k + m:] = False
    return np.packbits(bits, axis=1, bitorder="little").view(np.uint32)


@pytest.mark.parametrize("S", [104, 1400])
def test_content_of_repair_requests_with_and_without_the_hint(S):
    k, m, nb = 64, 32, 300
    dec = codec()[1]
    rng = np.random.default_rng(45)
    masks = _dev(random_masks(rng, nb, k, m, 0.45))
    content, block_start, totals = dec.repair_requests(masks, fec_id=5, fec_m=8, object_id=7, first_block_id=0xFFFF00)
    nbytes = int(_np(totals, np.uint64)[0])
    assert int(_np(block_start, np.uint64)[:nb, 1].tolist().count(1)) > 256  # more stretches than one workgroup's lanes
    host = content.cpu().numpy()[:nbytes]
    header = norm_amd.nack_header(**NACK)
    pitch = 24 + S
    cap = nbytes // (S - 32) + 8  # (a message that is not the last holds more than S - 4 - 16 bytes)
    hinted, want = fragment_both(host, S, 5, header, cap, pitch, block_start=block_start, content_dev=(content, totals[:1]))
    plain, _ = fragment_both(host, S, 5, header, cap, pitch, content_dev=(content, totals[:1]))
    assert_same(hinted, want, "hint")
    assert_same(plain, want, "no hint")
    assert int(want[3][0]) > (64 if S == 104 else 8) and int(want[3][3]) >= 1 and int(want[3][5]) == 0


def test_one_long_chain_that_the_hint_does_not_cut():
    k, m, nb = 64, 32, 5000
    dec = codec()[1]
    words = np.zeros((nb, 3), np.uint32)
    words[1::2] = 0xFFFFFFFF  # absent, complete, absent, ...
    content, block_start, totals = dec.repair_requests(_dev(words), fec_id=5, fec_m=8, object_id=7, max_units=3)
    t = _np(totals, np.uint64)
    assert t[2] == 0 and t[3] == nb // 2  # no needing block: offset 0 is the hint's only boundary
    host = content.cpu().numpy()[:int(t[0])]
    header = norm_amd.nack_header(**NACK)
    got, want = fragment_both(host, 104, 5, header, int(t[0]) // 72 + 8, 128, block_start=block_start,
                              content_dev=(content, totals[:1]))
    assert_same(got, want)
    assert int(want[3][0]) > 128 and int(want[3][2]) == int(t[1])


@pytest.mark.parametrize("lead", range(16))
def test_intake_at_every_misalignment(lead):
    enc = codec()[0]
    table = control_table()
    table.append(table[2])  # the last datagram, a whole NACK with its extension, ends on the buffer's last byte
    wire, offs, lens = lay_out(table, lead)
    f = norm_amd.ctl_filter(SENDER, INSTANCE, local_id=LOCAL, flags=N.NFEC_CTL_TAKE_NACK if lead & 1 else N.NFEC_CTL_TAKE_ADV)
    want = norm_amd.ctl_parse_host(f, wire, offs, lens)
    n = offs.size
    d_wire = torch.from_numpy(wire.copy()).cuda()
    assert d_wire.data_ptr() % 16 == 0 and int(offs[-1]) + int(lens[-1]) == d_wire.numel()
    cls = torch.full((n,), 0x55, dtype=torch.uint8, device="cuda")
    src = torch.zeros(n, dtype=torch.int32, device="cuda")
    grtt = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
    stats = torch.zeros(9, dtype=torch.int32, device="cuda")
    coff, clen = enc.ingest_control(d_wire, _dev(offs), _dev(lens), f, class_out=cls, source_id_out=src,
                                    grtt_response_out=grtt, stats=stats)
    torch.cuda.synchronize()
    got = (cls.cpu().numpy(), _np(coff, np.uint64), _np(clen, np.uint16), _np(src, np.uint32), _np(grtt, np.uint32),
           _np(stats, np.uint32))
    for g, w, name in zip(got, want, ("class", "content offset", "content length", "source id", "grtt response", "stats")):
        assert np.array_equal(g, w), (name, g[:8], w[:8])
    assert int(got[5].sum()) == n and (got[1] == 0).sum() > 10
    if lead & 1:
        # the table as it is goes to the sender: a (0, 0) entry is a readable, empty message
        state = norm_amd.tx_repair_state(4, 64, 32, 0, device="cuda")
        t = _np(enc.handle_nacks(state, d_wire, coff, clen, fec_id=5, fec_m=8), np.uint64)
        h_t = norm_amd.tx_handle_nacks_host(64, 32, norm_amd.tx_repair_state(4, 64, 32, 0), wire, want[1], want[2])
        assert np.array_equal(t, h_t) and t[5] == 0 and t[4] == ((want[2] > 0) & (want[2] < 4)).sum()  # (the cut datagrams)
        nothing = (want[1] == 0) & (want[2] == 0)
        t = _np(enc.handle_nacks(state, d_wire, coff[torch.from_numpy(nothing).cuda()].contiguous(),
                                 clen[torch.from_numpy(nothing).cuda()].contiguous(), fec_id=5, fec_m=8), np.uint64)
        assert nothing.sum() > 10 and t.tolist() == [0, 0, 0, 0, 0, 0]


@pytest.mark.parametrize("ext", [None, EXT], ids=["base", "extension"])
def test_adv_message_equals_the_host_twin(ext):
    enc = codec()[0]
    rng = np.random.default_rng(9)
    h = norm_amd.adv_header(SENDER, INSTANCE, sequence=0xBEEF, grtt=0x7A, backoff=4, gsize=3, ext=ext)
    H = 28 if ext else 16
    for table, fits in (([(ITEMS, 1, 2)], True), ([(ITEMS, 1, 1), (ITEMS, 2, 3)], True), ([(ITEMS, 1, 9), (RANGES, 1, 7)], False),
                        ([(ITEMS, 1, 1), (ITEMS, 1, 2), (ITEMS, 1, 2)], False), ([(RANGES, 1, 5)], False), ([], True)):
        content, reqs = build(table, 5, 8, rng)
        want, want_totals = norm_amd.adv_message_host(np.frombuffer(content, np.uint8), h, 40)
        cd, nbytes = bytes_dev(content)
        wire = torch.full((H + 40 + 16,), CANARY, dtype=torch.uint8, device="cuda")
        _, length, totals = enc.repair_adv_message(cd, nbytes, h, 40, wire=wire)
        torch.cuda.synchronize()
        n = int(_np(length, np.uint16)[0])
        got = wire.cpu().numpy()
        assert n == len(want) and got[:n].tobytes() == want and (got[n:] == CANARY).all()
        assert np.array_equal(_np(totals, np.uint64), want_totals) and int(want_totals[2]) == (0 if fits else 1)
        if table:
            assert got[13] == (0 if fits else 1)
            if fits:
                assert got[H:n].tobytes() == content


def test_closed_loop_with_the_nack_leg_in_hbm():
    """test_gpu_txrepair.py's loop, the NACKs never leaving HBM: every receiver's content is cut into
    NORM_NACK messages that interleave in one wire buffer (receiver r's message i in slot i * R + r),
    the sender's intake finds their content, and handle_nacks takes the intake's tables as they are.
    The host route (host content of the same masks, nfec_nack_fragment_host, nfec_ctl_parse_host,
    nfec_tx_handle_nacks_host) runs alongside on host state; after every round both states are equal.
    Round 2 also sends the sender's advertisement through the intake into a receiver's suppression
    state."""
    k, m, vec, nb, R, S = 64, 32, 1400, 300, 3, 1400
    fec_id, fec_m, first, idlen = 5, 8, 0xFFFF00, 4
    rng = np.random.default_rng(301)
    enc = NormEncoderRS8()
    decs = [NormDecoderRS8() for _ in range(R)]
    assert enc.Init(k, m, vec) and all(d.Init(k, m, vec) for d in decs)
    src = torch.from_numpy(rng.integers(0, 256, (nb, k + m, vec), dtype=np.uint8)).cuda()
    enc.encode_blocks(src)
    rxb = [torch.zeros_like(src) for _ in range(R)]
    masks = [norm_amd.received_mask(nb, k, m) for _ in range(R)]
    state = norm_amd.tx_repair_state(nb, k, m, 0, device="cuda")
    h_state = norm_amd.tx_repair_state(nb, k, m, 0)
    h_pending = Sender(k, m, [k] * nb).pending()
    pending = _dev(h_pending)
    gone = [int(b) for b in rng.choice(nb, 7, replace=False)]
    H = norm_amd.nack_header_bytes(0)
    pitch = H + S
    cap = norm_amd.repair_content_bound(k, m, nb, fec_id) // (S - 40) + 2  # messages of one receiver
    slots = cap * R
    table_off = torch.arange(slots, dtype=torch.int64, device="cuda") * pitch
    sender_filter = norm_amd.ctl_filter(SENDER, INSTANCE, local_id=SENDER, flags=N.NFEC_CTL_TAKE_NACK)
    rounds, adv_checked = 0, False
    while True:
        rounds += 1
        assert rounds <= 40
        off, blk, sym, ln, start = enc.list_pending(pending, gap=idlen)
        count, nbytes = (int(x) for x in _np(start, np.uint64)[nb])
        wire = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        enc.emit_segments(src, wire, off, blk, sym, ln, count_dev=start[nb, :1], fec_id=fec_id, fec_m=fec_m,
                          first_block_id=first, pending=pending)
        enc.end_blocks(state, pending)
        h_pending[:] = 0
        norm_amd.tx_end_blocks_host(k, m, h_state, h_pending)
        h_off, h_blk, h_ln = _np(off, np.uint64)[:count], _np(blk, np.uint32)[:count], _np(ln, np.uint16)[:count]
        # the device leg: nothing of the content comes to the host
        nack_wire = torch.zeros((slots + R) * pitch, dtype=torch.uint8, device="cuda")  # (room for every view's last slot)
        table_len = torch.zeros(slots, dtype=torch.int16, device="cuda")
        h_wire, h_len = np.zeros((slots + R) * pitch, np.uint8), np.zeros(slots, np.uint16)
        asked = 0
        for r in range(R):
            keep = rng.random(count) >= 0.45
            if rounds == 1 and r == 0:
                keep &= ~np.isin(h_blk, gone)
            decs[r].ingest_messages(rxb[r], masks[r], wire, _dev(h_off[keep]), _dev(h_ln[keep]), fec_id, fec_m,
                                    first_block_id=first)
            decs[r].decode_received(rxb[r], masks[r])
            content, block_start, totals = decs[r].repair_requests(masks[r], fec_id=fec_id, fec_m=fec_m, object_id=7,
                                                                   first_block_id=first)
            header = norm_amd.nack_header(0x0A000001 + r, SENDER, INSTANCE, grtt_response=(rounds, r))
            _, _, lens, _ = decs[r].nack_messages(content, totals[:1], header, S, fec_id=fec_id, block_start=block_start,
                                                  wire=nack_wire[r * pitch:], pitch=R * pitch, capacity=cap)
            table_len[r::R] = lens
            # the host route, from the mask
            h_content, _, h_totals = norm_amd.rx_repair_requests_host(k, m, _np(masks[r], np.uint32), None, fec_id, fec_m, 7, first)
            h_content = h_content[:int(h_totals[0])]
            asked += h_content.size
            w, o, ll, t = norm_amd.nack_fragment_host(h_content, header, S, fec_id=fec_id, capacity=cap)
            assert int(t[0]) <= cap and int(t[5]) == 0
            for i in range(int(t[0])):
                at = (i * R + r) * pitch
                h_wire[at:at + int(ll[i])] = w[int(o[i]):int(o[i]) + int(ll[i])]
                h_len[i * R + r] = ll[i]
        if not asked:
            break
        stats = torch.zeros(9, dtype=torch.int32, device="cuda")
        coff, clen = enc.ingest_control(nack_wire, table_off, table_len, sender_filter, stats=stats)
        t = enc.handle_nacks(state, nack_wire, coff, clen, fec_id=fec_id, fec_m=fec_m, object_id=7, first_block_id=first)
        h_table_off = np.arange(slots, dtype=np.uint64) * pitch
        h_cls, h_coff, h_clen, _, h_grtt, h_stats = norm_amd.ctl_parse_host(sender_filter, h_wire, h_table_off, h_len)
        h_t = norm_amd.tx_handle_nacks_host(k, m, h_state, h_wire, h_coff, h_clen, None, fec_id, fec_m, 7, first)
        if rounds == 2:
            adv_checked = check_advertisement(enc, decs[0], state, h_state, masks[0], k, m, nb, fec_id, fec_m, first)
        a = enc.activate_repairs(state, pending)
        h_a = norm_amd.tx_activate_repairs_host(k, m, h_state, h_pending)
        torch.cuda.synchronize()
        assert np.array_equal(nack_wire.cpu().numpy(), h_wire) and np.array_equal(_np(table_len, np.uint16), h_len)
        assert np.array_equal(_np(coff, np.uint64), h_coff) and np.array_equal(_np(clen, np.uint16), h_clen)
        assert np.array_equal(_np(stats, np.uint32), h_stats)
        assert h_stats[N.NFEC_CTL_NACK] == (h_len > 0).sum() and h_stats[N.NFEC_CTL_UNREADABLE] == (h_len == 0).sum()
        assert np.array_equal(_np(t, np.uint64), h_t) and np.array_equal(_np(a, np.uint64), h_a), (rounds, t, h_t, a, h_a)
        assert h_t[4] == 0 and h_t[5] == 0
        same_state(state.to_host(), h_state)
        assert np.array_equal(_np(pending, np.uint32), h_pending)
    assert rounds >= 3 and adv_checked
    for r in range(R):
        assert torch.equal(rxb[r][:, :k], src[:, :k])


def check_advertisement(enc, dec, state, h_state, mask, k, m, nb, fec_id, fec_m, first):
    """The sender's state -> repair_adv -> repair_adv_message -> ingest_control -> handle_repair_content
    on the device, against the host twins of all four."""
    S = 1400
    header = norm_amd.adv_header(SENDER, INSTANCE, sequence=9, grtt=0x40, backoff=4, gsize=1)
    f = norm_amd.ctl_filter(SENDER, INSTANCE, local_id=0x0A000001, flags=N.NFEC_CTL_TAKE_ADV)
    content, _, totals = enc.repair_adv(state, fec_id=fec_id, fec_m=fec_m, object_id=7, first_block_id=first)
    wire, length, adv_totals = enc.repair_adv_message(content, totals[:1], header, S, fec_id=fec_id)
    coff, clen = dec.ingest_control(wire, torch.zeros(1, dtype=torch.int64, device="cuda"), length, f)
    rx = norm_amd.rx_repair_state(nb, k, m, device="cuda")
    t = dec.handle_repair_content(rx, mask, wire, coff, clen, fec_id=fec_id, fec_m=fec_m, object_id=7, first_block_id=first)
    h_content, _, h_totals = norm_amd.tx_repair_adv_host(k, m, h_state, None, fec_id, fec_m, 7, first)
    h_msg, h_adv_totals = norm_amd.adv_message_host(h_content[:int(h_totals[0])], header, S, fec_id=fec_id)
    h_wire = np.frombuffer(h_msg, np.uint8)
    _, h_coff, h_clen, _, _, _ = norm_amd.ctl_parse_host(f, h_wire, np.zeros(1, np.uint64), np.array([h_wire.size], np.uint16))
    h_rx = norm_amd.rx_repair_state(nb, k, m)
    h_t = norm_amd.rx_handle_repair_content_host(k, m, h_rx, _np(mask, np.uint32), h_wire, h_coff, h_clen, None, fec_id, fec_m, 7,
                                                 first)
    torch.cuda.synchronize()
    n = int(_np(length, np.uint16)[0])
    assert n == h_wire.size > 16 and wire.cpu().numpy()[:n].tobytes() == h_msg
    assert np.array_equal(_np(adv_totals, np.uint64), h_adv_totals) and int(h_adv_totals[2]) == 1  # more than one message's worth
    assert np.array_equal(_np(t, np.uint64), h_t) and int(h_t[0]) > 0 and int(h_clen[0]) == n - 16
    same_rx_state(rx.to_host(), h_rx)
    return True
