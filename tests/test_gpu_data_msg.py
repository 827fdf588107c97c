"""Whole NORM_DATA messages on the device: nfec_tx_emit_data and nfec_rx_ingest_data.

The sender call writes the message header (reference include/normMessage.h:688-696, :769-779), the FEC
payload ID at byte 16 (:1183-1186), the FTI extension the reference's default sender attaches to every
NORM_DATA (fti_mode FTI_ALWAYS, src/common/normSession.cpp:58; src/common/normObject.cpp:1808-1857) and
the payload; the receiver call takes raw datagrams by (offset, length), classifies them by
NormMsg::InitFromBuffer's rule (src/common/normMessage.cpp:17-92) and places the payload found at
4 * hdr_len.  These tests hold the emission byte for byte to the model of tests/test_data_msg_host.py,
the intake to nfec_rx_parse_data_host (held to that model there) followed by nfec_rx_place, and run the
chain object -> blocks -> parity -> datagrams -> blocks -> repair -> object on one stream."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import norm_amd  # noqa: E402
from norm_amd import _native as N  # noqa: E402
from norm_amd import NFEC_MDP, NFEC_RS8, NFEC_RS16  # noqa: E402
from oracle import wire_ref as R  # noqa: E402
from test_data_msg_host import BITS, IDLEN, INST, OBJ, SRC, model_header  # noqa: E402
from test_gpu_tx import DEC, ENC, FIRST_BLOCK_ID, _dev, _np, wire_layout  # noqa: E402
from test_tx_host import num_data_for  # noqa: E402

FILL = 0xA5
# kind, k, m, vec, seg stride, blocks, fec_id, fec_m: tests/test_gpu_rx_ingest.py's shapes (1,400 bytes
# are 88 pieces of 16, so a wave needs a second round; vec 40 / 41 end in a whole and in a partial
# 8-byte piece below a 48-byte stride)
SHAPES = [
    (NFEC_RS8, 8, 2, 40, 48, 5, 2, 8),
    (NFEC_RS8, 64, 32, 1400, 1400, 3, 5, 8),
    (NFEC_RS16, 400, 100, 1400, 1400, 2, 2, 16),
    (NFEC_MDP, 8, 2, 41, 48, 5, 129, 8),
]
CASES = [s + (f,) for s in SHAPES for f in (False, True)]
IDS = ["%d-%d-fec%d-%s" % (s[1], s[3], s[6], "fti" if s[8] else "plain") for s in CASES]
HDR = dict(grtt=0x9C, backoff=5, gsize=3, flags=0x1A)
(U, T, M, S, C, O, REJ, DUP, PLACED) = range(9)


def _codec(table, kind, k, m, vec):
    c = table[kind]()
    assert c.Init(k, m, vec)
    return c


def _fti(fec_id, fec_m, seg=1392, k=64, m=32, size=0x123456789A):
    return R.fti(fec_id, seg, k, m, object_size=size, fec_m=fec_m)


def _field(fec_id, fec_m):
    return (1 << BITS[(fec_id, fec_m)]) - 1


def _filled(nb, k, m, stride):
    return torch.full((nb, k + m, stride), FILL, dtype=torch.uint8, device="cuda")


def _fill(n, dtype):
    return torch.full((n,), -86 if dtype != torch.uint8 else 0xAA, dtype=dtype, device="cuda")


def _accepts(b, s, ln, nb, nd, k, m, vec):
    return b < nb and 1 <= int(nd[b]) <= k and s < int(nd[b]) + m and ln <= vec


@pytest.mark.parametrize("kind,k,m,vec,stride,nb,fec_id,fec_m,with_fti", CASES, ids=IDS)
def test_emit_equals_the_model(kind, k, m, vec, stride, nb, fec_id, fec_m, with_fti):
    """Every payload length class at every residue of the payload offset, touching messages and junk
    gaps (wire_layout with gap = H), the wire buffer ending at its last message's last byte; rejected
    descriptors among the good ones."""
    rng = np.random.default_rng(k * 59 + vec + fec_id + with_fti)
    enc = _codec(ENC, kind, k, m, vec)
    ext = _fti(fec_id, fec_m) if with_fti else b""
    H = norm_amd.data_header_bytes(fec_id, len(ext))
    assert H == 16 + IDLEN[fec_id] + len(ext)
    nd = num_data_for(k, nb, 0)
    batch = rng.integers(1, 256, (nb, k + m, stride), dtype=np.uint8)
    valid = [(b, s) for b in range(nb) if 1 <= nd[b] <= k for s in range(int(nd[b]) + m)]
    last = max(valid)
    slots = [last] + [valid[i] for i in rng.integers(0, len(valid), 400)]
    entries, touching, seen, _ = wire_layout(rng, H, vec, slots)
    assert all((ln, r) in seen for ln in (0, 1, 7, 8, 9, 15, 16, 17, vec - 1, vec) for r in range(16))
    assert touching * 2 >= len(entries)
    P = max(off + ln for off, _, _, ln in entries)  # the buffer ends with its last message
    good = len(entries)
    bad_b = next(b for b in range(nb) if 1 <= nd[b] <= k)
    rejected = [
        (H + 100, nb, 0, 16),                         # block_index == nblocks
        (H + 200, bad_b, int(nd[bad_b]) + m, 16),     # symbol_id == nd_b + m
        (H + 300, bad_b, 0, vec + 1),                 # longer than the vector
        (H - 1, bad_b, 0, 4),                         # off < H
        (P - 3, bad_b, 0, 4),                         # ends one past payload_bytes
        (P + 8, bad_b, 0, 0),                         # off beyond the buffer
    ]
    if nb >= 5:
        rejected += [(H + 400, 3, 0, 8), (H + 500, 4, 0, 8)]  # numData 0 and k + 1
    order = [(e, True) for e in entries] + [(e, False) for e in rejected]
    order = [order[i] for i in rng.permutation(len(order))]
    first_seq = 65500
    hdr = norm_amd.data_header(SRC, INST, OBJ, fec_id, fec_m, first_sequence=first_seq, fti=ext or None, **HDR)
    want = np.full(P, FILL, np.uint8)
    want_off = np.zeros(len(order), np.uint64)
    want_len = np.zeros(len(order), np.uint16)
    words = (k + m + 31) // 32 + 1
    want_mask = np.full((nb, words), 0xFFFFFFFF, np.uint32)
    for i, ((off, b, s, ln), ok) in enumerate(order):
        if not ok:
            continue
        head = model_header(fec_id, fec_m, first_seq + i, (FIRST_BLOCK_ID + b) & _field(fec_id, fec_m), s, int(nd[b]),
                            ext, **HDR)
        assert len(head) == H
        want[off - H:off] = np.frombuffer(head, np.uint8)
        want[off:off + ln] = batch[b, s, :ln]
        want_off[i], want_len[i] = off - H, ln + H
        want_mask[b, s // 32] &= np.uint32(~(1 << (s % 32)) & 0xFFFFFFFF)
    cols = list(zip(*[e for e, _ in order]))
    dbatch = torch.from_numpy(batch.copy()).cuda()
    wire = torch.full((P,), FILL, dtype=torch.uint8, device="cuda")
    stats = torch.zeros(2, dtype=torch.int32, device="cuda")
    mask = _dev(np.full((nb, words), 0xFFFFFFFF, np.uint32))
    m_off, m_len = _fill(len(order), torch.int64), _fill(len(order), torch.int16)
    enc.emit_data_messages(dbatch, wire, _dev(np.array(cols[0], np.uint64)), _dev(np.array(cols[1], np.uint32)),
                           _dev(np.array(cols[2], np.uint16)), _dev(np.array(cols[3], np.uint16)), hdr,
                           first_block_id=FIRST_BLOCK_ID, pending=mask, num_data=_dev(nd), msg_offsets_out=m_off,
                           msg_length_out=m_len, stats=stats)
    torch.cuda.synchronize()
    got = wire.cpu().numpy()
    assert stats.cpu().tolist() == [good, len(rejected)]
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (bad[:8], len(bad))
    assert np.array_equal(_np(m_off, np.uint64), want_off) and np.array_equal(_np(m_len, np.uint16), want_len)
    assert np.array_equal(_np(mask, np.uint32), want_mask)
    assert np.array_equal(dbatch.cpu().numpy(), batch)


def _datagram_calls(rng, fec_id, fec_m, with_fti, k, m, vec, nb, nd, src, first):
    """Per call one pass over every slot of the batch in shuffled order (no slot twice in a call) with
    the other classes' datagrams among them.  Returns the wire bytes and per call a list of
    (offset, length, expected class, block, slot, payload length)."""
    idlen = IDLEN[fec_id]
    field = _field(fec_id, fec_m)
    fti = _fti(fec_id, fec_m)
    unknown = bytes([1, 2]) + b"\xAA" * 6
    exts = [b"", fti, unknown + fti] if with_fti else [b""]
    lengths = [0, 1, 7, 8, 9, 15, 16, 17, vec - 1, vec]
    other_code = 2 if fec_id != 2 else 5
    every = [(b, s) for b in range(nb) for s in range(k + m)]
    parts, calls, pos, seq = [], [], 0, 1000

    def put(gram, cls, b=-1, s=-1, ln=0, length=None):
        nonlocal pos
        gap = int(rng.integers(0, 6))
        parts.append(bytes(rng.integers(1, 256, gap, dtype=np.uint8)))
        pos += gap
        one.append((pos, len(gram) if length is None else length, cls, b, s, ln))
        parts.append(gram)
        pos += len(gram)

    for c in range(400 // len(every) + 2):
        one = []
        for j, i in enumerate(rng.permutation(len(every))):
            b, s = every[i]
            ln = lengths[(j + c) % len(lengths)] if (j + c) % 3 else int(rng.integers(0, vec + 1))
            blen = int(nd[b])
            cls = PLACED if _accepts(b, s, ln, nb, nd, k, m, vec) else REJ
            if j % 41 == 7:
                ln, cls = vec + 1, REJ                      # longer than the vector
            if fec_id == 129 and j % 29 == 5:
                blen, cls = blen + 1, REJ                   # the ID's block length is not the block's numData
            seq += 1
            head = model_header(fec_id, fec_m, seq, (first + b) & field, s, blen, exts[(j + c) % len(exts)], **HDR)
            pay = bytes(src[b, s, :min(ln, vec)]) + b"\x77" * max(0, ln - vec)
            put(head + pay, cls, b, s, ln)
            if j % 9 == 4:                                  # one of the other classes behind it
                pay = bytes(rng.integers(1, 256, 24, dtype=np.uint8))
                h = lambda **kw: model_header(fec_id, fec_m, seq, (first + b) & field, s, blen, **HDR, **kw)  # noqa: E731
                kind = (j // 9 + c) % 9
                if kind == 0:
                    put(h()[:7], U)
                elif kind == 1:
                    put(h(mtype=1) + pay, T)
                elif kind == 2:
                    put(h(mtype=4)[:8], T)
                elif kind == 3:
                    put(h(hdr_len=(16 + idlen) // 4 - 1) + pay, M)
                elif kind == 4:
                    put(h(hdr_len=(16 + idlen + 24) // 4 + 1) + pay, M)
                elif kind == 5:
                    put(h()[:16 + idlen - 1], M)
                elif kind == 6:
                    put(h(source=SRC ^ 0x100) + pay, S)
                elif kind == 7:
                    put(model_header(other_code, 8, seq, b, s, blen, **HDR) + pay, C)
                else:
                    put(h(obj=OBJ ^ 1) + pay, O)
        calls.append(one)
    # one datagram that claims more bytes than the buffer holds, in the last call
    calls[-1].append((pos - 10, 40, U, -1, -1, 0))
    return np.frombuffer(b"".join(parts), np.uint8).copy(), calls


@pytest.mark.parametrize("kind,k,m,vec,stride,nb,fec_id,fec_m,with_fti", CASES, ids=IDS)
def test_ingest_equals_host_parse_and_place(kind, k, m, vec, stride, nb, fec_id, fec_m, with_fti):
    rng = np.random.default_rng(k * 61 + vec + fec_id + with_fti)
    dec = _codec(DEC, kind, k, m, vec)
    nd = num_data_for(k, nb, 0)
    first = FIRST_BLOCK_ID
    src = rng.integers(1, 256, (nb, k + m, stride), dtype=np.uint8)
    wire, calls = _datagram_calls(rng, fec_id, fec_m, with_fti, k, m, vec, nb, nd, src, first)
    assert calls[-1][-2][0] + calls[-1][-2][1] == wire.size  # the buffer ends with its last datagram
    flt = norm_amd.data_filter(SRC, INST, OBJ, fec_id, fec_m)
    dwire = torch.from_numpy(wire.copy()).cuda()
    dnd = _dev(nd)
    words = (k + m + 31) // 32 + 1
    dev_a, dev_b = _filled(nb, k, m, stride), _filled(nb, k, m, stride)
    mask_a = torch.zeros((nb, words), dtype=torch.int32, device="cuda")
    mask_b = torch.zeros_like(mask_a)
    seen_cls, seen_res = set(), set()
    for call in calls:
        n = len(call)
        off = np.array([e[0] for e in call], np.uint64)
        ln = np.array([e[1] for e in call], np.uint16)
        want_cls = np.array([e[2] for e in call], np.uint8)
        h_cls, h_seq, h_blk, h_sym, h_blen, h_poff, h_plen, h_fti = norm_amd.rx_parse_data_host(flt, first, wire, off, ln)
        parsed = h_cls == N.NFEC_DGRAM_PARSED
        assert np.array_equal(parsed, want_cls >= REJ) and np.array_equal(h_cls[~parsed], want_cls[~parsed])
        assert h_blk[parsed].tolist() == [e[3] for e in call if e[2] >= REJ]
        assert h_sym[parsed].tolist() == [e[4] for e in call if e[2] >= REJ]
        assert h_plen[parsed].tolist() == [e[5] for e in call if e[2] >= REJ]
        # what nfec_rx_place gets: the parsed datagrams, without those whose block length is not numData
        keep = parsed.copy()
        if fec_id == 129:
            for i in np.nonzero(parsed)[0]:
                keep[i] = h_blk[i] < nb and h_blen[i] == nd[h_blk[i]]
        mask_a.zero_()
        mask_b.zero_()
        stats_a = torch.zeros(9, dtype=torch.int32, device="cuda")
        stats_b = torch.zeros(3, dtype=torch.int32, device="cuda")
        totals = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        o_cls, o_seq = _fill(n, torch.uint8), _fill(n, torch.int16)
        o_blk, o_sym = _fill(n, torch.int32), _fill(n, torch.int16)
        dec.ingest_datagrams(dev_a, mask_a, dwire, _dev(off), _dev(ln), flt, first_block_id=first, num_data=dnd,
                             class_out=o_cls, sequence_out=o_seq, block_index_out=o_blk, symbol_id_out=o_sym,
                             stats=stats_a, totals=totals)
        dec.place_segments(dev_b, mask_b, dwire, _dev(h_poff[keep]), _dev(h_blk[keep]), _dev(h_sym[keep]),
                           _dev(h_plen[keep]), num_data=dnd, stats=stats_b)
        torch.cuda.synchronize()
        got, ref = dev_a.cpu().numpy(), dev_b.cpu().numpy()
        placed, dup, rej = stats_b.cpu().tolist()
        want_stats = np.bincount(want_cls, minlength=9)
        assert stats_a.cpu().tolist() == want_stats.tolist()
        assert (placed, dup, rej + int((parsed & ~keep).sum())) == (want_stats[PLACED], 0, want_stats[REJ])
        assert np.array_equal(o_cls.cpu().numpy(), want_cls)
        assert np.array_equal(_np(mask_a, np.uint32), _np(mask_b, np.uint32))
        bad = np.argwhere(got != ref)
        assert bad.size == 0, (bad[:4], len(bad))
        assert (got[:, :, vec:] == FILL).all()  # the stride padding keeps the caller's bytes
        readable = want_cls != U
        g_seq = _np(o_seq, np.uint16)
        assert np.array_equal(g_seq[readable], h_seq[readable]) and (o_seq.cpu().numpy()[~readable] == -86).all()
        assert np.array_equal(_np(o_blk, np.uint32), h_blk) and np.array_equal(_np(o_sym, np.uint16), h_sym)
        assert int(totals.item()) == (-1 if h_fti is None else h_fti)
        assert (h_fti is not None) == with_fti
        for (_, _, cls, b, s, n_pay) in call:
            if cls == PLACED:
                assert np.array_equal(got[b, s, :n_pay], src[b, s, :n_pay]) and not got[b, s, n_pay:vec].any(), (b, s)
        seen_cls |= set(want_cls.tolist())
        seen_res |= {int(e[0]) % 16 for e in call}
    assert seen_cls == set(range(7)) | {PLACED} and seen_res == set(range(16))
    assert torch.equal(dwire.cpu(), torch.from_numpy(wire))  # read only
    # every datagram of the last call twice, in one call, into an empty batch: one copy of each slot
    # wins, whichever wave comes first
    call = calls[-1] * 2
    call = [call[i] for i in rng.permutation(len(call))]
    dev_c = _filled(nb, k, m, stride)
    mask_c = torch.zeros_like(mask_a)
    stats = torch.zeros(9, dtype=torch.int32, device="cuda")
    dec.ingest_datagrams(dev_c, mask_c, dwire, _dev(np.array([e[0] for e in call], np.uint64)),
                         _dev(np.array([e[1] for e in call], np.uint16)), flt, first_block_id=first, num_data=dnd,
                         stats=stats)
    torch.cuda.synchronize()
    once = np.bincount([e[2] for e in calls[-1]], minlength=9)
    st = stats.cpu().tolist()
    assert st[PLACED] + st[DUP] == 2 * once[PLACED] and st[PLACED] == once[PLACED]
    assert st[:REJ + 1] == (2 * once[:REJ + 1]).tolist()
    want = np.full(src.shape, FILL, np.uint8)
    for (_, _, cls, b, s, n_pay) in calls[-1]:
        if cls == PLACED:
            want[b, s, :n_pay] = src[b, s, :n_pay]
            want[b, s, n_pay:vec] = 0
    assert np.array_equal(dev_c.cpu().numpy(), want)
    assert np.array_equal(_np(mask_c, np.uint32), _np(mask_a, np.uint32))


@pytest.mark.parametrize("kind,k,m,vec,stride,nb,fec_id,fec_m", SHAPES, ids=IDS[1::2])
def test_default_layout_chain_on_one_stream(kind, k, m, vec, stride, nb, fec_id, fec_m):
    """read_object -> encode_blocks -> list_pending(gap = H) -> emit_data_messages -> ingest_datagrams
    (the emission's datagram table, the list's total) -> decode_received -> write_object with no
    synchronize between them, the FTI on every message.  Every block loses m of its datagrams, their
    length set to zero on the device: a third of them for (64, 32), and as many as the code repairs for
    the other shapes."""
    rng = np.random.default_rng(k * 67 + vec)
    enc, dec = _codec(ENC, kind, k, m, vec), _codec(DEC, kind, k, m, vec)
    seg = vec - 8
    nseg = nb * k - nb // 2
    lay = norm_amd.object_layout((nseg - 1) * seg + seg - 1, seg, k)
    assert lay.num_blocks == nb
    sizes = norm_amd.object_block_sizes(lay, 0, nb)
    obj = rng.integers(1, 256, lay.object_size, dtype=np.uint8)
    ext = _fti(fec_id, fec_m, seg=seg, k=min(k, 255) if fec_id == 5 else k, m=m, size=lay.object_size)
    H = norm_amd.data_header_bytes(fec_id, len(ext))
    idlen = IDLEN[fec_id]
    count = int(sizes.sum()) + nb * m
    # the loss: m datagrams of every block, by their index in the list (blocks ascending, slots ascending)
    drop, at = [], 0
    for b in range(nb):
        n = int(sizes[b]) + m
        drop += [at + int(x) for x in rng.choice(n, m, replace=False)]
        at += n
    assert at == count and ((k, m) != (64, 32) or abs(3 * len(drop) - count) <= nb)
    first_alive = min(set(range(count)) - set(drop))
    if first_alive == 0:  # make the first datagram one of the lost, so that totals[0] is not simply 0
        drop[drop.index(min(drop))] = 0
        first_alive = min(set(range(count)) - set(drop))
    assert len(set(drop)) == nb * m
    ddrop = torch.tensor(sorted(set(drop)), dtype=torch.int64, device="cuda")
    words = (k + m + 31) // 32
    pend = np.zeros((nb, words), np.uint32)
    for b in range(nb):
        for s in range(int(sizes[b]) + m):
            pend[b, s // 32] |= np.uint32(1 << (s % 32))
    first = FIRST_BLOCK_ID & _field(fec_id, fec_m)
    hdr = norm_amd.data_header(SRC, INST, OBJ, fec_id, fec_m, first_sequence=65000, fti=ext, **HDR)
    flt = norm_amd.data_filter(SRC, INST, OBJ, fec_id, fec_m)
    dobj = torch.from_numpy(obj).cuda()
    dev = torch.zeros((nb, k + m, stride), dtype=torch.uint8, device="cuda")
    dnd = torch.zeros(nb, dtype=torch.int16, device="cuda")
    dlens = torch.zeros((nb, k), dtype=torch.int16, device="cuda")
    dpend = _dev(pend)
    P = int(sizes.sum()) * seg - 1 + nb * m * seg + count * H  # every byte of it a message's
    wire = torch.full((P,), FILL, dtype=torch.uint8, device="cuda")
    dev2 = _filled(nb, k, m, stride)
    mask = norm_amd.received_mask(nb, k, m)
    cap = nb * (k + m)
    m_off, m_len = torch.zeros(cap, dtype=torch.int64, device="cuda"), torch.zeros(cap, dtype=torch.int16, device="cuda")
    o_seq = _fill(cap, torch.int16)
    o_cls = _fill(cap, torch.uint8)
    tstats = torch.zeros(2, dtype=torch.int32, device="cuda")
    rstats = torch.zeros(9, dtype=torch.int32, device="cuda")
    totals = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    dout = torch.full((lay.object_size,), FILL, dtype=torch.uint8, device="cuda")
    # sender
    enc.read_object(dobj, lay, dev, num_data=dnd, seg_length=dlens)
    enc.encode_blocks(dev, num_data=dnd)
    off, blk, sym, ln, start = enc.list_pending(dpend, num_data=dnd, seg_length=dlens, gap=H)
    enc.emit_data_messages(dev, wire, off, blk, sym, ln, hdr, count_dev=start[nb, :1], first_block_id=first,
                           num_data=dnd, msg_offsets_out=m_off, msg_length_out=m_len, stats=tstats)
    # the network
    m_len[ddrop] = 0
    # receiver: the wire buffer, the datagram table and the list's total
    dec.ingest_datagrams(dev2, mask, wire, m_off, m_len, flt, first_block_id=first, count_dev=start[nb, :1],
                         num_data=dnd, class_out=o_cls, sequence_out=o_seq, stats=rstats, totals=totals)
    st = dec.decode_received(dev2, mask, num_data=dnd)
    dec.write_object(dout, lay, dev2, received=mask, status=st)
    torch.cuda.synchronize()
    assert int(_np(start, np.uint64)[nb, 0]) == count and int(_np(start, np.uint64)[nb, 1]) == P
    assert tstats.cpu().tolist() == [count, 0]
    want_stats = [0] * 9
    want_stats[U], want_stats[PLACED] = nb * m, count - nb * m
    assert rstats.cpu().tolist() == want_stats
    assert np.array_equal(dout.cpu().numpy(), obj)
    cls = o_cls.cpu().numpy()
    lost = np.zeros(cap, bool)
    lost[sorted(set(drop))] = True
    assert (cls[:count][lost[:count]] == U).all() and (cls[:count][~lost[:count]] == PLACED).all()
    assert (cls[count:] == 0xAA).all()
    seqs = _np(o_seq, np.uint16)
    alive = np.nonzero(~lost[:count])[0]
    assert np.array_equal(seqs[alive], ((65000 + alive) & 0xFFFF).astype(np.uint16))
    # the first surviving datagram carries the FTI that sizes the object
    assert int(totals.item()) == first_alive
    got = wire.cpu().numpy()
    assert not (got == FILL).all() and got.size == P
    at = int(m_off.cpu().numpy()[first_alive]) + 16 + idlen
    out = N.Fti()
    fti_bytes = got[at:at + len(ext)].copy()
    assert N.lib().nfec_fti_read(fec_id, fti_bytes.ctypes.data, fti_bytes.size, out) == len(ext)
    assert out.object_size == lay.object_size and out.segment_size == seg


def test_count_dev_bounds_both_calls():
    kind, k, m, vec, stride, nb, fec_id, fec_m = SHAPES[0]
    rng = np.random.default_rng(29)
    enc, dec = _codec(ENC, kind, k, m, vec), _codec(DEC, kind, k, m, vec)
    ext = _fti(fec_id, fec_m)
    H = norm_amd.data_header_bytes(fec_id, len(ext))
    first = 0xFFFFFE
    batch = rng.integers(1, 256, (nb, k + m, stride), dtype=np.uint8)
    slots = [(b, s) for b in range(nb) for s in range(k + m)]
    slots = [slots[i] for i in rng.permutation(len(slots))]
    entries = [(H + i * (vec + H + 3), b, s, vec - i % 7) for i, (b, s) in enumerate(slots)]
    n = len(entries)
    P = entries[-1][0] + entries[-1][3]
    hdr = norm_amd.data_header(SRC, INST, OBJ, fec_id, fec_m, first_sequence=9, fti=ext, **HDR)
    flt = norm_amd.data_filter(SRC, INST, OBJ, fec_id, fec_m)
    cols = [_dev(np.array(c, dt)) for c, dt in zip(zip(*entries), (np.uint64, np.uint32, np.uint16, np.uint16))]
    dbatch = torch.from_numpy(batch.copy()).cuda()
    for have, done in ((37, 37), (0, 0), (1 << 40, n)):  # below count, nothing, above count
        cd = torch.tensor([have], dtype=torch.int64, device="cuda")
        wire = torch.full((P,), FILL, dtype=torch.uint8, device="cuda")
        tstats = torch.zeros(2, dtype=torch.int32, device="cuda")
        m_off, m_len = _fill(n, torch.int64), _fill(n, torch.int16)
        pend = _dev(np.full((nb, 1), 0xFFFFFFFF, np.uint32))
        enc.emit_data_messages(dbatch, wire, *cols, hdr, count_dev=cd, first_block_id=first, pending=pend,
                               msg_offsets_out=m_off, msg_length_out=m_len, stats=tstats)
        torch.cuda.synchronize()
        assert tstats.cpu().tolist() == [done, 0]
        want = np.full(P, FILL, np.uint8)
        for i, (off, b, s, ln) in enumerate(entries[:done]):
            want[off - H:off] = np.frombuffer(model_header(fec_id, fec_m, 9 + i, (first + b) & 0xFFFFFF, s, k, ext,
                                                           **HDR), np.uint8)
            want[off:off + ln] = batch[b, s, :ln]
        assert np.array_equal(wire.cpu().numpy(), want)
        mo, ml = m_off.cpu().numpy(), m_len.cpu().numpy()
        assert mo[:done].tolist() == [e[0] - H for e in entries[:done]] and (mo[done:] == -86).all()
        assert ml[:done].tolist() == [e[3] + H for e in entries[:done]] and (ml[done:] == -86).all()
        assert int(np.unpackbits(_np(pend, np.uint32).view(np.uint8)).sum()) == nb * 32 - done
        # the intake on the whole emission, bounded the same way
        full = torch.from_numpy(want if done == n else _emit_all(entries, batch, fec_id, fec_m, first, k, ext, H, P)).cuda()
        d_off = _dev(np.array([e[0] - H for e in entries], np.uint64))
        d_len = _dev(np.array([e[3] + H for e in entries], np.uint16))
        dev = _filled(nb, k, m, stride)
        mask = norm_amd.received_mask(nb, k, m)
        rstats = torch.zeros(9, dtype=torch.int32, device="cuda")
        totals = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        o_cls, o_seq = _fill(n, torch.uint8), _fill(n, torch.int16)
        o_blk, o_sym = _fill(n, torch.int32), _fill(n, torch.int16)
        dec.ingest_datagrams(dev, mask, full, d_off, d_len, flt, first_block_id=first, count_dev=cd, class_out=o_cls,
                             sequence_out=o_seq, block_index_out=o_blk, symbol_id_out=o_sym, stats=rstats,
                             totals=totals)
        torch.cuda.synchronize()
        want_stats = [0] * 9
        want_stats[PLACED] = done
        assert rstats.cpu().tolist() == want_stats
        assert int(totals.item()) == (0 if done else -1)
        wb = np.full(batch.shape, FILL, np.uint8)
        for _, b, s, ln in entries[:done]:
            wb[b, s, :ln] = batch[b, s, :ln]
            wb[b, s, ln:vec] = 0
        assert np.array_equal(dev.cpu().numpy(), wb)
        oc, oq, ob, os_ = o_cls.cpu().numpy(), o_seq.cpu().numpy(), o_blk.cpu().numpy(), o_sym.cpu().numpy()
        assert (oc[:done] == PLACED).all() and (oc[done:] == 0xAA).all()
        assert oq[:done].tolist() == [9 + i for i in range(done)] and (oq[done:] == -86).all()
        assert ob[:done].tolist() == [e[1] for e in entries[:done]] and (ob[done:] == -86).all()
        assert os_[:done].tolist() == [e[2] for e in entries[:done]] and (os_[done:] == -86).all()
        assert int(np.unpackbits(_np(mask, np.uint32).view(np.uint8)).sum()) == done


def _emit_all(entries, batch, fec_id, fec_m, first, k, ext, H, P):
    want = np.full(P, FILL, np.uint8)
    for i, (off, b, s, ln) in enumerate(entries):
        want[off - H:off] = np.frombuffer(model_header(fec_id, fec_m, 9 + i, (first + b) & 0xFFFFFF, s, k, ext, **HDR),
                                          np.uint8)
        want[off:off + ln] = batch[b, s, :ln]
    return want
