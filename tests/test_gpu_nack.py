"""Repair requests on the device: nfec_rx_repair_requests (norm_amd/csrc/kernels_nack.hip) against
the host entry's bytes, block_start and totals (nfec_rx_repair_requests_host, itself held to a serial
walk of the reference's rule in tests/test_nack_host.py), and the receiver's whole cycle on the
device: loss -> repair requests -> the sender's pending masks -> retransmission, until nothing is
asked for."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import norm_amd  # noqa: E402
from norm_amd import _native as N  # noqa: E402
from norm_amd import NormDecoderRS8, NormDecoderRS16, NormEncoderRS8  # noqa: E402
from test_gpu_tx import _dev, _np  # noqa: E402
from test_nack_host import (ABSENT, BLOCK, NEEDING, SEGMENT, SILENT, block_with_runs, blocks_from_classes, lossy,  # noqa: E402
                            to_words)

SENTINEL = 0xEE
TILE = 8192  # the scan kernel's tile (kNackScanTile)
_CODECS = {}


def codec(k, m):
    if (k, m) not in _CODECS:
        dec = NormDecoderRS8() if k + m <= 255 else NormDecoderRS16()
        assert dec.Init(k, m, 64)
        _CODECS[(k, m)] = dec
    return _CODECS[(k, m)]


def compare(k, m, words, nds, fec=(5, 8), object_id=0xBEEF, first=0, info=False, max_units=None, capacity=None,
            stream=None, content=None):
    """the device call against the host entry on the same words"""
    nds = np.asarray(nds, np.uint16)
    flags = N.NFEC_NACK_INFO if info else 0
    h_content, h_start, h_totals = norm_amd.rx_repair_requests_host(k, m, words, nds, fec[0], fec[1], object_id, first,
                                                                    flags, max_units)
    total = int(h_totals[0])
    if content is None:
        capacity = total + 64 if capacity is None else capacity
        content = torch.full((capacity + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    else:
        capacity = content.numel()
    dmask = _dev(words)
    out, start, totals = codec(k, m).repair_requests(dmask, num_data=_dev(nds), fec_id=fec[0], fec_m=fec[1],
                                                     object_id=object_id, first_block_id=first, flags=flags,
                                                     max_units=max_units, capacity=capacity, content=content,
                                                     stream=stream)
    torch.cuda.synchronize()
    assert np.array_equal(_np(totals, np.uint64), h_totals), (_np(totals, np.uint64), h_totals)
    bad = np.argwhere(_np(start, np.uint64) != h_start)
    assert bad.size == 0, (bad[:4], _np(start, np.uint64)[bad[0, 0]], h_start[bad[0, 0]])
    got = out.cpu().numpy()
    n = min(total, capacity)
    bad = np.argwhere(got[:n] != h_content[:n])
    assert bad.size == 0, (bad[:4].ravel(), len(bad), total)
    assert (got[n:] == SENTINEL).all()  # nothing at or past the capacity, nothing at or past the total
    assert np.array_equal(_np(dmask, np.uint32), words)  # the mask is only read
    return total, h_totals


def mixed(rng, nb, k, m, loss):
    got = lossy(rng, nb, k, m, loss)
    nds = np.where(rng.random(nb) < 0.5, k, k - 1)
    for b in range(nb):
        r = rng.random()
        if r < 0.2:
            got[b] = False
        elif r < 0.35:
            got[b, :nds[b]] = True
    nds[nb // 2] = 0
    return got, nds


@pytest.mark.parametrize("k,m", [(8, 4), (64, 32)])
def test_corners(k, m):
    rng = np.random.default_rng(k)
    for loss in (0.05, 0.4, 0.65, 0.95):
        got, nds = mixed(rng, 41, k, m, loss)
        words = to_words(got, nds, m, (k + m + 31) // 32 + 1, rng)
        for fec, first in (((5, 8), 0xFFFFF0), ((2, 16), 0xFFF0), ((129, 8), 0xFFFFFFF0)):
            compare(k, m, words, nds, fec=fec, first=first)
        for max_units in (1, 2, 3):
            compare(k, m, words, nds, max_units=max_units, info=True)
    A, S, Nd = ABSENT, SILENT, NEEDING
    for classes in ([A, S, A, A, S, A], [A, S, A, A, A, S, A], [A, A, A, S, A, A, A, A], [A, A, Nd, A, A, A],
                    [Nd, Nd, A], [S, A, S], [A] * 7, [S] * 5, [Nd], [A], [S]):
        got = blocks_from_classes(k, m, classes)
        words = to_words(got, [k] * len(classes), m)
        for info in (False, True):
            for max_units in (None, 1, 2):
                compare(k, m, words, [k] * len(classes), info=info, max_units=max_units)


@pytest.mark.parametrize("edge", [32, 64])
def test_runs_straddling_word_edges(edge):
    k, m = 64, 32
    blocks = []
    for length in (1, 2, 3, 4):
        for back in range(length + 1):
            start = edge - back
            # (across slot 64 the run lies in the source and the parity: e = m + back, p = m - the rest)
            blocks.append(block_with_runs(k, m, [(start, length), (start + length + 1, 1)]))
    got = np.stack(blocks)
    compare(k, m, to_words(got, [k] * len(blocks), m), [k] * len(blocks))
    compare(k, m, to_words(got, [k] * len(blocks), m), [k] * len(blocks), max_units=1, fec=(129, 8))


def test_erasures_against_m_and_p():
    k, m = 64, 32
    blocks = []
    for e, p in [(m, 0), (m + 1, 0), (m + 1, m), (2, 2), (3, 2), (1, 0), (m, m - 1), (m, m), (k, 0), (k, m), (5, 1)]:
        got = np.ones(k + m, bool)
        got[1:1 + e] = False
        got[k:] = False
        got[k + m - p:] = True
        blocks.append(got)
    got = np.stack(blocks)
    compare(k, m, to_words(got, [k] * len(blocks), m), [k] * len(blocks))


def test_three_blocks_of_c4():
    k, m = 4096, 256
    rng = np.random.default_rng(4)
    got = np.stack([block_with_runs(k, m, [(2047, 3), (2052, 1), (2060, 2), (3000, 700)]),
                    lossy(rng, 1, k, m, 0.5)[0],
                    lossy(rng, 1, k, m, 0.03)[0]])
    got[2, k + 100:] = False
    words = to_words(got, [k, k - 1, k], m, rng=rng)
    compare(k, m, words, [k, k - 1, k], fec=(2, 16))
    compare(k, m, words, [k, k - 1, k], fec=(129, 16), max_units=2)


@pytest.mark.parametrize("nb", [1, TILE - 1, TILE, TILE + 1, 2 * TILE + 3])
def test_scan_tiles(nb):
    """a block-level chain and an open request carried across the scan's tile boundary"""
    k, m = 8, 4
    rng = np.random.default_rng(nb)
    got, nds = mixed(rng, nb, k, m, 0.5)
    if nb > 1:
        # around every tile boundary: absent runs with silent blocks between them and no needing
        # block, so one chain and its open ITEMS request cross it; then a RANGES run across it
        for edge in range(TILE, nb, TILE):
            lo = edge - 9
            got[lo:edge + 9] = False
            nds[lo:edge + 9] = k
            for b in (lo + 2, edge - 3, edge + 2):
                if b < nb:
                    got[b, :k] = True
        if nb > 2 * TILE:
            got[2 * TILE - 3:2 * TILE + 2] = False
    words = to_words(got, nds, m)
    total, totals = compare(k, m, words, nds)
    assert nb == 1 or (totals[2] and totals[3])
    compare(k, m, words, nds, max_units=2, info=True, fec=(129, 8), first=0xFFFFFF00)
    compare(k, m, words, nds, max_units=4000)


def test_capacity_below_the_total_and_buffer_that_ends_its_allocation():
    k, m = 64, 32
    rng = np.random.default_rng(9)
    got, nds = mixed(rng, 50, k, m, 0.6)
    words = to_words(got, nds, m)
    total, _ = compare(k, m, words, nds)
    for cap in (0, 4, 8, total // 2 // 4 * 4, total - 4, total):
        compare(k, m, words, nds, capacity=cap)
    compare(k, m, words, nds, capacity=total // 2 // 4 * 4 + 2)  # a capacity that cuts a dword
    # the content's last byte is the last byte of a 2 MiB tensor
    big = torch.full((2 << 20,), SENTINEL, dtype=torch.uint8, device="cuda")
    compare(k, m, words, nds, content=big[big.numel() - total:])
    assert (big[:big.numel() - total] == SENTINEL).all()


def test_non_default_stream_and_argument_checks():
    k, m = 64, 32
    rng = np.random.default_rng(10)
    got, nds = mixed(rng, 33, k, m, 0.6)
    words = to_words(got, nds, m)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        compare(k, m, words, nds, stream=s)
    dec = codec(k, m)
    dmask = _dev(words)
    for bad in (dict(fec_id=0), dict(fec_id=2, fec_m=4), dict(max_units=0), dict(max_units=65535 // 16 + 1), dict(flags=2)):
        with pytest.raises(norm_amd.NfecError):
            dec.repair_requests(dmask, **bad)
    with pytest.raises(norm_amd.NfecError):
        dec.repair_requests(dmask, content=torch.zeros(64, dtype=torch.uint8, device="cuda")[1:])  # not 4-byte aligned
    with pytest.raises(norm_amd.NfecError):
        dec.repair_requests(_dev(np.zeros((4, 2), np.uint32)))  # a short mask_stride
    _, _, totals = dec.repair_requests(_dev(np.zeros((0, 3), np.uint32)), flags=N.NFEC_NACK_INFO)
    torch.cuda.synchronize()
    assert not totals.cpu().numpy().any()


def test_loopback_until_nothing_is_asked_for():
    """encode -> list / emit -> loss -> ingest -> decode -> repair requests -> the sender's pending
    masks -> list / emit ... until the totals read zero.  Every round loses 45 % of its messages, the
    first one also every message of 7 blocks.  The bound on the rounds: a requested message is lost
    with probability 0.45 a round, so 30 rounds lose one of the ~29,000 with probability below 1e-6;
    every round's content, block_start and totals are the host entry's on the same masks."""
    k, m, vec, nb = 64, 32, 1400, 300
    fec_id, fec_m, first, idlen = 5, 8, 0xFFFF00, 4
    rng = np.random.default_rng(300)
    enc, dec = NormEncoderRS8(), NormDecoderRS8()
    assert enc.Init(k, m, vec) and dec.Init(k, m, vec)
    src = torch.from_numpy(rng.integers(0, 256, (nb, k + m, vec), dtype=np.uint8)).cuda()
    enc.encode_blocks(src)
    rxb = torch.zeros_like(src)
    mask = norm_amd.received_mask(nb, k, m)
    words = (k + m + 31) // 32
    pend = np.zeros((nb, words * 32), bool)
    pend[:, :k + m] = True  # TxInit: everything
    gone = set(int(b) for b in rng.choice(nb, 7, replace=False))
    rounds, asked_blocks, asked_segments = 0, 0, 0
    while True:
        rounds += 1
        assert rounds <= 30
        dpend = _dev(np.packbits(pend.reshape(nb, words, 32), axis=2, bitorder="little").view(np.uint32).reshape(nb, words))
        off, blk, sym, ln, start = enc.list_pending(dpend, gap=idlen)
        count, nbytes = (int(x) for x in _np(start, np.uint64)[nb])
        assert count == int(pend.sum())
        wire = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        enc.emit_segments(src, wire, off, blk, sym, ln, count_dev=start[nb, :1], fec_id=fec_id, fec_m=fec_m,
                          first_block_id=first)
        h_off, h_blk, h_ln = _np(off, np.uint64)[:count], _np(blk, np.uint32)[:count], _np(ln, np.uint16)[:count]
        keep = rng.random(count) >= 0.45
        if rounds == 1:
            keep &= ~np.isin(h_blk, list(gone))
        dec.ingest_messages(rxb, mask, wire, _dev(h_off[keep]), _dev(h_ln[keep]), fec_id, fec_m, first_block_id=first)
        dec.decode_received(rxb, mask)
        content, bstart, totals = dec.repair_requests(mask, fec_id=fec_id, fec_m=fec_m, object_id=7, first_block_id=first)
        torch.cuda.synchronize()
        h_mask = _np(mask, np.uint32)
        h_content, h_bstart, h_totals = norm_amd.rx_repair_requests_host(k, m, h_mask, None, fec_id, fec_m, 7, first)
        t = _np(totals, np.uint64)
        assert np.array_equal(t, h_totals) and np.array_equal(_np(bstart, np.uint64), h_bstart)
        got = content.cpu().numpy()[:int(t[0])]
        assert np.array_equal(got, h_content[:int(t[0])])
        if rounds == 1:
            assert t[3] == 7 and t[2] > 0
        if t[0] == 0:
            break
        # the sender's side: exactly the requested slots become pending, a whole block as TxReset does
        fl, form, lo, hi, consumed = norm_amd.repair_parse_host(fec_id, fec_m, got)
        assert consumed == len(got) and len(fl)
        pend[:] = False
        for i in range(len(fl)):
            b0, b1 = (int(lo[i, 1]) - first) & 0xFFFFFF, (int(hi[i, 1]) - first) & 0xFFFFFF
            assert lo[i, 0] == 7 and b0 <= b1 < nb
            if fl[i] & BLOCK:
                pend[b0:b1 + 1, :k] = True
                asked_blocks += b1 - b0 + 1
            else:
                assert fl[i] & SEGMENT and b0 == b1
                pend[b0, int(lo[i, 3]):int(hi[i, 3]) + 1] = True
                asked_segments += 1
    assert rounds >= 3 and asked_blocks >= 7 and asked_segments
    assert torch.equal(rxb[:, :k], src[:, :k])  # every source byte is the original
