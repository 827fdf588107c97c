"""Receiver assembly on the device: nfec_rx_place, nfec_rx_erasures, nfec_decode_received.

A receiver holds segments in arrival order -- out of order, interleaved across blocks, of any
length up to the vector size and at whatever byte offset the packet header left them -- and NORM's
per-block reception mask.  NormObject::HandleObjectMessage (reference
src/common/normObject.cpp:1548-1644) drops a segment it already has, zero-pads a short one, builds
the erasure list from the mask (:1560-1606) and calls Decode.  These tests hold the device path to
that: placement byte for byte against a NumPy placement, the lists against nfec_rx_erasures_host,
and the repair against the oracle."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import norm_amd  # noqa: E402
from norm_amd import (NFEC_MDP, NFEC_RS8, NFEC_RS16, NormDecoderMDP, NormDecoderRS8, NormDecoderRS16)  # noqa: E402

DEC = {NFEC_RS8: NormDecoderRS8, NFEC_RS16: NormDecoderRS16, NFEC_MDP: NormDecoderMDP}


def _dev(a, signed):
    """a NumPy unsigned array as the signed torch tensor of the same bits, on the GPU"""
    return torch.from_numpy(np.ascontiguousarray(a).view(signed)).cuda()


def _mask_np(t):
    return t.cpu().numpy().view(np.uint32)


class Segments:
    """received segments in arrival order: a payload buffer and the descriptors of each"""

    def __init__(self, rng):
        self.rng = rng
        self.chunks, self.pos = [], 0
        self.off, self.blk, self.sym, self.len, self.data = [], [], [], [], []

    def add(self, b, s, data, residue=None):
        """append a segment whose payload starts at an offset with (offset % 16) == residue"""
        if residue is not None:
            gap = (residue - self.pos) % 16
            self.chunks.append(self.rng.integers(0, 256, gap, dtype=np.uint8))  # gaps hold junk, never zeros
            self.pos += gap
        self.off.append(self.pos)
        self.blk.append(b)
        self.sym.append(s)
        self.len.append(len(data))
        self.data.append(np.asarray(data, np.uint8))
        self.chunks.append(self.data[-1])
        self.pos += len(data)

    def shuffle(self):
        """arrival order differs from the order of the payload buffer"""
        p = self.rng.permutation(len(self.off))
        for name in ("off", "blk", "sym", "len", "data"):
            setattr(self, name, [getattr(self, name)[i] for i in p])

    def payloads(self):
        return np.concatenate(self.chunks) if self.chunks else np.zeros(0, np.uint8)

    def upload(self):
        pay = self.payloads()
        if pay.size == 0:
            pay = np.zeros(16, np.uint8)
        return dict(payloads=torch.from_numpy(pay).cuda(), offsets=_dev(np.array(self.off, np.uint64), np.int64),
                    block_index=_dev(np.array(self.blk, np.uint32), np.int32),
                    symbol_id=_dev(np.array(self.sym, np.uint16), np.int16),
                    length=_dev(np.array(self.len, np.uint16), np.int16))


def numpy_place(batch, mask, segs, k, m, vec, num_data):
    """the placement in NumPy, in arrival order: rejects, duplicates (first copy wins), zero pad"""
    stats = [0, 0, 0]
    nb = batch.shape[0]
    for b, s, data in zip(segs.blk, segs.sym, segs.data):
        nd = (k if num_data is None else int(num_data[b])) if b < nb else 0
        if b >= nb or nd < 1 or nd > k or s >= nd + m or len(data) > vec:
            stats[2] += 1
        elif (int(mask[b, s // 32]) >> (s % 32)) & 1:
            stats[1] += 1
        else:
            stats[0] += 1
            mask[b, s // 32] |= np.uint32(1 << (s % 32))
            batch[b, s, :len(data)] = data
            batch[b, s, len(data):vec] = 0
    return stats


PLACE_SHAPES = [(NFEC_RS8, 8, 2, 24, 24), (NFEC_RS8, 64, 32, 1405, 1408), (NFEC_RS16, 400, 100, 1460, 1464)]


@pytest.mark.parametrize("kind,k,m,vec,stride", PLACE_SHAPES)
def test_place_is_byte_exact(kind, k, m, vec, stride):
    rng = np.random.default_rng(k * 131 + vec)
    nb = 6
    nd = np.array([k, max(1, k // 2), k - 1, 1, k, max(1, k - 3)], np.uint16)
    dec = DEC[kind]()
    assert dec.Init(k, m, vec)
    junk = rng.integers(1, 256, (nb, k + m, stride), dtype=np.uint8)
    # distinct (block, slot) pairs, every block's first and last slot among them
    slots = [(b, s) for b in range(nb) for s in range(int(nd[b]) + m)]
    must = [(b, 0) for b in range(nb)] + [(b, int(nd[b]) + m - 1) for b in range(nb)]
    taken = set(must)
    rest = [p for p in slots if p not in taken]
    want_n = min(len(slots), 16 * 7 + 8)
    pick = must + [rest[i] for i in rng.permutation(len(rest))[:want_n - len(must)]]
    lengths = [0, 1, 7, 8, 9, vec - 1, vec]
    segs = Segments(rng)
    seen = set()
    for j, (b, s) in enumerate(pick):
        # the length classes against every source alignment, then random lengths
        ln = lengths[j % 7] if j < 16 * 7 else int(rng.integers(0, vec + 1))
        res = (j // 7 + 3 * (j % 7)) % 16 if j < 16 * 7 else int(rng.integers(16))
        seen.add((ln, res))
        segs.add(b, s, rng.integers(1, 256, ln, dtype=np.uint8), residue=res)
    assert {r for _, r in seen} == set(range(16)) and {ln for ln, _ in seen} >= set(lengths)
    if len(pick) >= 16 * 7:
        assert all((ln, r) in seen for ln in lengths for r in range(16))
    segs.shuffle()
    want = junk.copy()
    want_mask = np.zeros((nb, (k + m + 31) // 32 + 1), np.uint32)
    want_stats = numpy_place(want, want_mask, segs, k, m, vec, nd)
    assert want_stats == [len(pick), 0, 0]

    dev = torch.from_numpy(junk.copy()).cuda()
    mask = torch.zeros((nb, want_mask.shape[1]), dtype=torch.int32, device="cuda")
    stats = torch.zeros(3, dtype=torch.int32, device="cuda")
    up = segs.upload()
    pay_before = up["payloads"].clone()
    dec.place_segments(dev, mask, num_data=_dev(nd, np.int16), stats=stats, **up)
    torch.cuda.synchronize()
    got = dev.cpu().numpy()
    assert stats.cpu().tolist() == want_stats
    assert np.array_equal(_mask_np(mask), want_mask)
    # placed slots: payload + zero pad up to vec; stride padding and untouched slots keep the junk
    for b, s, data in zip(segs.blk, segs.sym, segs.data):
        assert np.array_equal(got[b, s, :len(data)], data), (b, s, len(data))
        assert not got[b, s, len(data):vec].any(), (b, s, len(data))
        assert np.array_equal(got[b, s, vec:], junk[b, s, vec:]), (b, s, len(data))
    assert np.array_equal(got, want)
    assert torch.equal(up["payloads"], pay_before)


def test_place_rejects_and_duplicates():
    k, m, vec, stride = 64, 32, 1405, 1408
    rng = np.random.default_rng(7)
    nd = np.array([64, 40, 0, 64, 65], np.uint16)
    nb = len(nd)
    dec = NormDecoderRS8()
    assert dec.Init(k, m, vec)
    junk = rng.integers(1, 256, (nb, k + m, stride), dtype=np.uint8)
    first = rng.integers(1, 256, vec - 3, dtype=np.uint8)

    def rnd(n):
        return rng.integers(1, 256, n, dtype=np.uint8)

    one = Segments(rng)
    one.add(0, 5, rnd(vec), residue=3)          # placed
    one.add(nb, 0, rnd(16), residue=1)          # block_index == nblocks
    one.add(1, 40 + m, rnd(16), residue=5)      # symbol_id == nd_b + m on a shortened block
    one.add(1, 40 + m - 1, rnd(11), residue=7)  # ... its last parity slot: placed
    one.add(0, 6, rnd(vec + 1), residue=9)      # length == vec + 1
    one.add(2, 0, rnd(16), residue=11)          # a block with numData 0
    one.add(4, 0, rnd(16), residue=13)          # ... and one with numData k + 1
    one.add(3, 7, first, residue=15)            # the same (b, s) twice, identical bytes: one wins
    one.add(3, 7, first.copy(), residue=2)
    want = junk.copy()
    want_mask = np.zeros((nb, 3), np.uint32)
    s1 = numpy_place(want, want_mask, one, k, m, vec, nd)
    assert s1 == [3, 1, 5]

    dev = torch.from_numpy(junk.copy()).cuda()
    mask = norm_amd.received_mask(nb, k, m)
    assert mask.shape == (nb, 3) and mask.dtype == torch.int32 and not mask.any()
    stats = torch.zeros(3, dtype=torch.int32, device="cuda")
    ndd = _dev(nd, np.int16)
    dec.place_segments(dev, mask, num_data=ndd, stats=stats, **one.upload())
    torch.cuda.synchronize()
    assert stats.cpu().tolist() == s1
    assert np.array_equal(_mask_np(mask), want_mask)
    assert np.array_equal(dev.cpu().numpy(), want)

    two = Segments(rng)
    two.add(3, 7, rnd(vec), residue=4)          # the slot is taken: dropped, whatever it carries
    two.add(0, 6, rnd(9), residue=6)            # placed
    s2 = numpy_place(want, want_mask, two, k, m, vec, nd)
    assert s2 == [1, 1, 0]
    dec.place_segments(dev, mask, num_data=ndd, stats=stats, **two.upload())
    torch.cuda.synchronize()
    got = dev.cpu().numpy()
    assert stats.cpu().tolist() == [4, 2, 5]    # the counters accumulate
    assert np.array_equal(got[3, 7, :vec - 3], first) and not got[3, 7, vec - 3:vec].any()
    assert np.array_equal(_mask_np(mask), want_mask)
    assert np.array_equal(got, want)
    # stats may be omitted; an empty call is fine
    dec.place_segments(dev, mask, num_data=ndd, **two.upload())
    dec.place_segments(dev, mask, num_data=ndd, **Segments(rng).upload())
    torch.cuda.synchronize()
    assert np.array_equal(dev.cpu().numpy(), want) and np.array_equal(_mask_np(mask), want_mask)


def make_masks(k, m, num_data, rng, stride, words):
    """per block one of: all received; only parity missing; one source (and one parity) missing;
    more than m missing; more than `stride` missing; random; stray bits past nd + m on odd rounds"""
    nb = len(num_data)
    mask = np.zeros((nb, words), np.uint32)
    for b in range(nb):
        nd = int(num_data[b])
        ndv = nd if 1 <= nd <= k else k
        n = ndv + m
        have = np.ones(n, bool)
        case = b % 6
        if case == 1:
            have[ndv + rng.choice(m, max(1, m // 2), replace=False)] = False
        elif case == 2:
            have[rng.integers(ndv)] = False
            have[ndv + rng.integers(m)] = False
        elif case == 3:
            have[rng.choice(n, min(n, m + 1), replace=False)] = False
            have[0] = False
        elif case == 4:
            have[rng.choice(n, min(n, stride + 3), replace=False)] = False
            have[ndv - 1] = False
        elif case == 5:
            have = rng.random(n) < 0.7
        bits = np.zeros(words * 32, bool)
        bits[:n] = have
        if (b // 6) % 2 == 1:
            bits[n:] = True
        mask[b] = np.packbits(bits, bitorder="little").view(np.uint32)
    return mask


@pytest.mark.parametrize("kind,k,m,nb", [(NFEC_RS8, 8, 2, 24), (NFEC_RS8, 64, 32, 24), (NFEC_RS16, 400, 100, 24),
                                         (NFEC_RS16, 4096, 256, 3)])
def test_erasure_lists_match_the_host_rule(kind, k, m, nb):
    rng = np.random.default_rng(k + 3 * m)
    dec = DEC[kind]()
    assert dec.Init(k, m, 64)
    if nb == 3:  # C4: 4,352 slots = 136 mask words, three rounds of the scan
        nd = np.array([k, k - 1, 2049], np.uint16)
        words = (k + m + 31) // 32
        mask = np.zeros((nb, words), np.uint32)
        for b in range(nb):
            bits = np.zeros(words * 32, bool)
            bits[:int(nd[b]) + m] = rng.random(int(nd[b]) + m) < (0.5, 0.95, 0.5)[b]
            if b == 0:
                bits[:k] = True  # only parity missing: no list
            mask[b] = np.packbits(bits, bitorder="little").view(np.uint32)
    else:
        nds = [k, 1, k - 1, 0, k + 1, max(1, k // 2), k, k, min(k, 33), k - 1, 1, k]
        nd = np.array((nds * 2)[:nb], np.uint16)
        words = (k + m + 31) // 32 + 1
        mask = make_masks(k, m, nd, rng, m, words)
    dmask, dnd = _dev(mask, np.int32), _dev(nd, np.int16)
    for stride in (m, max(1, m // 2), m + 7):
        hl, hc = norm_amd.erasures_from_received_host(k, m, mask, nd, stride=stride)
        locs, counts = dec.erasures_from_received(dmask, num_data=dnd, stride=stride)
        torch.cuda.synchronize()
        gc = counts.cpu().numpy().view(np.uint16)
        gl = locs.cpu().numpy().view(np.uint16)
        assert np.array_equal(gc, hc), stride
        assert np.array_equal(gl, hl), stride
        assert (hc == 0).any() and (stride > m or (hc > stride).any())  # lists cut at the stride are among them
    assert np.array_equal(_mask_np(dmask), mask)  # read only
    if nb != 3:  # num_data NULL = k
        full = make_masks(k, m, np.full(nb, k, np.uint16), rng, m, words)
        hl, hc = norm_amd.erasures_from_received_host(k, m, full)
        locs, counts = dec.erasures_from_received(_dev(full, np.int32))
        torch.cuda.synchronize()
        assert np.array_equal(counts.cpu().numpy().view(np.uint16), hc)
        assert np.array_equal(locs.cpu().numpy().view(np.uint16), hl)


def _oracle_decode(orc, kind, k, m, vec, blocks, locs, counts, nd):
    """the oracle's Decode per block; more than m erasures cannot be decoded: status 0, block as it
    is (the reference's decoding matrix cannot be built, normEncoderRS8.cpp:721-725)"""
    st = np.zeros(len(blocks), np.int32)
    for i in range(len(blocks)):
        if counts[i] > m:
            continue
        one = blocks[i:i + 1].copy()
        l1 = np.zeros((1, m), np.uint16)
        l1[0, :counts[i]] = locs[i, :counts[i]]
        st[i] = orc.decode_blocks(kind, k, m, vec, one, l1, counts[i:i + 1], nd[i:i + 1])[0]
        blocks[i] = one[0]
    return st


E2E = [
    # kind, k, m, vec, seg stride, the decode path the batch takes
    (NFEC_RS8, 64, 32, 1400, 1400, "fixed"),
    (NFEC_RS8, 16, 4, 100, 104, "runtime"),
    (NFEC_MDP, 64, 32, 1400, 1400, None),
    (NFEC_RS16, 400, 100, 1460, 1464, None),
]


@pytest.mark.parametrize("kind,k,m,vec,stride,path", E2E)
def test_place_then_decode_received(orc, kind, k, m, vec, stride, path):
    rng = np.random.default_rng(k * 17 + m + vec)
    nb = 24
    nd = np.full(nb, k, np.uint16)
    nd[[1, 6, 17, 21, 23]] = [k - 1, max(1, k // 2), k - 1, max(1, k - 5), max(1, k // 3)]
    host = orc.make_blocks(k, m, vec, nb, seg_stride=stride, num_data=nd)
    for b in range(nb):  # some source segments end in zeros: they arrive short
        for s in range(b % 5, int(nd[b]), 5):
            host[b, s, vec // 2 + s:] = 0
    clean = orc.encode_blocks(kind, k, m, vec, host, nd)
    # the loss plan: blocks 0-15 lose 1..m segments (at least one of them source), 16-19 nothing,
    # 20-23 m + 1 (undecodable)
    lost = []
    for b in range(nb):
        n = int(nd[b])
        if b < 16:
            e = int(rng.integers(1, m + 1)) if b else m       # block 0: all the parity can repair
            es = min(n, int(rng.integers(1, e + 1)))
            ep = min(m, e - es)
            miss = np.concatenate([rng.choice(n, es, replace=False), n + rng.choice(m, ep, replace=False)])
        elif b < 20:
            miss = np.zeros(0, np.int64)
        else:
            miss = rng.choice(n + m, m + 1, replace=False)
            if (miss >= n).all():
                miss[0] = 0
        lost.append(set(int(x) for x in miss))
    # what arrives: everything else, each segment at its own misaligned offset; a segment whose tail
    # is zeros may arrive short (NORM sends the last segment of an object short)
    segs = Segments(rng)
    for b in range(nb):
        for s in range(int(nd[b]) + m):
            if s not in lost[b]:
                data = clean[b, s, :vec]
                if s % 5 == b % 5:
                    data = np.trim_zeros(data, "b")
                segs.add(b, s, data, residue=int(rng.integers(16)))
    segs.shuffle()
    junk = rng.integers(1, 256, clean.shape, dtype=np.uint8)
    dec = DEC[kind]()
    assert dec.Init(k, m, vec)
    dev = torch.from_numpy(junk.copy()).cuda()
    mask = norm_amd.received_mask(nb, k, m)
    stats = torch.zeros(3, dtype=torch.int32, device="cuda")
    ndd = _dev(nd, np.int16)
    dec.place_segments(dev, mask, num_data=ndd, stats=stats, **segs.upload())
    torch.cuda.synchronize()
    placed = dev.cpu().numpy()
    assert stats.cpu().tolist() == [len(segs.off), 0, 0]
    for b in range(nb):
        for s in range(int(nd[b]) + m):
            if s in lost[b]:
                assert np.array_equal(placed[b, s], junk[b, s])
            else:
                assert np.array_equal(placed[b, s, :vec], clean[b, s, :vec])
    # the lists the mask stands for, and the oracle's Decode on them (erased source zero-filled, as
    # NORM hands it over, normObject.cpp:1579)
    hmask = _mask_np(mask)
    locs, counts = norm_amd.erasures_from_received_host(k, m, hmask, nd, stride=m + 1)
    for b in range(nb):
        src_lost = sorted(s for s in lost[b] if s < nd[b])
        want = (src_lost + sorted(s for s in lost[b] if s >= nd[b])) if src_lost else []
        assert counts[b] == len(want) and locs[b, :len(want)].tolist() == want
    ref = placed.copy()
    for b in range(nb):
        for s in locs[b, :counts[b]]:
            if s < nd[b]:
                ref[b, s, :vec] = 0
    st_ref = _oracle_decode(orc, kind, k, m, vec, ref, locs, counts, nd)
    assert (st_ref[:20] == counts[:20]).all() and not st_ref[20:].any()

    # the same batch through decode_blocks with explicit lists: which family it takes, and its bytes
    twin = torch.from_numpy(placed.copy()).cuda()
    before = dec.decode_paths()
    st_twin = dec.decode_blocks(twin, _dev(locs[:, :m].copy(), np.int16), _dev(counts, np.int16), num_data=ndd)
    torch.cuda.synchronize()
    mid = dec.decode_paths()
    st = dec.decode_received(dev, mask, num_data=ndd)
    torch.cuda.synchronize()
    after = dec.decode_paths()
    took_twin = {p: mid[p] - before[p] for p in mid if mid[p] != before[p]}
    took = {p: after[p] - mid[p] for p in after if after[p] != mid[p]}
    assert took == took_twin and sum(took.values()) == 1, (took, took_twin)
    assert path is None or took == {path: 1}, took
    got = dev.cpu().numpy()
    stg = st.cpu().numpy()
    assert np.array_equal(stg, st_ref), (stg, st_ref)
    assert np.array_equal(stg, st_twin.cpu().numpy())
    assert np.array_equal(_mask_np(mask), hmask)  # the mask is only read
    cov = vec & ~1 if kind == NFEC_RS16 else vec
    for b in range(20):
        n = int(nd[b])
        assert np.array_equal(got[b, :n, :cov], clean[b, :n, :cov]), b
        assert np.array_equal(got[b, :n, :cov], ref[b, :n, :cov]), b
    for b in range(20, nb):
        assert stg[b] == 0 and np.array_equal(got[b], placed[b]), b
    # nothing but erased source slots is written: parity, junk in lost parity slots, stride padding
    for b in range(20):
        for s in range(k + m):
            if not (s in lost[b] and s < nd[b]):
                assert np.array_equal(got[b, s], placed[b, s]), (b, s)
    assert np.array_equal(got, twin.cpu().numpy())
