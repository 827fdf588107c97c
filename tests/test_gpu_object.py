"""Object segmentation on the device: nfec_object_read and nfec_object_write.

The sender fills a block's source slots from its NORM data object with NormDataObject::ReadSegment
(reference src/common/normObject.cpp:2673-2718) and pads them with zeros before it encodes
(CalculateBlockParity, :2203-2229); the receiver delivers every received source segment (:1529) and,
after a successful Decode, every repaired one (:1616) with WriteSegment (:2628-2670).  These tests
hold the two device entries to that byte for byte: expected bytes come from NumPy loops over
nfec_object_segment (itself held to a restatement of the reference in tests/test_object_host.py),
everything a call must not write keeps a -86 fill, and the whole chain object -> blocks -> parity ->
wire -> blocks -> repair -> object returns the object."""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import norm_amd  # noqa: E402
from norm_amd import _native as N  # noqa: E402
from norm_amd import (NFEC_RS8, NFEC_RS16, NormDecoderRS8, NormDecoderRS16, NormEncoderRS8,  # noqa: E402
                      NormEncoderRS16)

ENC = {NFEC_RS8: NormEncoderRS8, NFEC_RS16: NormEncoderRS16}
DEC = {NFEC_RS8: NormDecoderRS8, NFEC_RS16: NormDecoderRS16}
FILL = 0xAA  # -86
GUARD = 64
BASES = (0, 1, 4, 8, 15)

# kind, k, m, segment_size, vector, seg_stride, blocks.  1,392 and 1,452 are more than 64 pieces per
# segment; k = 200 and k = 4,096 have runs past 64 segments and several runs per block
SHAPES = [
    (NFEC_RS8, 8, 2, 48, 56, 56, 5),
    (NFEC_RS8, 8, 2, 37, 45, 48, 7),
    (NFEC_RS8, 8, 2, 1, 9, 16, 3),
    (NFEC_RS8, 64, 32, 1392, 1400, 1400, 6),
    (NFEC_RS8, 64, 32, 1452, 1460, 1472, 4),
    (NFEC_RS8, 200, 55, 100, 108, 112, 3),
    (NFEC_RS16, 4096, 256, 56, 64, 64, 3),
]
IDS = ["%d-%d-%d" % (s[1], s[3], s[5]) for s in SHAPES]


@functools.lru_cache(maxsize=None)
def codec(kind, k, m, vec, decoder=False):
    c = (DEC if decoder else ENC)[kind]()
    assert c.Init(k, m, vec)
    return c


def finals(seg):
    """final segment sizes: 1 byte, segment_size - 1 and exactly segment_size"""
    return sorted({1, max(1, seg - 1), seg})


def layout_for(k, seg, nb, fin):
    """nb blocks, the first nb - nb // 2 of k segments and the rest of k - 1, the last segment of fin bytes"""
    nseg = nb * k - nb // 2
    lay = norm_amd.object_layout((nseg - 1) * seg + fin, seg, k)
    assert lay.num_blocks == nb and lay.final_segment_size == fin
    assert (lay.large_block_count, lay.small_block_count) == (nb - nb // 2, nb // 2)
    assert (lay.large_block_size, lay.small_block_size) == (k, k - 1)
    return lay


@functools.lru_cache(maxsize=None)
def _segments(size, seg, k):
    lay = norm_amd.object_layout(size, seg, k)
    sizes = norm_amd.object_block_sizes(lay, 0, lay.num_blocks)
    return [[norm_amd.object_segment(lay, b, s) for s in range(int(sizes[b]))] for b in range(lay.num_blocks)]


def segments(lay):
    """[block][segment] -> (offset, length), from nfec_object_segment"""
    return _segments(lay.object_size, lay.segment_size, lay.num_data)


def dev_object(content, base, tail=GUARD):
    """content at `base` bytes past a 64-byte guard in a fresh tensor; returns (whole tensor, the object's view)"""
    buf = np.full(GUARD + base + len(content) + tail, FILL, np.uint8)
    buf[GUARD + base:GUARD + base + len(content)] = content
    whole = torch.from_numpy(buf).cuda()
    return whole, whole[GUARD + base:GUARD + base + len(content)]


def dev_batch(host):
    """host batch [nb, slots, stride] between two guard blocks of fill"""
    nb = host.shape[0]
    buf = np.full((nb + 2,) + host.shape[1:], FILL, np.uint8)
    buf[1:nb + 1] = host
    whole = torch.from_numpy(buf).cuda()
    return whole, whole[1:nb + 1]


def expect_read(obj, lay, first, nb, slots, stride, vec):
    want = np.full((nb, slots, stride), FILL, np.uint8)
    segs = segments(lay)
    for i in range(nb):
        for s, (off, ln) in enumerate(segs[first + i]):
            want[i, s, :ln] = obj[off:off + ln]
            want[i, s, ln:vec] = 0
    return want


def expect_write(batch, lay, first, nbytes, selected=None):
    """the object buffer (nbytes of it, fill elsewhere) after the selected segments were written"""
    want = np.full(nbytes, FILL, np.uint8)
    segs = segments(lay)
    for i in range(batch.shape[0]):
        for s, (off, ln) in enumerate(segs[first + i]):
            if selected is not None and not selected[i][s]:
                continue
            if off >= nbytes:
                continue
            ln = min(ln, nbytes - off)
            want[off:off + ln] = batch[i, s, :ln]
    return want


def windows(lay):
    """(first_block, nblocks): the whole object, and a window that crosses the large/small boundary and
    ends at the final block"""
    first = max(1, lay.large_block_count - 1)
    return [(0, lay.num_blocks), (first, lay.num_blocks - first)]


@pytest.mark.parametrize("kind,k,m,seg,vec,stride,nb", SHAPES, ids=IDS)
def test_read_is_byte_exact(kind, k, m, seg, vec, stride, nb):
    rng = np.random.default_rng(k * 7 + seg)
    enc = codec(kind, k, m, vec)
    for n, (fin, base) in enumerate((f, b) for f in finals(seg) for b in BASES):
        lay = layout_for(k, seg, nb, fin)
        obj = rng.integers(1, 256, lay.object_size, dtype=np.uint8)
        whole_obj, dobj = dev_object(obj, base)
        before = whole_obj.cpu().numpy()
        for first, count in windows(lay) if n % 2 == 0 else windows(lay)[:1]:
            whole, dbatch = dev_batch(np.full((count, k + m, stride), FILL, np.uint8))
            nd_all = torch.full((count + 2,), -21846, dtype=torch.int16, device="cuda")  # 0xAAAA
            lens = torch.full((count, k + 3), -21846, dtype=torch.int16, device="cuda")
            enc.read_object(dobj, lay, dbatch, first_block=first, num_data=nd_all[1:count + 1], seg_length=lens)
            torch.cuda.synchronize()
            got = whole.cpu().numpy()
            want = expect_read(obj, lay, first, count, k + m, stride, vec)
            bad = np.argwhere(got[1:count + 1] != want)
            assert bad.size == 0, (fin, base, first, bad[:4], len(bad))
            assert (got[0] == FILL).all() and (got[count + 1] == FILL).all()  # the guard blocks
            sizes = norm_amd.object_block_sizes(lay, first, count)
            got_nd = nd_all.cpu().numpy().view(np.uint16)
            assert np.array_equal(got_nd[1:count + 1], sizes) and got_nd[0] == 0xAAAA and got_nd[-1] == 0xAAAA
            got_len = lens.cpu().numpy().view(np.uint16)
            for i in range(count):
                want_len = [ln for _, ln in segments(lay)[first + i]]
                assert got_len[i, :len(want_len)].tolist() == want_len, (fin, base, i)
                assert (got_len[i, len(want_len):] == 0xAAAA).all()
        # without the optional outputs, and the object is only read
        whole, dbatch = dev_batch(np.full((nb, k + m, stride), FILL, np.uint8))
        enc.read_object(dobj, lay, dbatch)
        torch.cuda.synchronize()
        assert np.array_equal(whole.cpu().numpy()[1:nb + 1], expect_read(obj, lay, 0, nb, k + m, stride, vec))
        assert np.array_equal(whole_obj.cpu().numpy(), before)


def random_selection(rng, lay, first, count, k, m, words):
    """a random reception mask (junk in the bits past the source slots too), a random status (0 or
    positive) and the selection they make"""
    mask = rng.integers(0, 1 << 32, (count, words), dtype=np.uint64).astype(np.uint32)
    status = np.where(rng.random(count) < 0.3, rng.integers(1, m + 1, count), 0).astype(np.int32)
    if count > 1:
        status[0], status[1] = 0, 2
    sel = [[bool(status[i] > 0 or (mask[i, s // 32] >> np.uint32(s % 32)) & 1) for s in range(len(segs))]
           for i, segs in enumerate(segments(lay)[first:first + count])]
    return mask, status, sel


@pytest.mark.parametrize("kind,k,m,seg,vec,stride,nb", SHAPES, ids=IDS)
def test_write_is_byte_exact(kind, k, m, seg, vec, stride, nb):
    rng = np.random.default_rng(k * 11 + seg)
    dec = codec(kind, k, m, vec, True)
    words = (k + m + 31) // 32 + 1
    for n, (fin, base) in enumerate((f, b) for f in finals(seg) for b in BASES):
        lay = layout_for(k, seg, nb, fin)
        size = lay.object_size
        for first, count in windows(lay) if n % 2 == 0 else windows(lay)[:1]:
            batch = rng.integers(1, 256, (count, k + m, stride), dtype=np.uint8)
            dbatch = torch.from_numpy(batch).cuda()
            # every segment
            whole, dobj = dev_object(np.full(size, FILL, np.uint8), base)
            dec.write_object(dobj, lay, dbatch, first_block=first)
            torch.cuda.synchronize()
            got = whole.cpu().numpy()
            want = expect_write(batch, lay, first, size)
            assert (got[:GUARD + base] == FILL).all() and (got[GUARD + base + size:] == FILL).all()
            bad = np.nonzero(got[GUARD + base:GUARD + base + size] != want)[0]
            assert bad.size == 0, (fin, base, first, bad[:8], len(bad))
            # a random mask and status: exactly the selected segments change
            mask, status, sel = random_selection(rng, lay, first, count, k, m, words)
            dmask = torch.from_numpy(mask.view(np.int32)).cuda()
            dstatus = torch.from_numpy(status).cuda()
            stats = torch.zeros(2, dtype=torch.int32, device="cuda")
            whole, dobj = dev_object(np.full(size, FILL, np.uint8), base)
            dec.write_object(dobj, lay, dbatch, first_block=first, received=dmask, status=dstatus, stats=stats)
            torch.cuda.synchronize()
            got = whole.cpu().numpy()
            want = expect_write(batch, lay, first, size, sel)
            assert (got[:GUARD + base] == FILL).all() and (got[GUARD + base + size:] == FILL).all()
            bad = np.nonzero(got[GUARD + base:GUARD + base + size] != want)[0]
            assert bad.size == 0, (fin, base, first, bad[:8], len(bad))
            picked = sum(sum(row) for row in sel)
            total = sum(len(row) for row in sel)
            assert 0 < picked < total
            assert stats.cpu().tolist() == [picked, total - picked]
            # the mask alone (status NULL)
            sel_m = [[bool((mask[i, s // 32] >> np.uint32(s % 32)) & 1) for s in range(len(row))]
                     for i, row in enumerate(sel)]
            whole, dobj = dev_object(np.full(size, FILL, np.uint8), base)
            dec.write_object(dobj, lay, dbatch, first_block=first, received=dmask)
            torch.cuda.synchronize()
            got = whole.cpu().numpy()
            assert np.array_equal(got[GUARD + base:GUARD + base + size], expect_write(batch, lay, first, size, sel_m))
            # the batch and the mask are only read
            assert np.array_equal(dbatch.cpu().numpy(), batch)
            assert np.array_equal(dmask.cpu().numpy().view(np.uint32), mask)


@pytest.mark.parametrize("kind,k,m,seg,vec,stride,nb", SHAPES, ids=IDS)
def test_write_clamps_at_object_bytes(kind, k, m, seg, vec, stride, nb):
    """WriteSegment:2664-2667: a buffer that ends inside a segment, at a segment's start, and inside the
    final segment; nothing past it is written"""
    rng = np.random.default_rng(k * 13 + seg)
    dec = codec(kind, k, m, vec, True)
    fin = max(1, seg - 1)
    lay = layout_for(k, seg, nb, fin)
    size = lay.object_size
    segs = segments(lay)
    off_mid, len_mid = segs[nb // 2][3]
    cuts = {off_mid + (len_mid + 1) // 2, off_mid, segs[1][0][0], size - (fin + 1) // 2, 1}
    batch = rng.integers(1, 256, (nb, k + m, stride), dtype=np.uint8)
    dbatch = torch.from_numpy(batch).cuda()
    for n, cut in enumerate(sorted(cuts)):
        assert 0 < cut <= size
        base = BASES[n % len(BASES)]
        # the object tensor ends at `cut`; what follows it in the allocation is guard
        whole, dobj = dev_object(np.full(cut, FILL, np.uint8), base, tail=2 * vec + GUARD)
        stats = torch.zeros(2, dtype=torch.int32, device="cuda")
        dec.write_object(dobj, lay, dbatch, stats=stats)
        torch.cuda.synchronize()
        got = whole.cpu().numpy()
        assert np.array_equal(got[GUARD + base:GUARD + base + cut], expect_write(batch, lay, 0, cut)), cut
        assert (got[:GUARD + base] == FILL).all() and (got[GUARD + base + cut:] == FILL).all(), cut
        assert stats.cpu().tolist() == [lay.num_segments, 0]


@pytest.mark.parametrize("kind,k,m,seg,vec,stride,nb", SHAPES, ids=IDS)
def test_write_after_read_is_the_identity(kind, k, m, seg, vec, stride, nb):
    rng = np.random.default_rng(k * 17 + seg)
    enc = codec(kind, k, m, vec)
    for fin, base_in, base_out in zip(finals(seg) * 2, (15, 0, 1, 8, 4, 3), (0, 15, 9, 8, 1, 4)):
        lay = layout_for(k, seg, nb, fin)
        obj = rng.integers(0, 256, lay.object_size, dtype=np.uint8)
        _, dobj = dev_object(obj, base_in)
        dbatch = torch.full((nb, k + m, stride), FILL, dtype=torch.uint8, device="cuda")
        whole, dout = dev_object(np.full(lay.object_size, FILL, np.uint8), base_out)
        enc.read_object(dobj, lay, dbatch)
        enc.write_object(dout, lay, dbatch)
        torch.cuda.synchronize()
        got = whole.cpu().numpy()
        assert np.array_equal(got[GUARD + base_out:GUARD + base_out + lay.object_size], obj)
        assert (got[:GUARD + base_out] == FILL).all() and (got[GUARD + base_out + lay.object_size:] == FILL).all()


def test_argument_errors_launch_nothing():
    k, m, seg, vec, stride, nb = 8, 2, 37, 45, 48, 7
    enc = codec(NFEC_RS8, k, m, vec)
    lay = layout_for(k, seg, nb, 5)
    L = N.lib()
    obj = torch.full((lay.object_size + 16,), FILL, dtype=torch.uint8, device="cuda")
    dbatch = torch.full((nb, k + m, stride), FILL, dtype=torch.uint8, device="cuda")
    nd = torch.full((nb,), -21846, dtype=torch.int16, device="cuda")
    lens = torch.full((nb, k), -21846, dtype=torch.int16, device="cuda")
    mask = torch.zeros((nb, 1), dtype=torch.int32, device="cuda")
    stats = torch.zeros(2, dtype=torch.int32, device="cuda")
    b = N.BlockBatch()
    b.blocks, b.block_stride, b.seg_stride, b.nblocks = dbatch.data_ptr(), (k + m) * stride, stride, nb
    pl, pb = ctypes.byref(lay), ctypes.byref(b)
    stream = torch.cuda.current_stream().cuda_stream
    E = N.NFEC_EINVAL

    def read(codec_=enc._h, layout=pl, o=obj.data_ptr(), nbytes=lay.object_size, first=0, batch=pb, ls=k):
        return L.nfec_object_read(codec_, layout, o, nbytes, first, batch, nd.data_ptr(), lens.data_ptr(), ls, stream)

    def write(codec_=enc._h, layout=pl, o=obj.data_ptr(), nbytes=lay.object_size, first=0, batch=pb, ms=1):
        return L.nfec_object_write(codec_, layout, o, nbytes, first, batch, mask.data_ptr(), ms, None,
                                   stats.data_ptr(), stream)

    other_k = norm_amd.object_layout(lay.object_size, seg, k - 1)
    wide = norm_amd.object_layout(lay.object_size, vec + 1, k)
    for call in (read, write):
        assert call(codec_=None) == E and call(layout=None) == E and call(o=None) == E and call(batch=None) == E
        assert call(layout=ctypes.byref(other_k)) == E  # layout->num_data != k
        assert call(layout=ctypes.byref(wide)) == E     # segment_size > vector_size
        assert call(first=1) == E                       # first_block + nblocks > num_blocks
        b.blocks = None
        assert call() == E
        b.blocks = dbatch.data_ptr()
        b.seg_stride = stride - 4                       # not a multiple of 8
        assert call() == E
        b.seg_stride = 40                               # below vector_size
        assert call() == E
        b.seg_stride = stride
    assert read(nbytes=lay.object_size - 1) == E        # ReadSegment would return 0
    assert read(ls=k - 1) == E                          # length_stride < k
    assert write(ms=0) == E                             # (k + m + 31) / 32 == 1
    if torch.cuda.device_count() > 1:                   # object and batch on different devices
        far = torch.full((lay.object_size,), FILL, dtype=torch.uint8, device="cuda:1")
        assert read(o=far.data_ptr()) == E and write(o=far.data_ptr()) == E
    # zero blocks: NFEC_OK, nothing launched
    b.nblocks = 0
    assert read() == N.NFEC_OK and write() == N.NFEC_OK
    torch.cuda.synchronize()
    for t in (obj, dbatch):
        assert (t == FILL).all().item()
    assert (nd == -21846).all().item() and (lens == -21846).all().item()
    assert not mask.any().item() and not stats.any().item()
    # and the well-formed calls pass
    b.nblocks = nb
    assert read() == N.NFEC_OK and write(ms=1) == N.NFEC_OK
    torch.cuda.synchronize()
    assert stats.cpu().tolist() == [0, lay.num_segments]  # an empty mask selects nothing


def identity_descriptors(lay, first, count):
    """the parent commit's route: one descriptor per source segment, its offset the object's"""
    rows = [(off, i, s, ln) for i in range(count) for s, (off, ln) in enumerate(segments(lay)[first + i])]
    off, blk, sym, ln = zip(*rows)
    return (torch.from_numpy(np.array(off, np.int64)).cuda(), torch.from_numpy(np.array(blk, np.int32)).cuda(),
            torch.from_numpy(np.array(sym, np.int16)).cuda(), torch.from_numpy(np.array(ln, np.int16)).cuda())


@pytest.mark.parametrize("kind,k,m,seg,vec,stride,nb", [SHAPES[1], SHAPES[3]], ids=[IDS[1], IDS[3]])
def test_equals_the_assembly_calls(kind, k, m, seg, vec, stride, nb):
    """read_object against place_segments fed with identity descriptors on a zeroed mask, and
    write_object(received=None) against emit_segments without a payload ID at the object's offsets"""
    rng = np.random.default_rng(k * 23 + seg)
    enc, dec = codec(kind, k, m, vec), codec(kind, k, m, vec, True)
    for fin, base in zip(finals(seg), (1, 15, 8)):
        lay = layout_for(k, seg, nb, fin)
        obj = rng.integers(1, 256, lay.object_size, dtype=np.uint8)
        _, dobj = dev_object(obj, base)
        desc = identity_descriptors(lay, 0, nb)
        dnd = torch.from_numpy(norm_amd.object_block_sizes(lay, 0, nb).view(np.int16)).cuda()
        mine = torch.full((nb, k + m, stride), FILL, dtype=torch.uint8, device="cuda")
        theirs = mine.clone()
        enc.read_object(dobj, lay, mine)
        mask = norm_amd.received_mask(nb, k, m)
        dec.place_segments(theirs, mask, dobj, *desc, num_data=dnd)
        torch.cuda.synchronize()
        assert torch.equal(mine, theirs)
        batch = torch.from_numpy(rng.integers(1, 256, (nb, k + m, stride), dtype=np.uint8)).cuda()
        whole_a, out_a = dev_object(np.full(lay.object_size, FILL, np.uint8), base)
        whole_b, out_b = dev_object(np.full(lay.object_size, FILL, np.uint8), base)
        dec.write_object(out_a, lay, batch)
        enc.emit_segments(batch, out_b, *desc, fec_id=0, num_data=dnd)
        torch.cuda.synchronize()
        assert torch.equal(whole_a, whole_b)


@pytest.mark.parametrize("k,m,seg,vec,stride,nb", [(64, 32, 1392, 1400, 1400, 6), (8, 2, 37, 45, 48, 7)])
def test_whole_chain_returns_the_object(orc, k, m, seg, vec, stride, nb):
    """object -> blocks -> parity -> wire -> loss -> blocks -> repair -> object on the device"""
    rng = np.random.default_rng(k * 29 + seg)
    enc, dec = codec(NFEC_RS8, k, m, vec), codec(NFEC_RS8, k, m, vec, True)
    lay = layout_for(k, seg, nb, seg - 1)
    size = lay.object_size
    obj = rng.integers(1, 256, size, dtype=np.uint8)
    _, dobj = dev_object(obj, 5)
    sizes = norm_amd.object_block_sizes(lay, 0, nb)
    gap, fec_id, fec_m = 13, 5, 8
    # sender: read, encode, list, emit; num_data and seg_length come from the read
    dev = torch.zeros((nb, k + m, stride), dtype=torch.uint8, device="cuda")
    dnd = torch.zeros(nb, dtype=torch.int16, device="cuda")
    dlens = torch.zeros((nb, k), dtype=torch.int16, device="cuda")
    enc.read_object(dobj, lay, dev, num_data=dnd, seg_length=dlens)
    enc.encode_blocks(dev, num_data=dnd)
    words = (k + m + 31) // 32
    pend = np.zeros((nb, words), np.uint32)
    for b in range(nb):
        for s in range(int(sizes[b]) + m):
            pend[b, s // 32] |= np.uint32(1 << (s % 32))
    dpend = torch.from_numpy(pend.view(np.int32)).cuda()
    off, blk, sym, ln, start = enc.list_pending(dpend, num_data=dnd, seg_length=dlens, gap=gap)
    count = int(sizes.sum()) + nb * m
    nbytes = count * gap + size + nb * m * seg  # parity goes out at the block's longest source segment
    wire = torch.from_numpy(rng.integers(1, 256, nbytes + 40, dtype=np.uint8)).cuda()
    enc.emit_segments(dev, wire, off, blk, sym, ln, count_dev=start[nb, :1], fec_id=fec_id, fec_m=fec_m,
                      pending=dpend, num_data=dnd)
    torch.cuda.synchronize()
    assert np.array_equal(dnd.cpu().numpy().view(np.uint16), sizes)
    assert start.cpu().numpy().view(np.uint64)[nb].tolist() == [count, nbytes]
    # the parity of one large and one small block against the oracle
    sent = dev.cpu().numpy()
    for b in (0, nb - 1):
        ref = sent[b:b + 1].copy()
        ref[0, int(sizes[b]):] = 0
        orc.encode_blocks(orc.RS8, k, m, vec, ref, num_data=sizes[b:b + 1])
        n = int(sizes[b])
        assert np.array_equal(sent[b, n:n + m, :vec], ref[0, n:n + m, :vec]), b
    # the loss: block b loses lost[b] source segments, one of them more than the parity repairs; the
    # final block loses its short last segment
    h_off, h_blk, h_sym, h_ln = [t.cpu().numpy()[:count] for t in (off, blk, sym, ln)]
    lost = [(b * 5 + 1) % (m + 1) for b in range(nb)]
    lost[0], lost[2], lost[nb - 1] = 0, m + 1, max(1, lost[nb - 1])
    keep = np.ones(count, bool)
    missing = set()
    for b in range(nb):
        src = np.nonzero((h_blk == b) & (h_sym < sizes[b]))[0]
        drop = rng.choice(src, lost[b], replace=False)
        if b == nb - 1 and src[-1] not in drop:
            drop[0] = src[-1]
        keep[drop] = False
        if lost[b] > m:
            missing |= {(b, int(h_sym[i])) for i in drop}
    order = rng.permutation(np.nonzero(keep)[0])
    # receiver: place, repair, deliver
    dev2 = torch.from_numpy(rng.integers(1, 256, sent.shape, dtype=np.uint8)).cuda()
    mask = norm_amd.received_mask(nb, k, m)
    up = [torch.from_numpy(np.ascontiguousarray(a[order])).cuda() for a in (h_off, h_blk, h_sym, h_ln)]
    dec.place_segments(dev2, mask, wire, *up, num_data=dnd)
    st = dec.decode_received(dev2, mask, num_data=dnd)
    whole, dout = dev_object(np.full(size, FILL, np.uint8), 11)
    stats = torch.zeros(2, dtype=torch.int32, device="cuda")
    dec.write_object(dout, lay, dev2, received=mask, status=st, stats=stats)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [n if n <= m else 0 for n in lost]
    want = obj.copy()
    for b, s in missing:
        o, n = segments(lay)[b][s]
        want[o:o + n] = FILL
    got = whole.cpu().numpy()
    assert len(missing) == m + 1
    assert np.array_equal(got[GUARD + 11:GUARD + 11 + size], want)
    assert (got[:GUARD + 11] == FILL).all() and (got[GUARD + 11 + size:] == FILL).all()
    assert stats.cpu().tolist() == [lay.num_segments - (m + 1), m + 1]


def test_multi_device_codec_runs_where_the_batch_is():
    k, m, seg, vec, stride, nb = 8, 2, 37, 45, 48, 7
    enc = NormEncoderRS8(devices=[0, 0])
    assert enc.Init(k, m, vec)
    assert enc.num_devices() == [0, 0]
    rng = np.random.default_rng(3)
    lay = layout_for(k, seg, nb, 36)
    obj = rng.integers(1, 256, lay.object_size, dtype=np.uint8)
    _, dobj = dev_object(obj, 1)
    whole, dbatch = dev_batch(np.full((nb, k + m, stride), FILL, np.uint8))
    enc.read_object(dobj, lay, dbatch)
    out_whole, dout = dev_object(np.full(lay.object_size, FILL, np.uint8), 15)
    enc.write_object(dout, lay, dbatch)
    torch.cuda.synchronize()
    assert np.array_equal(whole.cpu().numpy()[1:nb + 1], expect_read(obj, lay, 0, nb, k + m, stride, vec))
    assert np.array_equal(out_whole.cpu().numpy()[GUARD + 15:GUARD + 15 + lay.object_size], obj)
