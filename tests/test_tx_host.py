"""Sender assembly, the parts that need no GPU: the ABI of the new entries, the host form of the
transmission-list rule (nfec_tx_list_host) against a plain-loop restatement of
NormObject::NextSenderMsg's walk (ref_tx_list below; reference src/common/normObject.cpp:1877,
:1989, :2035, :2050, :2071), and the argument / device checks of the device entries on a host-only
codec."""
import ctypes

import numpy as np
import pytest

import norm_amd
from norm_amd import NormEncoderRS8
from norm_amd import _native as N

NEW = ("nfec_tx_list", "nfec_tx_list_host", "nfec_tx_emit")


def ref_tx_list(k, m, vec, mask, num_data, seg_length, gap, capacity):
    """a plain loop over blocks and slots; arrays of `capacity` entries, zero past the list"""
    nb = mask.shape[0]
    off = np.zeros(capacity, np.uint64)
    blk = np.zeros(capacity, np.uint32)
    sym = np.zeros(capacity, np.uint16)
    ln = np.zeros(capacity, np.uint16)
    start = np.zeros((nb + 1, 2), np.uint64)
    count = nbytes = 0
    for b in range(nb):
        start[b] = (count, nbytes)
        nd = k if num_data is None else int(num_data[b])
        if nd < 1 or nd > k:
            continue
        if seg_length is None:
            seg_size_max = vec
        else:
            seg_size_max = max(int(seg_length[b, s]) for s in range(nd))
        row = [int(w) for w in mask[b]]
        for s in range(nd + m):
            if not (row[s // 32] >> (s % 32)) & 1:
                continue
            if s >= nd:
                length = seg_size_max
            elif seg_length is None:
                length = vec
            else:
                length = int(seg_length[b, s])
            if count < capacity:
                off[count], blk[count], sym[count], ln[count] = nbytes + gap, b, s, length
            count += 1
            nbytes += gap + length
    start[nb] = (count, nbytes)
    return off, blk, sym, ln, start


def _set(mask, b, slots):
    for s in slots:
        mask[b, s // 32] |= np.uint32(1 << (s % 32))


ROWS = 6  # the kinds of mask row below


def num_data_for(k, nb, variant):
    """numData per block from {k, k - 1, 1, 0, k + 1} (the last two list nothing); `variant` turns the
    assignment so that over five variants every kind of mask row meets every one of them"""
    if nb == 1:
        return np.array([(k, max(1, k - 1), 1, 0, k + 1)[variant % 5]], np.uint16)
    nds = [k, max(1, k - 1), 1, 0, k + 1]
    return np.array([nds[(b + variant) % 5] for b in range(nb)], np.uint16)


def build_pending(k, m, num_data, rng, words, first=0):
    """per block one of: 0 empty; 1 full; 2 source only; 3 parity only; 4 one bit on each side of every
    word boundary; 5 random (block b gets kind (b + first) % 6).  Odd blocks also carry junk bits at and
    past nd + m."""
    nb = len(num_data)
    mask = np.zeros((nb, words), np.uint32)
    for b in range(nb):
        nd = int(num_data[b])
        ndv = nd if 1 <= nd <= k else k
        n = ndv + m
        kind = (b + first) % ROWS
        if kind == 1:
            _set(mask, b, range(n))
        elif kind == 2:
            _set(mask, b, range(ndv))
        elif kind == 3:
            _set(mask, b, range(ndv, n))
        elif kind == 4:
            _set(mask, b, [s for w in range(1, words + 1) for s in (32 * w - 1, 32 * w) if s < n])
            _set(mask, b, [0, n - 1])
        elif kind == 5:
            _set(mask, b, np.nonzero(rng.random(n) < 0.5)[0].tolist())
        if b % 2 == 1:
            _set(mask, b, range(n, words * 32))
    return mask


def build_lengths(k, m, vec, num_data, mask, rng, stride):
    """Source segment lengths in [0, vec], junk past numData.  In every block with a pending parity
    slot and more than one source segment the longest source segment is made unique and NOT pending
    (the mask is changed for it): the parity length comes from a segment that is not sent.  One
    valid block (where there is one) also gets a source length of vec + 5, listed as it is.
    Returns (lengths, blocks whose longest segment is not pending)."""
    nb = len(num_data)
    lens = rng.integers(0, vec + 1, (nb, stride)).astype(np.uint16)
    unsent_max = []
    over = False
    for b in range(nb):
        nd = int(num_data[b])
        if nd < 1 or nd > k:
            continue
        lens[b, nd:] = 65535  # not source lengths: never read into a maximum
        parity_pending = any((int(mask[b, s // 32]) >> (s % 32)) & 1 for s in range(nd, nd + m))
        if parity_pending and nd > 1 and len(unsent_max) < 64:
            lens[b, :nd] = np.minimum(lens[b, :nd], vec - 1)
            j = int(rng.integers(nd))
            lens[b, j] = vec
            mask[b, j // 32] &= np.uint32(~(1 << (j % 32)) & 0xFFFFFFFF)
            unsent_max.append(b)
        elif not over and (int(mask[b, 0]) & 1):
            lens[b, 0] = vec + 5
            over = True
    return lens, unsent_max


NAMES =("offsets", "block_index", "symbol_id", "length", "block_start")


def test_tx_symbols_declared_exported_and_bound():
    declared = N.declared_symbols()
    L = N.lib()
    for name in NEW:
        assert name in declared, f"{name} not declared in include/nfec.h"
        assert hasattr(L, name), f"{name} not exported"
        assert name in N._SIGS, f"{name} missing from _SIGS"
    assert [f[0] for f in N.TxSegments._fields_] == ["payloads", "payload_bytes", "offsets", "block_index",
                                                      "symbol_id", "length", "count", "count_dev"]
    assert ctypes.sizeof(N.TxSegments) == 64 and N.TxSegments.count_dev.offset == 56
    assert hasattr(norm_amd, "tx_list_host")
    for name in ("list_pending", "emit_segments"):
        assert hasattr(NormEncoderRS8, name) and hasattr(norm_amd.NormDecoderRS8, name)


def _same(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        assert np.array_equal(g, w), (what, name)


SHAPES = [(8, 2, 6), (64, 32, 6), (4096, 256, 6), (8, 2, 1), (8, 2, 4099)]


@pytest.mark.parametrize("k,m,nb", SHAPES)
def test_tx_list_host_matches_reference_rule(k, m, nb):
    vec = 1400
    rng = np.random.default_rng(k * 37 + m + nb)
    listed_unsent_max = listed_nothing = cut = 0
    for variant in range(5 if k < 4096 else 2):
        nd = num_data_for(k, nb, variant)
        words = (k + m + 31) // 32 + variant % 2  # the minimal mask_stride and a larger one
        mask = build_pending(k, m, nd, rng, words, first=variant + 1 if nb == 1 else 0)
        lstride = k + 3 * (variant % 2)
        for gap in (0, 13):
            # seg_length NULL: every length is vector_size
            want = ref_tx_list(k, m, vec, mask, nd, None, gap, nb * (k + m))
            _same(norm_amd.tx_list_host(k, m, vec, mask, nd, None, gap), want, (variant, gap, "no lengths"))
            total = int(want[4][nb, 0])
            assert int(want[4][nb, 1]) == total * (gap + vec)
            # seg_length given, the longest source segment of some blocks not pending
            mask2 = mask.copy()
            lens, unsent = build_lengths(k, m, vec, nd, mask2, rng, lstride)
            want = ref_tx_list(k, m, vec, mask2, nd, lens, gap, nb * (k + m))
            got = norm_amd.tx_list_host(k, m, vec, mask2, nd, lens, gap)
            _same(got, want, (variant, gap, "lengths"))
            for b in unsent:  # the parity entries of such a block carry vec, which no listed source entry has
                mine = got[1][:int(got[4][nb, 0])] == b
                par = mine & (got[2][:len(mine)] >= nd[b])
                assert par.any() and (got[3][:len(mine)][par] == vec).all()
                assert (got[3][:len(mine)][mine & ~par] < vec).all()
            listed_unsent_max += len(unsent)
            listed_nothing += int(((nd < 1) | (nd > k)).sum())
            # capacity below the total: full totals, the same block_start, nothing written past it
            total = int(want[4][nb, 0])
            if total >= 2:
                cap = total // 2
                arrs = [np.full(total, 0xAB, dt) for dt in (np.uint64, np.uint32, np.uint16, np.uint16)]
                start = np.zeros((nb + 1, 2), np.uint64)
                rc = N.lib().nfec_tx_list_host(k, m, vec, mask2.ctypes.data, words, nd.ctypes.data, nb,
                                               lens.ctypes.data, lstride, gap, *[a.ctypes.data for a in arrs], cap,
                                               start.ctypes.data)
                assert rc == N.NFEC_OK
                assert np.array_equal(start, want[4])
                for a, w in zip(arrs, want[:4]):
                    assert np.array_equal(a[:cap], w[:cap]) and (a[cap:] == 0xAB).all()
                cut += 1
        if variant == 0 and nb > 1:  # num_data NULL = k
            full = build_pending(k, m, np.full(nb, k, np.uint16), rng, words)
            _same(norm_amd.tx_list_host(k, m, vec, full, None, None, 13),
                  ref_tx_list(k, m, vec, full, None, None, 13, nb * (k + m)), "num_data NULL")
    assert cut and listed_nothing and (nb == 1 or listed_unsent_max)


def test_tx_list_host_small_example():
    """RS(8,2), two blocks, by hand: block 0 sends source 1 and 3 and parity 8, block 1 (numData 5)
    parity 6 only; lengths 100, 90; 250 is block 0's longest (not pending), 70 block 1's"""
    mask = np.array([[(1 << 1) | (1 << 3) | (1 << 8)], [(1 << 6) | (1 << 7) | (1 << 9)]], np.uint32)
    nd = np.array([8, 5], np.uint16)
    lens = np.array([[10, 100, 250, 90, 1, 2, 3, 4], [70, 5, 6, 7, 8, 999, 999, 999]], np.uint16)
    off, blk, sym, ln, start = norm_amd.tx_list_host(8, 2, 300, mask, nd, lens, gap=13, capacity=6)
    assert start.tolist() == [[0, 0], [3, 100 + 90 + 250 + 39], [4, 479 + 70 + 13]]
    assert blk.tolist() == [0, 0, 0, 1, 0, 0] and sym.tolist() == [1, 3, 8, 6, 0, 0]
    assert ln.tolist() == [100, 90, 250, 70, 0, 0]
    assert off.tolist() == [13, 126, 229, 492, 0, 0]


def test_tx_list_host_argument_checks():
    L = N.lib()
    mask = np.zeros((2, 3), np.uint32)
    lens = np.zeros((2, 64), np.uint16)
    off, blk = np.zeros(8, np.uint64), np.zeros(8, np.uint32)
    sym, ln = np.zeros(8, np.uint16), np.zeros(8, np.uint16)
    start = np.zeros((3, 2), np.uint64)
    E = N.NFEC_EINVAL

    def call(k=64, m=32, vec=100, pending=mask.ctypes.data, stride=3, nb=2, seg=lens.ctypes.data, lstride=64,
             o=off.ctypes.data, bi=blk.ctypes.data, s=sym.ctypes.data, le=ln.ctypes.data, cap=8, st=start.ctypes.data):
        return L.nfec_tx_list_host(k, m, vec, pending, stride, None, nb, seg, lstride, 0, o, bi, s, le, cap, st)

    assert call() == N.NFEC_OK
    assert call(stride=2) == E and "mask_stride" in N.last_error()
    assert call(lstride=63) == E and "length_stride" in N.last_error()
    assert call(seg=None, lstride=0) == N.NFEC_OK  # no lengths: length_stride is not looked at
    assert call(pending=None) == E and "pending" in N.last_error()
    for name in ("o", "bi", "s", "le"):
        assert call(**{name: None}) == E and "output" in N.last_error()
    assert call(st=None) == E and "block_start" in N.last_error()
    assert call(k=0) == E and call(m=0) == E and call(vec=0) == E and call(vec=65536) == E
    # no blocks: only the totals row, both zero
    start[:] = 7
    assert call(nb=0, pending=None) == N.NFEC_OK and start[0].tolist() == [0, 0] and (start[1:] == 7).all()


def _host_only_call_args():
    """well-formed arguments for the device entries (host arrays: a host-only codec never reads them)"""
    blk = np.zeros((2, 96, 64), np.uint8)
    b = N.BlockBatch()
    b.blocks, b.block_stride, b.seg_stride, b.nblocks = blk.ctypes.data, 96 * 64, 64, 2
    pay = np.zeros(256, np.uint8)
    off = np.full(2, 16, np.uint64)
    bi = np.zeros(2, np.uint32)
    sid = np.zeros(2, np.uint16)
    ln = np.full(2, 64, np.uint16)
    seg = N.TxSegments()
    seg.payloads, seg.payload_bytes = pay.ctypes.data, 256
    seg.offsets, seg.block_index = off.ctypes.data, bi.ctypes.data
    seg.symbol_id, seg.length, seg.count = sid.ctypes.data, ln.ctypes.data, 2
    mask = np.full((2, 3), 0xFFFFFFFF, np.uint32)
    start = np.zeros((3, 2), np.uint64)
    return b, seg, mask, start, (blk, pay, off, bi, sid, ln)


def test_tx_device_entries_argument_checks_and_host_only_codec():
    """null arrays, a short mask and a bad fec_id / fec_m pair are NFEC_EINVAL before the codec's
    device is looked at; a host-only codec answers NFEC_EDEVICE to well-formed calls"""
    enc = NormEncoderRS8(options=N.NFEC_OPT_HOST_ONLY)
    assert enc.Init(64, 32, 64)  # 96 slots: mask_stride >= 3
    L = N.lib()
    b, seg, mask, start, keep = _host_only_call_args()
    blk, pay, off, bi, sid, ln = keep
    E, D = N.NFEC_EINVAL, N.NFEC_EDEVICE
    bb, sg, mp = ctypes.byref(b), ctypes.byref(seg), mask.ctypes.data

    def emit(codec=enc._h, batch=bb, segs=sg, fec_id=5, fec_m=8, pending=mp, stride=3):
        return L.nfec_tx_emit(codec, batch, segs, fec_id, fec_m, 0, pending, stride, None, None)

    assert emit() == D and emit(pending=None, stride=0) == D and emit(fec_id=0, fec_m=0) == D
    assert emit(fec_id=2, fec_m=16) == D and emit(fec_id=129) == D
    assert emit(codec=None) == E and emit(batch=None) == E and emit(segs=None) == E
    assert emit(stride=2) == E and "mask_stride" in N.last_error()
    assert emit(fec_id=2, fec_m=12) == E and "fec_id" in N.last_error()
    assert emit(fec_id=7) == E
    for field in ("payloads", "offsets", "block_index", "symbol_id", "length"):
        saved = getattr(seg, field)
        setattr(seg, field, None)
        assert emit() == E and field in N.last_error()
        setattr(seg, field, saved)
    assert not pay.any() and (mask == 0xFFFFFFFF).all()

    def lst(codec=enc._h, pending=mp, stride=3, seg_length=None, lstride=0, o=off.ctypes.data, st=start.ctypes.data):
        return L.nfec_tx_list(codec, pending, stride, None, 2, seg_length, lstride, 0, o, bi.ctypes.data,
                              sid.ctypes.data, ln.ctypes.data, 2, st, None)

    assert lst() == D
    assert lst(codec=None) == E and lst(o=None) == E and lst(st=None) == E
    assert lst(pending=None) == E and "pending" in N.last_error()
    assert lst(stride=2) == E and "mask_stride" in N.last_error()
    assert lst(seg_length=ln.ctypes.data, lstride=63) == E and "length_stride" in N.last_error()
    assert not start.any()
