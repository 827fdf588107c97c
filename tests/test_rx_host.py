"""Receiver assembly, the parts that need no GPU: the ABI of the new entries, the host form of the
erasure-list rule (nfec_rx_erasures_host) against a NumPy restatement of what
NormObject::HandleObjectMessage does before Decode (reference src/common/normObject.cpp:1560-1606),
and the argument / device checks of the device entries on a host-only codec."""
import ctypes

import numpy as np
import pytest

import norm_amd
from norm_amd import NormDecoderRS8
from norm_amd import _native as N

NEW = ("nfec_rx_place", "nfec_rx_erasures", "nfec_decode_received", "nfec_rx_erasures_host")


def test_rx_symbols_declared_exported_and_bound():
    declared = N.declared_symbols()
    L = N.lib()
    for name in NEW:
        assert name in declared, f"{name} not declared in include/nfec.h"
        assert hasattr(L, name), f"{name} not exported"
        assert name in N._SIGS, f"{name} missing from _SIGS"
    # the segment descriptor: five pointers and a count, C layout
    assert [f[0] for f in N.RxSegments._fields_] == ["payloads", "offsets", "block_index", "symbol_id", "length",
                                                      "count"]
    assert ctypes.sizeof(N.RxSegments) == 48
    for name in ("received_mask", "erasures_from_received_host"):
        assert hasattr(norm_amd, name)
    for name in ("place_segments", "erasures_from_received", "decode_received"):
        assert hasattr(NormDecoderRS8, name)
    assert hasattr(norm_amd.NormEncoderRS8, "place_segments") and not hasattr(norm_amd.NormEncoderRS8,
                                                                             "decode_received")


def ref_erasures(k, m, mask, num_data, stride):
    """normObject.cpp:1560-1606 on a bit mask of RECEIVED slots (NORM's pending mask inverted):
    GetFirstPending < numData -> every pending source slot, then every pending parity slot."""
    nb = mask.shape[0]
    locs = np.zeros((nb, stride), np.uint16)
    counts = np.zeros(nb, np.uint16)
    for b in range(nb):
        nd = k if num_data is None else int(num_data[b])
        if nd < 1 or nd > k:
            continue
        pending = [s for s in range(nd + m) if not (int(mask[b, s // 32]) >> (s % 32)) & 1]
        if not pending or pending[0] >= nd:
            continue
        out = [s for s in pending if s < nd] + [s for s in pending if s >= nd]
        counts[b] = len(out)
        locs[b, :min(len(out), stride)] = out[:stride]
    return locs, counts


def _set(mask, b, slots):
    for s in slots:
        mask[b, s // 32] |= np.uint32(1 << (s % 32))


def build_masks(k, m, num_data, rng, stride, words):
    """One block per case of the issue's list (cycled over the blocks' numData):
    0 all received; 1 only parity missing; 2 one source missing; 3 more than m missing;
    4 more than `stride` missing (source and parity); 5 random; each with stray bits set past nd + m
    on odd rounds."""
    nb = len(num_data)
    mask = np.zeros((nb, words), np.uint32)
    for b in range(nb):
        nd = int(num_data[b])
        ndv = nd if 1 <= nd <= k else k
        n = ndv + m
        have = set(range(n))
        case = b % 6
        if case == 1:
            have -= set((ndv + rng.choice(m, max(1, m // 2), replace=False)).tolist())
        elif case == 2:
            have.discard(int(rng.integers(ndv)))
            have.discard(ndv + int(rng.integers(m)))
        elif case == 3:
            miss = rng.choice(n, min(n, m + 1), replace=False)
            have -= set(miss.tolist())
            have.discard(0)
        elif case == 4:
            have -= set(rng.choice(n, min(n, stride + 3), replace=False).tolist())
            have.discard(ndv - 1)
        elif case == 5:
            have = set(np.nonzero(rng.random(n) < 0.7)[0].tolist())
        _set(mask, b, have)
        if (b // 6) % 2 == 1:  # stray bits past the block's slots: ignored
            _set(mask, b, range(n, words * 32))
    return mask


SHAPES = [(8, 2), (64, 32), (400, 100), (4096, 256)]


@pytest.mark.parametrize("k,m", SHAPES)
def test_rx_erasures_host_matches_reference_rule(k, m):
    rng = np.random.default_rng(k * 31 + m)
    nds = [k, 1, k - 1, 0, k + 1, max(1, k // 2), k, k, min(k, 33), k - 1, 1, k]
    num_data = np.array((nds * 2)[:24], np.uint16)
    stride = m
    words = (k + m + 31) // 32 + 1  # a mask_stride larger than needed
    mask = build_masks(k, m, num_data, rng, stride, words)
    locs, counts = norm_amd.erasures_from_received_host(k, m, mask, num_data)
    rl, rc = ref_erasures(k, m, mask, num_data, stride)
    assert np.array_equal(counts, rc)
    assert np.array_equal(locs, rl)
    assert (rc > m).any() and (rc == 0).any() and (rc == 2).any()
    # a stride smaller than the counts: the full count, the first `stride` entries, nothing past them
    small = max(1, m // 2)
    locs2, counts2 = norm_amd.erasures_from_received_host(k, m, mask, num_data, stride=small)
    rl2, rc2 = ref_erasures(k, m, mask, num_data, small)
    assert np.array_equal(counts2, rc) and np.array_equal(locs2, rl2) and (rc > small).any()
    # num_data NULL = k, on the minimal mask_stride
    full = np.ascontiguousarray(build_masks(k, m, np.full(12, k, np.uint16), rng, stride, words)[:, :words - 1])
    locs3, counts3 = norm_amd.erasures_from_received_host(k, m, full, None)
    rl3, rc3 = ref_erasures(k, m, full, None, stride)
    assert np.array_equal(counts3, rc3) and np.array_equal(locs3, rl3)


def test_rx_erasures_host_only_parity_missing_is_zero():
    mask = np.zeros((1, 1), np.uint32)
    _set(mask, 0, range(8))  # all source, no parity
    locs, counts = norm_amd.erasures_from_received_host(8, 2, mask)
    assert counts[0] == 0 and not locs.any()
    mask[0, 0] &= np.uint32(~(1 << 3) & 0xFFFFFFFF)
    locs, counts = norm_amd.erasures_from_received_host(8, 2, mask)
    assert counts[0] == 3 and locs[0].tolist() == [3, 8]  # stride m = 2: [3, 8], then 9 is counted only


def test_rx_erasures_host_argument_checks():
    L = N.lib()
    mask = np.zeros((2, 3), np.uint32)
    locs = np.zeros((2, 32), np.uint16)
    counts = np.zeros(2, np.uint16)
    ok = L.nfec_rx_erasures_host(64, 32, mask.ctypes.data, 3, None, 2, locs.ctypes.data, 32, counts.ctypes.data)
    assert ok == N.NFEC_OK and counts.tolist() == [96, 96]
    assert L.nfec_rx_erasures_host(64, 32, mask.ctypes.data, 2, None, 2, locs.ctypes.data, 32,
                                   counts.ctypes.data) == N.NFEC_EINVAL
    assert "mask_stride" in N.last_error()
    assert L.nfec_rx_erasures_host(64, 32, None, 3, None, 2, locs.ctypes.data, 32,
                                   counts.ctypes.data) == N.NFEC_EINVAL
    assert "received" in N.last_error()
    assert L.nfec_rx_erasures_host(64, 32, mask.ctypes.data, 3, None, 2, None, 32,
                                   counts.ctypes.data) == N.NFEC_EINVAL
    assert "erasure_locs" in N.last_error()
    assert L.nfec_rx_erasures_host(64, 32, mask.ctypes.data, 3, None, 2, locs.ctypes.data, 32,
                                   None) == N.NFEC_EINVAL
    assert "erasure_counts" in N.last_error()
    assert L.nfec_rx_erasures_host(0, 32, mask.ctypes.data, 3, None, 2, locs.ctypes.data, 32,
                                   counts.ctypes.data) == N.NFEC_EINVAL


def _host_only_call_args():
    """well-formed arguments for the device entries (host arrays: a host-only codec never reads them)"""
    blk = np.zeros((2, 20, 64), np.uint8)
    b = N.BlockBatch()
    b.blocks, b.block_stride, b.seg_stride, b.nblocks = blk.ctypes.data, 20 * 64, 64, 2
    pay = np.zeros(256, np.uint8)
    off = np.zeros(2, np.uint64)
    bi = np.zeros(2, np.uint32)
    sid = np.zeros(2, np.uint16)
    ln = np.full(2, 64, np.uint16)
    seg = N.RxSegments()
    seg.payloads, seg.offsets, seg.block_index = pay.ctypes.data, off.ctypes.data, bi.ctypes.data
    seg.symbol_id, seg.length, seg.count = sid.ctypes.data, ln.ctypes.data, 2
    mask = np.zeros((2, 1), np.uint32)
    locs = np.zeros((2, 4), np.uint16)
    counts = np.zeros(2, np.uint16)
    status = np.zeros(2, np.int32)
    return b, seg, mask, locs, counts, status, (blk, pay, off, bi, sid, ln)


def test_rx_device_entries_refuse_host_only_codec():
    dec = NormDecoderRS8(options=N.NFEC_OPT_HOST_ONLY)
    assert dec.Init(16, 4, 64)
    L = N.lib()
    b, seg, mask, locs, counts, status, keep = _host_only_call_args()
    assert L.nfec_rx_place(dec._h, ctypes.byref(b), ctypes.byref(seg), mask.ctypes.data, 1, None,
                           None) == N.NFEC_EDEVICE
    assert L.nfec_rx_erasures(dec._h, mask.ctypes.data, 1, None, 2, locs.ctypes.data, 4, counts.ctypes.data,
                              None) == N.NFEC_EDEVICE
    assert L.nfec_decode_received(dec._h, ctypes.byref(b), mask.ctypes.data, 1, status.ctypes.data,
                                  None) == N.NFEC_EDEVICE
    assert not mask.any() and not counts.any()


def test_rx_device_entries_argument_checks():
    """null arrays and a short mask are NFEC_EINVAL before the codec's device is looked at"""
    dec = NormDecoderRS8(options=N.NFEC_OPT_HOST_ONLY)
    assert dec.Init(64, 32, 64)  # 96 slots: mask_stride >= 3
    L = N.lib()
    b, seg, _, locs, counts, status, keep = _host_only_call_args()
    b.block_stride = 96 * 64
    mask = np.zeros((2, 3), np.uint32)
    E = N.NFEC_EINVAL
    # mask_stride too small / null mask
    assert L.nfec_rx_place(dec._h, ctypes.byref(b), ctypes.byref(seg), mask.ctypes.data, 2, None, None) == E
    assert "mask_stride" in N.last_error()
    assert L.nfec_rx_erasures(dec._h, mask.ctypes.data, 2, None, 2, locs.ctypes.data, 4, counts.ctypes.data, None) == E
    assert L.nfec_decode_received(dec._h, ctypes.byref(b), mask.ctypes.data, 2, status.ctypes.data, None) == E
    assert L.nfec_rx_place(dec._h, ctypes.byref(b), ctypes.byref(seg), None, 3, None, None) == E
    assert L.nfec_rx_erasures(dec._h, None, 3, None, 2, locs.ctypes.data, 4, counts.ctypes.data, None) == E
    assert L.nfec_decode_received(dec._h, ctypes.byref(b), None, 3, status.ctypes.data, None) == E
    # null codec / batch / segments
    assert L.nfec_rx_place(None, ctypes.byref(b), ctypes.byref(seg), mask.ctypes.data, 3, None, None) == E
    assert L.nfec_rx_place(dec._h, None, ctypes.byref(seg), mask.ctypes.data, 3, None, None) == E
    assert L.nfec_rx_place(dec._h, ctypes.byref(b), None, mask.ctypes.data, 3, None, None) == E
    assert L.nfec_rx_erasures(None, mask.ctypes.data, 3, None, 2, locs.ctypes.data, 4, counts.ctypes.data, None) == E
    assert L.nfec_decode_received(None, ctypes.byref(b), mask.ctypes.data, 3, status.ctypes.data, None) == E
    assert L.nfec_decode_received(dec._h, None, mask.ctypes.data, 3, status.ctypes.data, None) == E
    # null descriptor arrays, each named in the message
    for field in ("payloads", "offsets", "block_index", "symbol_id", "length"):
        saved = getattr(seg, field)
        setattr(seg, field, None)
        assert L.nfec_rx_place(dec._h, ctypes.byref(b), ctypes.byref(seg), mask.ctypes.data, 3, None, None) == E
        assert field in N.last_error()
        setattr(seg, field, saved)
    # null output lists
    assert L.nfec_rx_erasures(dec._h, mask.ctypes.data, 3, None, 2, None, 4, counts.ctypes.data, None) == E
    assert L.nfec_rx_erasures(dec._h, mask.ctypes.data, 3, None, 2, locs.ctypes.data, 4, None, None) == E
    # and with everything in place the host-only codec answers for its missing device
    assert L.nfec_rx_place(dec._h, ctypes.byref(b), ctypes.byref(seg), mask.ctypes.data, 3, None,
                           None) == N.NFEC_EDEVICE
