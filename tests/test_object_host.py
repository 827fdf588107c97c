"""Object segmentation, the host rules: nfec_object_layout_for, nfec_object_segment and
nfec_object_block_sizes against a plain-integer restatement of NormObject::Open's block partition
(reference src/common/normObject.cpp:134-137, :203-231) and of ReadSegment's offset rule
(:2682-2709), and the argument checks of the two device entries that need no device."""
import ctypes

import numpy as np
import pytest

import norm_amd
from norm_amd import NormEncoderRS8
from norm_amd import _native as N

FIELDS = [f for f, _ in N.ObjectLayout._fields_]
BIG = [(2 ** 40 + 3, 1392, 64), (65535 * 4096 * 2 + 1, 65535, 4096)]


def ceil_div(a, b):
    return -(-a // b)


def open_ref(object_size, segment_size, num_data):
    """Open:134-137, 203-231 in Python integers (NormObjectSize's divide rounds up)"""
    num_segments = ceil_div(object_size, segment_size)
    num_blocks = ceil_div(num_segments, num_data)
    large_block_size = ceil_div(num_segments, num_blocks)
    if num_segments == num_blocks * large_block_size:
        small_block_size, small_block_count, large_block_count = large_block_size, num_blocks, 0
    else:
        small_block_size = large_block_size - 1
        large_block_count = num_segments - num_blocks * small_block_size
        small_block_count = num_blocks - large_block_count
    return dict(object_size=object_size, segment_size=segment_size, num_data=num_data, num_segments=num_segments,
                num_blocks=num_blocks, large_block_size=large_block_size, large_block_count=large_block_count,
                small_block_size=small_block_size, small_block_count=small_block_count,
                final_block_id=large_block_count + small_block_count - 1,
                final_segment_size=object_size - (num_segments - 1) * segment_size)


def as_dict(layout):
    return {f: getattr(layout, f) for f in FIELDS}


def block_size(lay, b):
    return lay.large_block_size if b < lay.large_block_count else lay.small_block_size


def check_invariants(lay):
    sizes_sum = lay.large_block_count * lay.large_block_size + lay.small_block_count * lay.small_block_size
    assert sizes_sum == lay.num_segments                      # the block sizes sum to num_segments
    assert lay.large_block_count + lay.small_block_count == lay.num_blocks
    assert 0 <= lay.large_block_size - lay.small_block_size <= 1  # large first, sizes differ by at most 1
    assert 1 <= lay.small_block_size and lay.large_block_size <= lay.num_data
    assert 1 <= lay.final_segment_size <= lay.segment_size
    assert lay.final_block_id == lay.num_blocks - 1


def test_layout_matches_open_exhaustively():
    for seg in (1, 7, 16, 37):
        for k in (1, 2, 8, 64):
            for size in range(1, 601):
                lay = norm_amd.object_layout(size, seg, k)
                assert as_dict(lay) == open_ref(size, seg, k), (size, seg, k)
                check_invariants(lay)


@pytest.mark.parametrize("size,seg,k", BIG)
def test_layout_matches_open_large(size, seg, k):
    lay = norm_amd.object_layout(size, seg, k)
    assert as_dict(lay) == open_ref(size, seg, k)
    check_invariants(lay)


def test_layout_degenerate_case_is_the_references():
    """num_segments == num_blocks * large_block_size: no large blocks, every block 'small'"""
    lay = norm_amd.object_layout(16 * 8 * 3, 16, 8)
    assert (lay.large_block_count, lay.small_block_size, lay.small_block_count) == (0, 8, 3)
    assert lay.large_block_size == 8 and lay.final_segment_size == 16
    lay = norm_amd.object_layout(65535 * 4096 * 2 + 1, 65535, 4096)  # 8,193 segments in 3 blocks of 2,731
    assert (lay.num_segments, lay.num_blocks, lay.large_block_count, lay.small_block_size) == (8193, 3, 0, 2731)


def test_segments_tile_small_objects_exactly():
    """offsets are the running sum of the lengths in (block, segment) order and end at object_size"""
    L = N.lib()
    off, ln = ctypes.c_uint64(), ctypes.c_uint32()
    for seg in (1, 7, 16, 37):
        for k in (1, 2, 8, 64):
            for size in range(1, 601):
                lay = norm_amd.object_layout(size, seg, k)
                at = 0
                for b in range(lay.num_blocks):
                    for s in range(block_size(lay, b)):
                        assert L.nfec_object_segment(ctypes.byref(lay), b, s, ctypes.byref(off), ctypes.byref(ln)) == 0
                        assert off.value == at, (size, seg, k, b, s)
                        last = b == lay.num_blocks - 1 and s == block_size(lay, b) - 1
                        assert ln.value == (lay.final_segment_size if last else seg)
                        at += ln.value
                assert at == size


def test_segments_of_the_large_object_at_its_boundaries():
    """2^40 + 3 bytes: 64-bit offsets at the large/small boundary and in the final block"""
    size, seg, k = BIG[0]
    lay = norm_amd.object_layout(size, seg, k)
    assert lay.large_block_count > 0 and lay.small_block_count > 0
    lbc, lbs, sbs = lay.large_block_count, lay.large_block_size, lay.small_block_size

    def start(b):  # first byte of block b, restated
        return (b * lbs if b < lbc else lbc * lbs + (b - lbc) * sbs) * seg

    for b in (0, 1, lbc - 2, lbc - 1, lbc, lbc + 1, lay.num_blocks - 2, lay.num_blocks - 1):
        at = start(b)
        for s in range(block_size(lay, b)):
            off, ln = norm_amd.object_segment(lay, b, s)
            assert off == at
            at += ln
        assert at == (start(b + 1) if b + 1 < lay.num_blocks else size)
    assert start(lbc) > 2 ** 40 - 2 ** 24  # the boundary lies past 32 bits of offset by far
    off, ln = norm_amd.object_segment(lay, lay.final_block_id, sbs - 1)
    assert ln == lay.final_segment_size and off + ln == size


def test_segment_range_errors():
    L = N.lib()
    lay = norm_amd.object_layout(1000, 37, 8)  # 28 segments: 4 blocks of 7
    off, ln = ctypes.c_uint64(), ctypes.c_uint32()
    args = (ctypes.byref(off), ctypes.byref(ln))
    assert L.nfec_object_segment(ctypes.byref(lay), lay.num_blocks - 1, 6, *args) == N.NFEC_OK
    assert L.nfec_object_segment(ctypes.byref(lay), lay.num_blocks, 0, *args) == N.NFEC_ERANGE
    assert L.nfec_object_segment(ctypes.byref(lay), 0, 7, *args) == N.NFEC_ERANGE
    lay = norm_amd.object_layout(1000, 37, 5)  # 28 segments in 6 blocks: 4 of 5, 2 of 4
    assert (lay.large_block_count, lay.small_block_count) == (4, 2)
    assert L.nfec_object_segment(ctypes.byref(lay), 3, 4, *args) == N.NFEC_OK
    assert L.nfec_object_segment(ctypes.byref(lay), 4, 4, *args) == N.NFEC_ERANGE  # a small block has 4
    assert L.nfec_object_segment(ctypes.byref(lay), 4, 3, None, None) == N.NFEC_OK  # outputs are optional
    assert L.nfec_object_segment(None, 0, 0, *args) == N.NFEC_EINVAL


def test_block_sizes_windows():
    lay = norm_amd.object_layout(1000, 37, 5)  # sizes 5 5 5 5 4 4
    assert list(norm_amd.object_block_sizes(lay, 0, 6)) == [5, 5, 5, 5, 4, 4]
    assert list(norm_amd.object_block_sizes(lay, 3, 2)) == [5, 4]       # straddles large_block_count
    assert list(norm_amd.object_block_sizes(lay, 2, 4)) == [5, 5, 4, 4]  # ... and ends at the last block
    assert list(norm_amd.object_block_sizes(lay, 5, 1)) == [4]
    assert len(norm_amd.object_block_sizes(lay, 6, 0)) == 0
    size, seg, k = BIG[0]
    big = norm_amd.object_layout(size, seg, k)
    lbc = big.large_block_count
    assert list(norm_amd.object_block_sizes(big, lbc - 2, 4)) == [64, 64, 63, 63]
    assert list(norm_amd.object_block_sizes(big, big.num_blocks - 2, 2)) == [63, 63]
    L = N.lib()
    out = np.full(8, 0xAAAA, np.uint16)
    assert L.nfec_object_block_sizes(ctypes.byref(lay), 5, 2, out.ctypes.data) == N.NFEC_ERANGE
    assert L.nfec_object_block_sizes(ctypes.byref(lay), 0xFFFFFFFF, 2, out.ctypes.data) == N.NFEC_ERANGE
    assert (out == 0xAAAA).all()
    assert L.nfec_object_block_sizes(None, 0, 1, out.ctypes.data) == N.NFEC_EINVAL
    assert L.nfec_object_block_sizes(ctypes.byref(lay), 0, 1, None) == N.NFEC_EINVAL


def test_layout_argument_errors():
    L = N.lib()
    out = N.ObjectLayout()
    E = N.NFEC_EINVAL
    assert L.nfec_object_layout_for(100, 10, 4, None) == E
    assert L.nfec_object_layout_for(0, 10, 4, ctypes.byref(out)) == E
    assert L.nfec_object_layout_for(100, 0, 4, ctypes.byref(out)) == E
    assert L.nfec_object_layout_for(100, 10, 0, ctypes.byref(out)) == E
    assert L.nfec_object_layout_for(100, 65536, 4, ctypes.byref(out)) == E
    assert L.nfec_object_layout_for(100, 10, 65536, ctypes.byref(out)) == E
    assert L.nfec_object_layout_for(100, 65535, 65535, ctypes.byref(out)) == N.NFEC_OK
    # num_blocks must fit 32 bits: 2^32 - 1 blocks of one 1-byte segment pass, one more does not
    assert L.nfec_object_layout_for(2 ** 32 - 1, 1, 1, ctypes.byref(out)) == N.NFEC_OK
    assert out.num_blocks == 2 ** 32 - 1 and out.final_block_id == 2 ** 32 - 2
    assert L.nfec_object_layout_for(2 ** 32, 1, 1, ctypes.byref(out)) == N.NFEC_ERANGE
    assert L.nfec_object_layout_for(2 ** 64 - 1, 1, 65535, ctypes.byref(out)) == N.NFEC_ERANGE
    assert L.nfec_object_layout_for(2 ** 64 - 1, 65535, 65535, ctypes.byref(out)) == N.NFEC_ERANGE  # 2^32 + 131,077 blocks
    assert L.nfec_object_layout_for(2 ** 63 + 5, 65535, 65535, ctypes.byref(out)) == N.NFEC_OK
    assert as_dict(out) == open_ref(2 ** 63 + 5, 65535, 65535)
    check_invariants(out)


# ---- the device entries' argument checks (before the codec's device is looked at) ----

def _device_call_args(k=16, m=4, stride=64, nblocks=2):
    """well-formed host arrays: a host-only codec never reads them"""
    blk = np.zeros((nblocks, k + m, stride), np.uint8)
    b = N.BlockBatch()
    b.blocks, b.block_stride, b.seg_stride, b.nblocks = blk.ctypes.data, (k + m) * stride, stride, nblocks
    obj = np.zeros(4096, np.uint8)
    nd = np.full(nblocks, 0xAAAA, np.uint16)
    lens = np.full((nblocks, k), 0xAAAA, np.uint16)
    mask = np.zeros((nblocks, (k + m + 31) // 32), np.uint32)
    status = np.zeros(nblocks, np.int32)
    return b, obj, nd, lens, mask, status, blk


def test_object_device_entries_argument_checks():
    enc = NormEncoderRS8(options=N.NFEC_OPT_HOST_ONLY)
    assert enc.Init(16, 4, 64)
    L = N.lib()
    b, obj, nd, lens, mask, status, keep = _device_call_args()
    lay = norm_amd.object_layout(16 * 56 * 2 - 5, 56, 16)  # two blocks of 16 segments of 56 bytes
    assert lay.num_blocks == 2
    E, D = N.NFEC_EINVAL, N.NFEC_EDEVICE
    pl, pb = ctypes.byref(lay), ctypes.byref(b)

    def read(codec=enc._h, layout=pl, o=obj.ctypes.data, nbytes=obj.nbytes, first=0, batch=pb, ndo=nd.ctypes.data,
             lo=lens.ctypes.data, ls=16):
        return L.nfec_object_read(codec, layout, o, nbytes, first, batch, ndo, lo, ls, None)

    def write(codec=enc._h, layout=pl, o=obj.ctypes.data, nbytes=obj.nbytes, first=0, batch=pb, rcv=mask.ctypes.data,
              ms=1, st=status.ctypes.data):
        return L.nfec_object_write(codec, layout, o, nbytes, first, batch, rcv, ms, st, None, None)

    # well-formed calls reach the codec, which has no device
    assert read() == D and write() == D
    assert read(ndo=None, lo=None, ls=0) == D and write(rcv=None, ms=0, st=None) == D
    for call in (read, write):
        assert call(codec=None) == E
        assert call(layout=None) == E
        assert call(o=None) == E
        assert call(batch=None) == E
        assert call(first=1) == E and "first_block" in N.last_error()  # first_block + nblocks > num_blocks
    assert read(nbytes=lay.object_size - 1) == E and "object_bytes" in N.last_error()
    assert read(nbytes=lay.object_size) == D
    assert write(nbytes=1) == D  # the write clamps instead
    assert read(ls=15) == E and "length_stride" in N.last_error()
    assert read(lo=None, ls=0) == D
    assert write(ms=0) == E and "mask_stride" in N.last_error()
    # layout->num_data != k, segment_size > vector_size, a layout nfec_object_layout_for did not make
    other_k = norm_amd.object_layout(1000, 56, 8)
    assert read(layout=ctypes.byref(other_k)) == E and "num_data" in N.last_error()
    assert write(layout=ctypes.byref(other_k)) == E
    wide = norm_amd.object_layout(16 * 65 * 2, 65, 16)
    assert read(layout=ctypes.byref(wide)) == E and "segment_size" in N.last_error()
    assert write(layout=ctypes.byref(wide)) == E
    forged = norm_amd.object_layout(16 * 56 * 2 - 5, 56, 16)
    forged.large_block_size = 40
    assert read(layout=ctypes.byref(forged)) == E and write(layout=ctypes.byref(forged)) == E
    # nothing was written
    assert (nd == 0xAAAA).all() and (lens == 0xAAAA).all() and not obj.any() and not keep.any()


def test_object_symbols_declared_and_bound():
    names = ("nfec_object_layout_for", "nfec_object_segment", "nfec_object_block_sizes", "nfec_object_read",
             "nfec_object_write")
    declared = N.declared_symbols()
    for name in names:
        assert name in declared and name in N._SIGS and hasattr(N.lib(), name)
    assert ctypes.sizeof(N.ObjectLayout) == 56
