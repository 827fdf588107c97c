"""The 3-waves-per-SIMD fused RS8 repair (rs8_fdec3.hip), byte for byte against the oracle,
statuses included.

The kernel takes the lane-major batches of RS8(64,32) and RS8(64,16) whose segment fits its
per-wave LDS region (vec up to 1,664 B; (64,8) stays on the 2-waves kernel); it stages every
source column through an LDS ring filled by 16-byte LDS-DMA pieces and parks z rows 8..15 in LDS
during the solve.  The cases sit where that can go wrong: segments of one
item, of less than one piece, with a half-filled last piece (1,400 B) and exactly 4 * 44 items
(1,408 B), the dispatch bound and 8 B past it (the 2-waves kernel), last workgroups that are partly
empty (nb = 5, 7, 13), e on both sides of the second half of outputs (8 / 9) and of the parked rows,
and the e = 16 copy of the solve."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from norm_amd import NFEC_RS8, NormDecoderRS8  # noqa: E402

K = 64
F3_MAX_VEC = 1664   # gen_fdec_asm.py F3_MAX_VEC: 52 lanes of 4 items


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from norm_amd import device_count

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    assert device_count() >= 1, "no gfx950 device visible to libnfec"


def _i16(a):
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.uint16).view(np.int16)).cuda()


def _decoder(m, vec):
    dec = NormDecoderRS8()
    assert dec.Init(K, m, vec)
    return dec


def _clean(orc, m, vec, nb, nd=None):
    if nd is None:
        return orc.encode_blocks(NFEC_RS8, K, m, vec, orc.make_blocks(K, m, vec, nb))
    return orc.encode_blocks(NFEC_RS8, K, m, vec, orc.make_blocks(K, m, vec, nb, num_data=nd), num_data=nd)


def _check(orc, dec, m, vec, clean, erasures, nd=None, accumulate=False, seed=1):
    """erase the listed slots of each block (source slot < numData, parity row r at numData + r),
    decode on the GPU and with the oracle, compare every byte and every status"""
    nb = clean.shape[0]
    rng = np.random.default_rng(seed)
    locs = np.zeros((nb, m), np.uint16)
    counts = np.zeros(nb, np.uint16)
    rx = clean.copy()
    for b, e in enumerate(erasures):
        e = np.sort(np.asarray(e, int))
        locs[b, :len(e)] = e
        counts[b] = len(e)
        n = K if nd is None else int(nd[b])
        for s in e:
            rx[b, s] = rng.integers(0, 256, vec, dtype=np.uint8) if (accumulate and s < n) else 0
    ref = rx.copy()
    for b, e in enumerate(erasures):
        ref[b, np.asarray(e, int)] = 0
    args = (nd,) if nd is not None else ()
    st_ref = orc.decode_blocks(NFEC_RS8, K, m, vec, ref, locs, counts, *args)
    expect = ref
    if accumulate:  # the repair XORs into the erased source buffers
        expect = rx.copy()
        for b, e in enumerate(erasures):
            n = K if nd is None else int(nd[b])
            for s in e:
                if s < n:
                    expect[b, s] ^= clean[b, s]
    dev = torch.from_numpy(rx).cuda()
    kw = {"num_data": _i16(nd)} if nd is not None else {}
    st = dec.decode_blocks(dev, _i16(locs), _i16(counts), accumulate=accumulate, **kw)
    torch.cuda.synchronize()
    assert np.array_equal(st.cpu().numpy(), st_ref)
    got = dev.cpu().numpy()
    bad = np.argwhere(got != expect)
    assert bad.size == 0, f"{len(bad)} bytes differ, first (block, slot, byte) = {bad[0]}"


def _source_erasures(rng, e, b, n=K):
    """e erased source columns; column 0 and the last one among them in turn"""
    e = min(e, n)
    must = [[0], [n - 1], [0, n - 1], []][b % 4][:e]
    rest = [c for c in range(n) if c not in must]
    return sorted(must + list(rng.choice(rest, e - len(must), replace=False)))


VECS = [(8, 5), (24, 7), (1400, 13), (1408, 5), (F3_MAX_VEC, 7), (F3_MAX_VEC + 8, 13)]


@pytest.mark.parametrize("m", [32, 16])
@pytest.mark.parametrize("vec,nb", VECS)
def test_fdec3_segment_sizes_and_erasure_counts(orc, m, vec, nb):
    """e in {1, 8, 9, 16} (capped by m) over the blocks of a batch, erasures in columns 0 and 63"""
    rng = np.random.default_rng(100 * m + vec)
    clean = _clean(orc, m, vec, nb)
    es = [1, 8, 9, 16, 16, 9, 8, 1, 16, 2, 15, 7, 10]
    erasures = [_source_erasures(rng, min(es[b], m), b) for b in range(nb)]
    _check(orc, _decoder(m, vec), m, vec, clean, erasures)


@pytest.mark.parametrize("m", [32, 16])
@pytest.mark.parametrize("vec,nb", [(1400, 7), (F3_MAX_VEC, 5), (24, 13)])
def test_fdec3_accumulate(orc, m, vec, nb):
    rng = np.random.default_rng(7 * m + vec)
    clean = _clean(orc, m, vec, nb)
    es = [16, 1, 9, 8, 3, 16, 12, 5, 9, 8, 1, 16, 4]
    erasures = [_source_erasures(rng, min(es[b], m), b) for b in range(nb)]
    _check(orc, _decoder(m, vec), m, vec, clean, erasures, accumulate=True)


@pytest.mark.parametrize("m", [32, 16])
def test_fdec3_erased_parity_rows_and_unfused_neighbours(orc, m):
    """An erased parity row below the last used one gives a zero coefficient row (the block stays
    fused, its highest used row moves up, past row 8 in block 1).  m = 32: a block whose
    substitute parity lies at row >= 16 and a block with e > 16 go to the unfused kernels in the
    same batch: the fused kernel must leave them alone and the unfused ones must skip the blocks
    it cleared.  Two more calls on the same decoder follow: all fused, then mixed again."""
    vec, nb = 1400, 13
    rng = np.random.default_rng(m)
    clean = _clean(orc, m, vec, nb)
    dec = _decoder(m, vec)

    def batch(mixed):
        out = []
        for b in range(nb):
            if b == 0:
                e = _source_erasures(rng, 3, b) + [K + 1]                       # rows 0, 2, 3
            elif b == 1:
                e = _source_erasures(rng, min(7, m - 3), b) + [K, K + 2, K + 5]  # rows up to 9
            elif b == 2 and m == 32 and mixed:
                e = _source_erasures(rng, 2, b) + list(range(K, K + 15))         # rows 15, 16
            elif b == 3 and m == 32 and mixed:
                e = _source_erasures(rng, 17, b)                                  # e > 16
            elif b == nb - 1 and mixed:
                e = _source_erasures(rng, 1, b) + list(range(K, K + m - 1))      # last row only
            else:
                e = _source_erasures(rng, min([16, 9, 8, 1][b % 4], m), b)
            out.append(e)
        return out

    _check(orc, dec, m, vec, clean, batch(True), seed=2)
    _check(orc, dec, m, vec, clean, batch(False), seed=3)
    _check(orc, dec, m, vec, clean, batch(True), seed=4, accumulate=True)


@pytest.mark.parametrize("m", [32, 16])
@pytest.mark.parametrize("accumulate", [False, True])
def test_fdec3_shortened_blocks(orc, m, accumulate):
    """numData in {k, k - 1, 13}: columns past numData are skipped, parity read at numData + t"""
    vec, nb = 1400, 7
    rng = np.random.default_rng(31 + m)
    nd = np.array([K, K - 1, 13, K, 13, K - 1, K], np.uint16)
    clean = _clean(orc, m, vec, nb, nd)
    es = [16, 9, 8, 1, 13, 16, 8]
    erasures = [_source_erasures(rng, min(es[b], m), b, int(nd[b])) for b in range(nb)]
    erasures[5] = erasures[5][:min(5, m - 1)] + [int(nd[5]) + 1]   # and an erased parity row
    _check(orc, _decoder(m, vec), m, vec, clean, erasures, nd=nd, accumulate=accumulate)


def test_fdec3_last_segment_at_the_end_of_the_storage(orc):
    """m = e = 16: parity row e - 1 is the block's last segment, and the last block's ends the
    exactly sized tensor.  Its last 16-byte piece is half inside the segment; column 63 is erased
    and repaired in every block.  (What keeps the piece's second half from being read is the
    load descriptor: it starts at the segment and has vec records.)"""
    m, vec, nb = 16, 1400, 5
    rng = np.random.default_rng(63)
    clean = _clean(orc, m, vec, nb)
    erasures = [sorted([K - 1] + list(rng.choice(K - 1, 15, replace=False))) for _ in range(nb)]
    _check(orc, _decoder(m, vec), m, vec, clean, erasures)
    _check(orc, _decoder(m, vec), m, vec, clean, erasures, accumulate=True)
