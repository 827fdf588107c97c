"""RS8 and MDP vectors of any length on the fast kernels (segment tails), bit-exact against the oracle.

NORM codes segmentSize + 8 bytes per segment (normSession.cpp:883): 1452-byte segments give
1460-byte vectors, not a multiple of the bit-sliced kernels' 8-byte pieces.  Such batches now run
the fast kernels (q4, the runtime-coefficient kernel, the closed-form and fused repairs) over
vec & ~7 bytes and the tail kernels (kernels_gf8tail.hip) over the last 1..7 bytes.

Every comparison is over the WHOLE array: the stride padding [vec, seg_stride) of every slot
holds junk before the call and must come back unchanged.  encode_paths() / decode_paths() tell
which kernel family took the batch, tail_batches() that the tail kernels ran beside it."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from norm_amd import (NFEC_MDP, NFEC_RS8, NormDecoderMDP, NormDecoderRS8, NormEncoderMDP,  # noqa: E402
                      NormEncoderRS8)

ENC = {NFEC_RS8: NormEncoderRS8, NFEC_MDP: NormEncoderMDP}
DEC = {NFEC_RS8: NormDecoderRS8, NFEC_MDP: NormDecoderMDP}
FIXED_RS8 = {(64, 32), (64, 16), (64, 8)}   # shapes with fixed-generator kernels
FIXED_MDP = {(64, 32)}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from norm_amd import device_count

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    assert device_count() >= 1, "no gfx950 device visible to libnfec"


def _i16(a):
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.uint16).view(np.int16)).cuda()


def _stride(vec):
    return (vec + 7) // 8 * 8


def _enc_path(kind, k, m, shortened=False):
    if kind == NFEC_RS8:
        return "fixed" if (k, m) in FIXED_RS8 else "runtime"
    return "fixed" if (k, m) in FIXED_MDP and not shortened else "runtime"


def _moved(before, after):
    return {p: after[p] - before[p] for p in after if after[p] != before[p]}


def _num_data(k, nb, seed, invalid=False):
    """numData mixed in 1..k, including k and 1 (and, invalid, a 0 and a k + 1: left alone)"""
    rng = np.random.default_rng(seed)
    nd = rng.integers(1, k + 1, nb).astype(np.uint16)
    fixed = [max(1, k // 4 - 1), max(1, k // 2 - 1), max(1, 3 * k // 4 - 1), k - 1, k, 1]
    nd[:min(nb, len(fixed))] = fixed[:nb]
    if invalid:
        nd[6] = 0
        nd[7] = k + 1
    return nd


def _encode_case(orc, kind, k, m, vec, stride, nb, nd=None, accumulate=False, expect_tail=1):
    """one device-batch encode against the oracle: junk in the stride padding of every slot, in the
    parity slots (overwritten, or XORed into under accumulate) and in the slots past numData + m"""
    rng = np.random.default_rng(k * 1000 + m * 10 + vec + nb)
    valid = np.ones(nb, bool) if nd is None else (nd >= 1) & (nd <= k)
    ndc = None if nd is None else np.clip(nd, 1, k)
    host = orc.make_blocks(k, m, vec, nb, seg_stride=stride, num_data=ndc)
    for b in range(nb):
        n = k if nd is None else int(ndc[b])
        host[b, n:, :] = rng.integers(0, 256, (k + m - n, stride), dtype=np.uint8)
    host[:, :, vec:] = rng.integers(0, 256, (nb, k + m, stride - vec), dtype=np.uint8)
    ref = host.copy()
    if valid.any():
        ref[valid] = orc.encode_blocks(kind, k, m, vec, host[valid].copy(), num_data=None if nd is None else nd[valid])
    for b in np.nonzero(valid)[0]:
        n = k if nd is None else int(nd[b])
        if accumulate:
            ref[b, n:n + m, :vec] ^= host[b, n:n + m, :vec]
    ref[:, :, vec:] = host[:, :, vec:]  # the oracle zero-fills whole parity vectors; the padding is the caller's
    enc = ENC[kind]()
    assert enc.Init(k, m, vec)
    dev = torch.from_numpy(host).cuda()
    p0, t0 = enc.encode_paths(), enc.tail_batches()
    enc.encode_blocks(dev, num_data=None if nd is None else _i16(nd), accumulate=accumulate)
    torch.cuda.synchronize()
    p1, t1 = enc.encode_paths(), enc.tail_batches()
    got = dev.cpu().numpy()
    assert np.array_equal(got, ref)
    assert t1["encode"] - t0["encode"] == expect_tail and t1["decode"] == t0["decode"]
    assert _moved(p0, p1) == {_enc_path(kind, k, m, nd is not None): 1}, _moved(p0, p1)


ENC_CASES = [
    # kind, k, m, vec, seg_stride, nblocks
    (NFEC_RS8, 64, 32, 1397, 1400, 6),
    (NFEC_RS8, 64, 16, 1460, 1464, 5),   # NORM's 1452-byte segments + 8
    (NFEC_RS8, 64, 8, 9, 16, 7),
    (NFEC_RS8, 32, 16, 1460, 1464, 5),
    (NFEC_RS8, 16, 4, 1401, 1408, 9),    # 1-byte tail
    (NFEC_RS8, 200, 55, 143, 144, 3),    # 7-byte tail, two pass sets
    (NFEC_RS8, 127, 128, 77, 80, 2),     # k + m = 255, more rows than a tail workgroup holds
    (NFEC_RS8, 10, 4, 5, 8, 11),         # no 8-byte piece: the tail kernel alone
    (NFEC_RS8, 3, 100, 1403, 1408, 3),
    (NFEC_MDP, 64, 32, 1460, 1464, 4),
    (NFEC_MDP, 30, 20, 203, 208, 5),
]


@pytest.mark.parametrize("kind,k,m,vec,stride,nb", ENC_CASES)
def test_encode_flat(orc, kind, k, m, vec, stride, nb):
    _encode_case(orc, kind, k, m, vec, stride, nb)


@pytest.mark.parametrize("invalid", [False, True])
@pytest.mark.parametrize("kind,k,m,vec", [(NFEC_RS8, 64, 32, 1460), (NFEC_RS8, 32, 16, 1397), (NFEC_MDP, 64, 32, 1397)])
def test_encode_shortened(orc, kind, k, m, vec, invalid):
    """per-block numData (q4's shortened form, the flat shortened runtime kernel, MDP's per-numData
    tables); blocks whose numData is 0 or k + 1 stay untouched in all their bytes"""
    nb = 13
    _encode_case(orc, kind, k, m, vec, _stride(vec), nb, nd=_num_data(k, nb, k + m + vec, invalid))


@pytest.mark.parametrize("k,m,vec", [(64, 32, 1397), (16, 4, 1401)])
def test_encode_accumulates_over_junk_parity(orc, k, m, vec):
    _encode_case(orc, NFEC_RS8, k, m, vec, _stride(vec), 5, accumulate=True)


def _oracle_decode(orc, kind, k, m, vec, blocks, locs, counts, nd):
    """the oracle's Decode per block; a list longer than m (undecodable) gives status 0 and leaves
    the block alone, as the reference's matrix build fails (normEncoderRS8.cpp:721-725)"""
    st = np.zeros(len(blocks), np.int32)
    for i in range(len(blocks)):
        if counts[i] > m or nd[i] < 1 or nd[i] > k:
            continue
        one = blocks[i:i + 1].copy()
        l1 = np.zeros((1, m), np.uint16)
        l1[0, :counts[i]] = locs[i, :counts[i]]
        st[i] = orc.decode_blocks(kind, k, m, vec, one, l1, counts[i:i + 1], nd[i:i + 1])[0]
        blocks[i] = one[0]
    return st


def _decode_case(orc, kind, k, m, vec, nb, nd, locs, counts, acc, expect_path, expect_tail=1):
    """encode with the oracle, erase (zero-fill, or junk under accumulate), repair on the device,
    compare statuses and every byte with the oracle's Decode"""
    rng = np.random.default_rng(k * 77 + m + vec + nb + int(acc))
    stride = _stride(vec)
    valid = (nd >= 1) & (nd <= k)
    host = orc.make_blocks(k, m, vec, nb, seg_stride=stride, num_data=np.clip(nd, 1, k))
    clean = host.copy()
    clean[valid] = orc.encode_blocks(kind, k, m, vec, host[valid].copy(), num_data=nd[valid])
    rx = clean.copy()
    for b in range(nb):
        for s in locs[b, :counts[b]]:
            rx[b, s] = rng.integers(0, 256, stride, dtype=np.uint8) if acc else 0
    rx[:, :, vec:] = rng.integers(0, 256, (nb, k + m, stride - vec), dtype=np.uint8)
    want = rx.copy()
    st_ref = _oracle_decode(orc, kind, k, m, vec, want, locs, counts, nd)
    assert np.array_equal(want[:, :, vec:], rx[:, :, vec:])  # the reference writes vec bytes only
    dec = DEC[kind]()
    assert dec.Init(k, m, vec)
    dev = torch.from_numpy(rx).cuda()
    p0, t0 = dec.decode_paths(), dec.tail_batches()
    shortened = not (nd == k).all()
    st = dec.decode_blocks(dev, _i16(locs), _i16(counts), num_data=_i16(nd) if shortened else None, accumulate=acc)
    torch.cuda.synchronize()
    p1, t1 = dec.decode_paths(), dec.tail_batches()
    got = dev.cpu().numpy()
    stg = st.cpu().numpy()
    assert np.array_equal(stg, st_ref), (stg, st_ref)
    assert np.array_equal(got, want)
    assert t1["decode"] - t0["decode"] == expect_tail and t1["encode"] == t0["encode"]
    assert _moved(p0, p1) == {expect_path: 1}, _moved(p0, p1)
    return st_ref


def _mixed_erasures(k, m, nb, nd, rng):
    """block kinds in turn: source only with e <= 16 (the fused kernel); source + the first parity
    rows, so the substitutes pass row 16 where m > 16 (the inverse by rank); more than 16 source
    (m = 32); nothing lost; parity only; e = m; and block 7 with m + 1 erasures (status 0)"""
    locs = np.zeros((nb, m + 1), np.uint16)
    counts = np.zeros(nb, np.uint16)
    for b in range(nb):
        n = int(np.clip(nd[b], 1, k))
        kind = b % 6
        par = None
        if kind == 0:
            es = int(rng.integers(1, min(16, m) + 1))
        elif kind == 1:
            es = int(rng.integers(1, min(8, m - 1) + 1))
            es = min(es, n)
            par = np.arange(min(16, m - es))
        elif kind == 2:
            es = m // 2 + 4 if m > 16 else m
        elif kind == 3:
            es = 0
        elif kind == 4:
            es, par = 0, np.sort(rng.choice(m, int(rng.integers(1, m + 1)), replace=False))
        else:
            es = min(n, m // 2)
            par = np.sort(rng.choice(m, m - es, replace=False))
        es = min(es, n, m)
        src = np.sort(rng.choice(n, es, replace=False))
        e = np.concatenate([src, n + (par if par is not None else np.zeros(0, int))])
        if b == 7:
            e = np.sort(rng.choice(n + m, min(n + m, m + 1), replace=False))
        locs[b, :len(e)] = e
        counts[b] = len(e)
    return locs, counts


@pytest.mark.parametrize("mode", ["unshortened", "num_data", "accumulate"])
def test_repair_fixed_64_32_every_block_kind(orc, mode):
    k, m, vec, nb = 64, 32, 1397, 24
    nd = np.full(nb, k, np.uint16)
    if mode == "num_data":
        nd = _num_data(k, nb, 99)
        nd[13], nd[14] = 0, k + 1   # invalid numData: status 0, left alone
    locs, counts = _mixed_erasures(k, m, nb, nd, np.random.default_rng(5 + len(mode)))
    st = _decode_case(orc, NFEC_RS8, k, m, vec, nb, nd, locs, counts, mode == "accumulate", "fixed")
    assert st[7] == 0 and (st[np.arange(nb) % 6 == 0] > 0).all()


@pytest.mark.parametrize("k,m,vec,nb", [(64, 16, 1460, 10), (64, 8, 13, 12)])
def test_repair_fixed_other_shapes(orc, k, m, vec, nb):
    """(64, 8) x 13 bytes: one 8-byte piece on the fused kernel and a 5-byte tail"""
    nd = np.full(nb, k, np.uint16)
    locs, counts = _mixed_erasures(k, m, nb, nd, np.random.default_rng(k + m + vec))
    _decode_case(orc, NFEC_RS8, k, m, vec, nb, nd, locs, counts, False, "fixed")


def _plain_erasures(orc, k, m, nb, es, ep, nd):
    locs = np.zeros((nb, m), np.uint16)
    counts = np.zeros(nb, np.uint16)
    for b in range(nb):
        n = int(nd[b])
        src = orc.erasure_pattern(b, n, min(es, n))
        par = (n + orc.erasure_pattern(b + 9000, m, ep)).astype(np.uint16) if ep else np.zeros(0, np.uint16)
        e = np.sort(np.concatenate([src, par]))[:m]
        locs[b, :len(e)] = e
        counts[b] = len(e)
    return locs, counts


REPAIR_CASES = [
    # kind, k, m, vec, nblocks, source erasures, parity erasures, numData (None: k)
    (NFEC_RS8, 32, 16, 1460, 9, 10, 4, None),
    (NFEC_RS8, 200, 55, 143, 4, 40, 10, [200, 150, 199, 60]),   # two passes of the pass-major table
    (NFEC_RS8, 10, 7, 5, 20, 7, 0, None),                        # e = m, no 8-byte piece
    (NFEC_MDP, 64, 32, 1460, 6, 16, 0, None),
    (NFEC_MDP, 30, 20, 203, 5, 12, 5, [30, 20, 29, 13, 30]),
]


@pytest.mark.parametrize("kind,k,m,vec,nb,es,ep,nd", REPAIR_CASES)
def test_repair_runtime_kernel(orc, kind, k, m, vec, nb, es, ep, nd):
    nd = np.full(nb, k, np.uint16) if nd is None else np.array(nd, np.uint16)
    locs, counts = _plain_erasures(orc, k, m, nb, es, ep, nd)
    st = _decode_case(orc, kind, k, m, vec, nb, nd, locs, counts, False, "runtime")
    assert (st == counts).all()


@pytest.mark.parametrize("k,m,vec", [(64, 32, 1400), (32, 16, 1408)])
def test_multiples_of_8_launch_no_tail_kernel(orc, k, m, vec):
    nb = 6
    _encode_case(orc, NFEC_RS8, k, m, vec, vec, nb, expect_tail=0)
    nd = np.full(nb, k, np.uint16)
    locs, counts = _plain_erasures(orc, k, m, nb, m // 2, 2, nd)
    _decode_case(orc, NFEC_RS8, k, m, vec, nb, nd, locs, counts, False, "fixed" if (k, m) in FIXED_RS8 else "runtime",
                 expect_tail=0)


def test_host_entries_inherit_the_tails(orc):
    """nfec_encode_host / nfec_decode_host stage the batch and run the same device functions"""
    k, m, vec, nb = 32, 16, 1460, 8
    stride = _stride(vec)
    enc, dec = NormEncoderRS8(), NormDecoderRS8()
    assert enc.Init(k, m, vec) and dec.Init(k, m, vec)
    host = orc.make_blocks(k, m, vec, nb, seg_stride=stride)
    host[:, :, vec:] = 0xA5
    host[:, k:, :vec] = 0x3C   # stale parity must be overwritten
    ref = orc.encode_blocks(NFEC_RS8, k, m, vec, host.copy())
    ref[:, :, vec:] = 0xA5
    t0 = enc.tail_batches()["encode"]
    enc.encode_blocks_host(host)
    assert np.array_equal(host, ref)
    assert enc.tail_batches()["encode"] > t0
    locs, counts = _plain_erasures(orc, k, m, nb, 10, 4, np.full(nb, k, np.uint16))
    for b in range(nb):
        for s in locs[b, :counts[b]]:
            host[b, s, :vec] = 0
    want = host.copy()
    st_ref = orc.decode_blocks(NFEC_RS8, k, m, vec, want, locs, counts)
    t0 = dec.tail_batches()["decode"]
    st = dec.decode_blocks_host(host, locs, counts)
    assert np.array_equal(st, st_ref) and (st == counts).all()
    assert np.array_equal(host, want)
    assert np.array_equal(host[:, :k], ref[:, :k])
    assert dec.tail_batches()["decode"] > t0
