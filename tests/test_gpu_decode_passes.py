"""Decode batches past one pass, on every route of dispatch_decode.cpp.

nfec_decode cuts a device batch into passes (decode_device_impl, decode_rs16_tw) and addresses
each pass by hand: blocks, numData, erasure lists, counts and status move by the pass's first
block, the fixed route's gate gets a new generation, and pass n + 1 reuses the workspace of
pass n.  A dropped offset or a stale workspace row passes every batch whose blocks all look
alike, so the batches here are composed from a library of L = 97 different blocks (erasure
count, source / parity loss, numData, status, one undecodable list) by a fixed-seed random index
map: the oracle (Encode per segment, normObject.cpp:2203-2229; Decode, normObject.cpp:1548-1644)
runs once on the library, and block b of the batch is expected to come out as the library's
block pat[b], every byte of every slot, the stride padding (a sentinel) included.

The tests rely only on nblocks > max_pass meaning at least two passes: decode_pass_size may pick
smaller ones.  Segments are 10 to 16 bytes, so the largest batch is 134 MB."""
import ctypes
import functools
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from norm_amd import (NFEC_MDP, NFEC_RS8, NFEC_RS16, NormDecoderMDP, NormDecoderRS8,  # noqa: E402
                      NormDecoderRS16, NormEncoderMDP, NormEncoderRS8, NormEncoderRS16)
from norm_amd import _native as N  # noqa: E402
from norm_amd.codec import _batch_struct, _stream_handle, _tensor_ptr  # noqa: E402

ENC = {NFEC_RS8: NormEncoderRS8, NFEC_RS16: NormEncoderRS16, NFEC_MDP: NormEncoderMDP}
DEC = {NFEC_RS8: NormDecoderRS8, NFEC_RS16: NormDecoderRS16, NFEC_MDP: NormDecoderMDP}

MAX_PASS = 65536        # decode_route: r.max_pass of every route but RS8_RT (decode_rs16_tw: the same cap)
MAX_PASS_RT = 1 << 20   # decode_route: r.max_pass on the RS8_RT route
EXTRA = 101
L = 97                  # library blocks per case
SENTINEL = 0xA5         # bytes [vec, seg_stride) of every slot: never written

# route: the decode_paths() counter; short: the route takes shortened batches; opts: codec options
Case = namedtuple("Case", "id kind k m vec stride nblocks max_pass route short opts enc_path")
SHARED = N.NFEC_OPT_RS16_SHARED_TABLES
CASES = [
    Case("fixed-64-32", NFEC_RS8, 64, 32, 12, 16, MAX_PASS + EXTRA, MAX_PASS, "fixed", True, 0, "fixed"),
    Case("fixed-64-16", NFEC_RS8, 64, 16, 12, 16, MAX_PASS + EXTRA, MAX_PASS, "fixed", True, 0, "fixed"),
    Case("fixed-64-8", NFEC_RS8, 64, 8, 12, 16, MAX_PASS + EXTRA, MAX_PASS, "fixed", True, 0, "fixed"),
    # one pass over a grid the route has not launched before, then two passes
    Case("rt-5-3", NFEC_RS8, 5, 3, 12, 16, MAX_PASS + EXTRA, MAX_PASS_RT, "runtime", True, 0, "runtime"),
    Case("rt-5-3-2p", NFEC_RS8, 5, 3, 12, 16, MAX_PASS_RT + EXTRA, MAX_PASS_RT, "runtime", True, 0, "runtime"),
    Case("mdp-10-4", NFEC_MDP, 10, 4, 12, 16, MAX_PASS + EXTRA, MAX_PASS, "runtime", True, 0, "runtime"),
    # one 8-byte piece and a 2-byte tail; vec 11: the odd last byte stays as it is
    Case("tower-v10", NFEC_RS16, 40, 10, 10, 16, MAX_PASS + EXTRA, MAX_PASS, "rs16_tower", True, 0, "rs16_product"),
    Case("tower-v11", NFEC_RS16, 40, 10, 11, 16, MAX_PASS + EXTRA, MAX_PASS, "rs16_tower", True, 0, "rs16_product"),
    # vec 16, unshortened: the product-kernel stage 1; vec 10: every block on the gather stage
    Case("generic-v16", NFEC_RS16, 40, 10, 16, 16, MAX_PASS + EXTRA, MAX_PASS, "generic", False, SHARED, "rs16_product"),
    Case("generic-v10", NFEC_RS16, 40, 10, 10, 16, MAX_PASS + EXTRA, MAX_PASS, "generic", True, SHARED, "generic"),
]
BY_ID = {c.id: c for c in CASES}
ALL = [pytest.param(c, id=c.id) for c in CASES]
RS = [pytest.param(c, id=c.id) for c in CASES if c.kind != NFEC_MDP]
ABI = [pytest.param(BY_ID[i], id=i) for i in ("fixed-64-32", "tower-v10")]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from norm_amd import device_count

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    assert device_count() >= 1, "no gfx950 device visible to libnfec"


def _cov(c):
    """bytes of a vector the code covers: RS16 codes vec / 2 symbols (normEncoderRS16.cpp:479)"""
    return c.vec & ~1 if c.kind == NFEC_RS16 else c.vec


def _gate_class(nd, m, locs, count):
    """rs_plan2_kernel's rule for one block.  None: nothing to repair (no source erased, or
    undecodable), the gate stays as it is; True: the fused kernel takes it (1..16 source erasures,
    substitute parity rows below min(16, m)); False: it opens the gate for the unfused kernels"""
    if count > m:
        return None
    e = locs[:count].astype(int)
    es = int((e < nd).sum())
    if es == 0:
        return None
    lost = set(e[e >= nd] - nd)
    used = [p for p in range(m) if p not in lost][:es]
    return es <= 16 and used[-1] < min(16, m)


@functools.lru_cache(maxsize=None)
def _library(cid):
    """The case's L blocks: encode input and output, received bytes and the oracle's repair
    (overwrite and accumulate), statuses, reception masks.  Built once per case, only read."""
    from oracle import pyoracle as orc

    c = BY_ID[cid]
    k, m, vec, n, cov = c.k, c.m, c.vec, c.k + c.m, _cov(c)
    rng = np.random.default_rng(1000 + CASES.index(c))
    nd = np.full(L, k, np.uint16)
    if c.short:
        nd[9:] = rng.integers(1, k + 1, L - 9)
        nd[9:13] = [1, k - 1, max(1, k // 2), k]
    ls = m + 1  # room for the undecodable list
    locs = np.zeros((L, ls), np.uint16)
    counts = np.zeros(L, np.uint16)
    for i in range(L):
        n_d = int(nd[i])
        lo = min(n_d, m)
        ep_fixed = max(1, m // 2 - 1)
        named = {
            0: (0, []),                                            # nothing lost
            1: (1, []),
            2: (lo, []),                                           # all the block can lose
            3: (max(1, lo // 2), []),
            # the first parity rows lost: the substitutes move up (m = 32: to rows 15 and 16)
            4: (max(1, min(2, n_d, m - ep_fixed)), list(range(ep_fixed))),
            6: (0, sorted(rng.choice(m, max(1, m // 3), replace=False))),   # parity only
            7: (min(17, lo), []),                                  # m = 32: one past the fused kernel
            8: (min(n_d, m // 2), None),                           # source and every parity row left
            9: (1, []),                                            # numData = 1
        }
        if i == 5:  # one more than m, anywhere in the block: undecodable
            e = np.sort(rng.choice(n_d + m, m + 1, replace=False))
        else:
            if i in named:
                es, par = named[i]
                if par is None:
                    par = sorted(rng.choice(m, m - es, replace=False))
            else:  # test_gpu_random.py's draw
                es = int(rng.integers(0, lo + 1))
                ep = int(rng.integers(0, m - es + 1)) if rng.integers(0, 3) == 0 else 0
                par = sorted(rng.choice(m, ep, replace=False))
            e = np.concatenate([np.sort(rng.choice(n_d, es, replace=False)), n_d + np.asarray(par, int)])
        locs[i, :len(e)] = e
        counts[i] = len(e)
    ndo = nd if c.short else None
    decodable = counts <= m

    # encode: parity slots (and a shortened block's slots past them) hold junk, the padding a sentinel
    enc_in = orc.make_blocks(k, m, vec, L, seg_stride=c.stride, num_data=ndo, seed=orc.SEED + CASES.index(c))
    for i in range(L):
        enc_in[i, nd[i]:, :vec] = rng.integers(0, 256, (n - nd[i], vec), dtype=np.uint8)
    enc_in[:, :, vec:] = SENTINEL
    clean = orc.encode_blocks(c.kind, k, m, vec, enc_in.copy(), ndo)
    for i in range(L):  # (the oracle zero-fills whole parity vectors first; the code leaves an odd last byte)
        clean[i, nd[i]:nd[i] + m, cov:vec] = enc_in[i, nd[i]:nd[i] + m, cov:vec]

    # decode, overwrite: erased slots zeroed (NORM's zero-fill), an uncoded last byte holds junk
    rx = clean.copy()
    rx_acc = clean.copy()
    for i in range(L):
        for s in locs[i, :counts[i]]:
            junk = rng.integers(0, 256, vec, dtype=np.uint8)
            rx[i, s, :cov] = 0
            rx[i, s, cov:vec] = junk[cov:]
            if s < nd[i]:
                rx_acc[i, s, :vec] = junk   # accumulate: the repair is XORed into what is there
            else:
                rx_acc[i, s, :cov] = 0
    want = rx.copy()
    status = np.zeros(L, np.int32)  # an undecodable list: status 0, the block as received
    sub = want[decodable].copy()
    status[decodable] = orc.decode_blocks(c.kind, k, m, vec, sub, locs[decodable], counts[decodable],
                                          nd[decodable] if c.short else None)
    want[decodable] = sub
    want_acc = rx_acc.copy()
    mask = np.zeros((L, (n + 31) // 32), np.uint32)
    status_rx = status.copy()
    gate = []
    for i in range(L):
        src = [int(s) for s in locs[i, :counts[i]] if s < nd[i]]
        if decodable[i]:
            # the premise of composing expectations from the library: Decode returns its count and
            # brings back the clean source
            assert status[i] == counts[i], (cid, i)
            assert np.array_equal(want[i, :nd[i], :cov], clean[i, :nd[i], :cov]), (cid, i)
            for s in src:
                want_acc[i, s, :cov] ^= clean[i, s, :cov]
        bits = np.ones(n, bool)
        bits[locs[i, :counts[i]]] = False
        for s in np.nonzero(bits)[0]:
            mask[i, s // 32] |= np.uint32(1 << (s % 32))
        if not src:  # nfec_rx_erasures lists nothing for a block with no source missing (nfec.h)
            status_rx[i] = 0
        gate.append(_gate_class(int(nd[i]), m, locs[i], int(counts[i])))
    assert not np.array_equal(want[5], clean[5]) and status[5] == 0

    # every group the batches must hold
    es = np.array([int((locs[i, :counts[i]] < nd[i]).sum()) for i in range(L)])
    ep = counts.astype(int) - es
    assert (counts == 0).any() and (counts == 1).any() and (counts == m + 1).sum() == 1
    assert ((es == np.minimum(nd, m)) & decodable).any() and ((es > 1) & (es < np.minimum(nd, m)) & decodable).any()
    assert ((es > 0) & (ep == 0)).any() and ((es > 0) & (ep > 0) & decodable).any()
    if c.short:
        assert {1, k}.issubset(set(nd.tolist())) and len(set(nd.tolist())) >= 3
    return SimpleNamespace(nd=nd, locs=locs, counts=counts, enc_in=enc_in, clean=clean, rx=rx, want=want,
                           rx_acc=rx_acc, want_acc=want_acc, status=status, mask=mask, status_rx=status_rx,
                           quiet=np.array([g is not False for g in gate]), unfused=np.array([g is False for g in gate]))


def _up(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def _pat(c, seed=0, among=None):
    rng = np.random.default_rng(77 + 13 * CASES.index(c) + seed)
    idx = np.arange(L) if among is None else np.nonzero(among)[0]
    return idx[rng.integers(0, len(idx), c.nblocks)]


def _same(c, got, want, pat, what):
    """every byte (status) of every block; names the first block that differs"""
    if torch.equal(got, want):
        return
    bad = (got != want).reshape(got.shape[0], -1).any(1)
    b = int(bad.nonzero()[0])
    npass = -(-len(pat) // c.max_pass)
    sb = -(-len(pat) // npass)
    pytest.fail(f"{c.id} {what}: {int(bad.sum())} of {len(pat)} blocks differ, the first is block {b} "
                f"(library pattern {int(pat[b])}), in pass {b // sb} of {npass} if the passes are equal")


def _delta(before, after):
    return {p: after[p] - before[p] for p in after if after[p] != before[p]}


def _decoder(c):
    dec = DEC[c.kind](options=c.opts) if c.opts else DEC[c.kind]()
    assert dec.Init(c.k, c.m, c.vec)
    return dec


def _decode(c, lib, dec, pat, accumulate=False, how="blocks"):
    """decode the batch lib[pat] and compare bytes and statuses with the library's; how: "blocks"
    (decode_blocks), "null" (nfec_decode with status NULL) or "received" (nfec_decode_received)"""
    p = _up(pat.astype(np.int64))
    dev = _up(lib.rx_acc if accumulate else lib.rx)[p]
    want = _up(lib.want_acc if accumulate else lib.want)[p]
    ndev = _up(lib.nd)[p] if c.short else None
    assert not torch.equal(dev, want)   # (the batch needs repair)
    p0, t0 = dec.decode_paths(), dec.tail_batches()["decode"]
    st = None
    if how == "received":
        st = dec.decode_received(dev, _up(lib.mask)[p].contiguous(), num_data=ndev, accumulate=accumulate)
    else:
        locs, counts = _up(lib.locs)[p].contiguous(), _up(lib.counts)[p]
        if how == "null":
            b = _batch_struct(dev, ndev, accumulate)
            N.check(N.lib().nfec_decode(dec._h, ctypes.byref(b), _tensor_ptr(locs, "locs"), locs.shape[1],
                                        _tensor_ptr(counts, "counts"), None, _stream_handle(None)), "nfec_decode")
        else:
            st = dec.decode_blocks(dev, locs, counts, num_data=ndev, accumulate=accumulate)
    torch.cuda.synchronize()
    assert _delta(p0, dec.decode_paths()) == {c.route: 1}
    if c.kind != NFEC_RS16 and c.vec % 8:   # (the counter is the RS8 / MDP tail kernels')
        assert dec.tail_batches()["decode"] == t0 + 1
    if st is not None:
        _same(c, st, _up(lib.status_rx if how == "received" else lib.status)[p], pat, "status")
    _same(c, dev, want, pat, "bytes")


@pytest.mark.parametrize("c", ALL)
def test_encode_matches_library(c):
    """the same block counts through the encode ladder's flat launches"""
    lib = _library(c.id)
    enc = ENC[c.kind](options=c.opts | N.NFEC_OPT_RS16_TOEPLITZ_OFF) if c.kind == NFEC_RS16 else ENC[c.kind]()
    assert enc.Init(c.k, c.m, c.vec)
    pat = _pat(c)
    p = _up(pat.astype(np.int64))
    dev = _up(lib.enc_in)[p]
    p0, t0 = enc.encode_paths(), enc.tail_batches()["encode"]
    enc.encode_blocks(dev, num_data=_up(lib.nd)[p] if c.short else None)
    torch.cuda.synchronize()
    assert _delta(p0, enc.encode_paths()) == {c.enc_path: 1}
    if c.kind != NFEC_RS16 and c.vec % 8:
        assert enc.tail_batches()["encode"] == t0 + 1
    _same(c, dev, _up(lib.clean)[p], pat, "encode")


@pytest.mark.parametrize("c", ALL)
def test_decode_overwrite(c):
    _decode(c, _library(c.id), _decoder(c), _pat(c, 1))


@pytest.mark.parametrize("c", RS)
def test_decode_accumulate(c):
    """erased source buffers hold junk per pattern; the repair is XORed into it"""
    _decode(c, _library(c.id), _decoder(c), _pat(c, 2), accumulate=True)


def test_mdp_refuses_accumulate():
    c = BY_ID["mdp-10-4"]
    lib = _library(c.id)
    dec = _decoder(c)
    p = _up(np.arange(7, dtype=np.int64))
    dev = _up(lib.rx)[p]
    with pytest.raises(N.NfecError) as err:
        dec.decode_blocks(dev, _up(lib.locs)[p].contiguous(), _up(lib.counts)[p], num_data=_up(lib.nd)[p],
                          accumulate=True)
    assert err.value.code == N.NFEC_ENOTSUP
    torch.cuda.synchronize()
    assert torch.equal(dev, _up(lib.rx)[p])


@pytest.mark.parametrize("c", ALL)
def test_small_large_small_on_one_decoder(c):
    """the workspace regrows between the calls, and the gate generation carries over"""
    lib, dec = _library(c.id), _decoder(c)
    small = np.array([1, 2, 4, 5, 0, 7, 8])
    _decode(c, lib, dec, small)
    _decode(c, lib, dec, _pat(c, 3))
    _decode(c, lib, dec, small)


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("where", ["first", "last", "both"])
def test_fixed_route_gate_per_pass(where, accumulate):
    """Blocks the fused kernel does not take (e = 17, or a lost parity row that moves a substitute
    to row 16 or past it) only in the first 50 blocks (the first pass whatever its size), only in
    the last 50 (the last pass), or both; every other block is one the fused kernel takes or one
    with nothing to repair.  A pass whose gate stays shut must leave its blocks to the fused
    kernel; a pass whose gate opens must not touch what the fused kernel repaired (under
    accumulate a second repair would XOR the source away)."""
    c = BY_ID["fixed-64-32"]
    lib = _library(c.id)
    assert lib.unfused.sum() >= 3 and lib.quiet.sum() >= 30
    pat = _pat(c, 4, among=lib.quiet)
    rng = np.random.default_rng(5)
    unfused = np.nonzero(lib.unfused)[0]
    if where in ("first", "both"):
        pat[:50] = unfused[rng.integers(0, len(unfused), 50)]
    if where in ("last", "both"):
        pat[-50:] = unfused[rng.integers(0, len(unfused), 50)]
    _decode(c, lib, _decoder(c), pat, accumulate=accumulate)


@pytest.mark.parametrize("c", ABI)
def test_null_status(c):
    """nfec_decode with status NULL: the plan writes the codec's own status array, per pass"""
    _decode(c, _library(c.id), _decoder(c), _pat(c, 6), how="null")


@pytest.mark.parametrize("c", ABI)
def test_decode_received(c):
    """the erasure lists from per-block reception masks (bit s set unless slot s is in the
    pattern's list), lists and counts in the codec's workspace; nfec_rx_erasures lists nothing
    for a block that misses parity only, whose status is then 0"""
    _decode(c, _library(c.id), _decoder(c), _pat(c, 7), how="received")
