"""Branches of the host-resident batch pipeline (norm_amd/csrc/host_pipeline.cpp) that the other
host tests leave out.

Strided host encode that accumulates or is shortened: the chunk's whole block span goes up and
comes down (not source up / parity down).  Strided host decode with accumulate over non-zero
erased slots.  Both at a padded stride, pinned and pageable, in chunks of 4 of 12 blocks: one
chunk per pipeline slot.

The window-DMA decode.  The product library moves a host decode's bytes by the zero-copy slot
kernels (pinned staging is always device-mapped on this hardware): up the surviving source and
the first e surviving parities of each block, down the repaired slots; that is the path
test_host_decode_windows, test_host_batch_pipeline and test_decode_vectors_matches_oracle run.
The window DMA stays for setups without the mapping: up [0, the last parity slot a block of the
chunk uses), down [0, max numData) of the chunk, the staged chunk both ways for segment lists.
Where the diagnostic library is loaded (NFEC_LIBRARY), NFEC_HOST_ZC=0 selects it, and this module
then runs those three tests' cases, and the accumulating decode, once more through it.  The
product library ignores the knob, so there the second passes are not defined."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import test_gpu_parity as P  # noqa: E402
import test_gpu_vectors as V  # noqa: E402
from norm_amd import NFEC_RS8, _native  # noqa: E402

DIAG = "diag" in os.path.basename(_native.LIB_PATH)
# RS8(20,12) x 1000 B at a padded stride, 12 blocks
KIND, K, M, VEC, STRIDE, NB = NFEC_RS8, 20, 12, 1000, 1008, 12


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from norm_amd import device_count

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    assert device_count() >= 1, "no gfx950 device visible to libnfec"


def _buffer(arr, pinned):
    """a copy of arr in page-locked (pinned) or pageable host memory"""
    if not pinned:
        return arr.copy()
    buf = torch.empty(arr.shape, dtype=torch.uint8).pin_memory().numpy()
    buf[...] = arr
    return buf


@pytest.mark.parametrize("pinned", [False, True])
@pytest.mark.parametrize("case", ["accumulate", "shortened"])
def test_host_encode_whole_span(orc, case, pinned, monkeypatch):
    """accumulate: parity ^= what the parity slots held (as test_encode_accumulates_like_reference);
    shortened: numData of k, k - 1 and 1, parity in [numData, numData + m), the slots past it
    untouched.  Padding stays 0xA5."""
    monkeypatch.setenv("NFEC_HOST_CHUNK_BLOCKS", "4")
    enc, _ = P._codecs(KIND, K, M, VEC)
    nd = np.array([K, K - 1, 1] * 4, np.uint16) if case == "shortened" else None
    base = orc.make_blocks(K, M, VEC, NB, seg_stride=STRIDE, num_data=nd)
    ref = orc.encode_blocks(KIND, K, M, VEC, base.copy(), nd)
    junk = np.random.default_rng(3).integers(0, 256, (NB, K + M, VEC), dtype=np.uint8)
    expect = base.copy()
    for b in range(NB):
        n = K if nd is None else int(nd[b])
        base[b, n:, :VEC] = junk[b, n:]            # stale bytes in the parity slots and past them
        expect[b, n:, :VEC] = junk[b, n:]
        expect[b, n:n + M, :VEC] = ref[b, n:n + M, :VEC] ^ (junk[b, n:n + M] if case == "accumulate" else 0)
    base[:, :, VEC:] = 0xA5
    expect[:, :, VEC:] = 0xA5
    host = _buffer(base, pinned)
    enc.encode_blocks_host(host, num_data=nd, accumulate=case == "accumulate")
    assert np.all(host[:, :, VEC:] == 0xA5)
    assert np.array_equal(host, expect)


@pytest.mark.parametrize("pinned", [False, True])
def test_host_decode_accumulates(orc, pinned, monkeypatch):
    """junk ^ data in the erased source slots, as the reference's Decode leaves them
    (test_decode_accumulates_into_nonzero_erased_buffers), in every chunk; padding untouched."""
    monkeypatch.setenv("NFEC_HOST_CHUNK_BLOCKS", "4")
    _, dec = P._codecs(KIND, K, M, VEC)
    base = orc.encode_blocks(KIND, K, M, VEC, orc.make_blocks(K, M, VEC, NB, seg_stride=STRIDE))
    locs, counts = P._erasures(orc, KIND, K, M, NB, 6, 1)
    rng = np.random.default_rng(7)
    for b in range(NB):
        for s in locs[b, : counts[b]]:
            base[b, s, :VEC] = rng.integers(0, 256, VEC, dtype=np.uint8)
    base[:, :, VEC:] = 0xA5
    ref = base.copy()
    st_ref = orc.decode_blocks(KIND, K, M, VEC, ref, locs, counts)
    assert np.all(ref[:, :, VEC:] == 0xA5)
    host = _buffer(base, pinned)
    st = dec.decode_blocks_host(host, locs, counts, accumulate=True)
    assert np.array_equal(st, st_ref)
    assert np.array_equal(host, ref)


def _cases_of(test):
    """the parametrize marks of another module's test"""
    def apply(fn):
        for mk in test.pytestmark:
            fn = getattr(pytest.mark, mk.name)(*mk.args, **mk.kwargs)(fn)
        return fn
    return apply


if DIAG:
    @pytest.fixture
    def window_dma(monkeypatch):
        monkeypatch.setenv("NFEC_HOST_ZC", "0")
        return monkeypatch

    @_cases_of(P.test_host_batch_pipeline)
    def test_host_batch_pipeline_window_dma(orc, kind, k, m, vec, stride, nb, pinned, window_dma):
        P.test_host_batch_pipeline(orc, kind, k, m, vec, stride, nb, pinned, window_dma)

    @_cases_of(P.test_host_decode_windows)
    def test_host_decode_windows_window_dma(orc, kind, pinned, window_dma):
        P.test_host_decode_windows(orc, kind, pinned, window_dma)

    @_cases_of(V.test_decode_vectors_matches_oracle)
    def test_decode_vectors_window_dma(orc, kind, k, m, vec, nb, es, ep, window_dma):
        window_dma.setenv("NFEC_HOST_CHUNK_BLOCKS", "300")  # test_gpu_vectors' several chunks per batch
        V.test_decode_vectors_matches_oracle(orc, kind, k, m, vec, nb, es, ep)

    @_cases_of(test_host_decode_accumulates)
    def test_host_decode_accumulates_window_dma(orc, pinned, window_dma):
        test_host_decode_accumulates(orc, pinned, window_dma)
