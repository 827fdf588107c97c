"""RS8(64,32) encode on the 3-role-wave Karatsuba kernel (rs8_enc_t3.hip), byte for byte against the
oracle.

The kernel walks the batch as rs8_enc_d2.hip does (a flat list of 16-byte pairs, 128 per workgroup,
fetched by 16-byte LDS-DMA pieces) and takes exactly its batches, so the cases are that kernel's:
segments of half a pair, one pair and one and a half pairs (vec 8, 16, 24), the 1,400-byte segment
whose last pair is half valid and its 1,408-byte neighbour; 1, 3 and 47 blocks; strides longer
than the vector with junk in the padding; a batch that starts 8 mod 16; vec 1460, where this
kernel takes 1,456 bytes and the tail kernel the rest; accumulate; and a shortened batch, which
must still reach the 4-role-wave kernels.  Every comparison is over the whole buffer: sources,
padding, the bytes in front of the batch and behind its last block must come back unchanged.

Where the diagnostic library is loaded (NFEC_LIBRARY), every case also runs with NFEC_ENC_T3=0
(the 2-role-wave kernel) and with NFEC_ENC_T3=0 NFEC_ENC_D2=0 (the 4-role-wave kernel), and all
three must give the oracle's bytes."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from norm_amd import NFEC_RS8, NormEncoderRS8, _native  # noqa: E402

K, M = 64, 32
DIAG = "diag" in os.path.basename(_native.LIB_PATH)
LEAD = 16     # sentinel bytes in front of the batch (8: the batch starts 8 mod 16)
TAIL = 64     # sentinel bytes behind the last block
KNOBS = [{}, {"NFEC_ENC_T3": "0"}, {"NFEC_ENC_T3": "0", "NFEC_ENC_D2": "0"}] if DIAG else [{}]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from norm_amd import device_count

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    assert device_count() >= 1, "no gfx950 device visible to libnfec"


def _i16(a):
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.uint16).view(np.int16)).cuda()


def _case(orc, vec, stride, nb, lead=LEAD, nd=None, accumulate=False, expect_tail=0):
    rng = np.random.default_rng(vec * 7919 + stride * 31 + nb + lead)
    blocks = orc.make_blocks(K, M, vec, nb, seg_stride=stride, num_data=nd)
    for b in range(nb):   # junk in the parity slots and past them, and in every slot's padding
        n = K if nd is None else int(nd[b])
        blocks[b, n:] = rng.integers(0, 256, (K + M - n, stride), dtype=np.uint8)
    blocks[:, :, vec:] = rng.integers(0, 256, (nb, K + M, stride - vec), dtype=np.uint8)
    ref = orc.encode_blocks(NFEC_RS8, K, M, vec, blocks.copy(), num_data=nd)
    for b in range(nb):
        n = K if nd is None else int(nd[b])
        if accumulate:
            ref[b, n:n + M, :vec] ^= blocks[b, n:n + M, :vec]
        ref[b, n + M:] = blocks[b, n + M:]
    ref[:, :, vec:] = blocks[:, :, vec:]   # the oracle zero-fills whole parity vectors; the padding is the caller's
    flat = np.concatenate([rng.integers(0, 256, lead, dtype=np.uint8), blocks.reshape(-1),
                           rng.integers(0, 256, TAIL, dtype=np.uint8)])
    want = flat.copy()
    want[lead:lead + blocks.size] = ref.reshape(-1)
    for knobs in KNOBS:
        for name in ("NFEC_ENC_T3", "NFEC_ENC_D2"):
            os.environ.pop(name, None)
        os.environ.update(knobs)
        try:
            enc = NormEncoderRS8()
            assert enc.Init(K, M, vec)
            dev = torch.from_numpy(flat).cuda()
            assert dev.data_ptr() % 256 == 0
            view = dev[lead:lead + blocks.size].view(nb, K + M, stride)
            assert view.data_ptr() % 16 == lead % 16
            t0 = enc.tail_batches()["encode"]
            enc.encode_blocks(view, num_data=None if nd is None else _i16(nd), accumulate=accumulate)
            torch.cuda.synchronize()
            got = dev.cpu().numpy()
            assert enc.tail_batches()["encode"] - t0 == expect_tail
        finally:
            for name in ("NFEC_ENC_T3", "NFEC_ENC_D2"):
                os.environ.pop(name, None)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (knobs, bad.size, bad[:8] - lead)


@pytest.mark.parametrize("vec", [8, 16, 24, 1400, 1408])
def test_encode_matches_the_oracle(orc, vec):
    for nb in (1, 3, 47):
        _case(orc, vec, vec, nb)


@pytest.mark.parametrize("stride", [1408, 1416])
def test_padded_segments_keep_their_padding(orc, stride):
    _case(orc, 1400, stride, 3)
    _case(orc, 1400, stride, 47)


@pytest.mark.parametrize("vec,stride", [(1400, 1400), (1408, 1408), (24, 24), (1400, 1416)])
def test_batch_base_8_mod_16(orc, vec, stride):
    _case(orc, vec, stride, 5, lead=8)


def test_vec_1460_splits_with_the_tail_kernel(orc):
    _case(orc, 1460, 1464, 5, expect_tail=1)
    _case(orc, 1460, 1464, 5, lead=8, expect_tail=1)


@pytest.mark.parametrize("vec", [24, 1400])
def test_accumulate(orc, vec):
    _case(orc, vec, vec, 7, accumulate=True)


def test_shortened_batch_still_reaches_q4(orc):
    nd = np.array([64, 63, 1, 17, 64, 32, 48], np.uint16)
    _case(orc, 1400, 1400, len(nd), nd=nd)
