"""nfec_codec_tail_batches at the C-ABI boundary: how many device batches had their last
vector_size % 8 bytes computed by the segment-tail kernels beside the fast kernels (RS8 / MDP
vectors of any length, norm_amd/csrc/kernels_gf8tail.hip).  No GPU is touched here."""
import ctypes

from norm_amd import NormDecoderRS8, NormEncoderMDP, NormEncoderRS8
from norm_amd import _native as N


def test_tail_batches_declared_and_exported():
    assert "nfec_codec_tail_batches" in N.declared_symbols()
    assert hasattr(N.lib(), "nfec_codec_tail_batches")


def test_tail_batches_rejects_null_arguments():
    cnt = (ctypes.c_uint64 * 2)()
    assert N.lib().nfec_codec_tail_batches(None, cnt, 2) == N.NFEC_EINVAL
    enc = NormEncoderRS8(options=N.NFEC_OPT_HOST_ONLY)
    assert enc.Init(16, 4, 61)
    assert N.lib().nfec_codec_tail_batches(enc._h, None, 2) == N.NFEC_EINVAL


def test_host_only_codec_reports_no_tail_batches():
    for cls in (NormEncoderRS8, NormDecoderRS8, NormEncoderMDP):
        c = cls(options=N.NFEC_OPT_HOST_ONLY)
        assert c.Init(64, 32, 1460)
        cnt = (ctypes.c_uint64 * 4)(7, 7, 7, 7)
        assert N.lib().nfec_codec_tail_batches(c._h, cnt, 4) == 2
        assert list(cnt) == [0, 0, 0, 0]  # entries past the two counters read 0
        assert c.tail_batches() == {"encode": 0, "decode": 0}
