"""bench.py --dump-outputs on the CPU: the choice of sampled blocks is fixed by the batch shape,
the arrays are float copies of the batch, and the files stay within the size budget."""
import numpy as np
import torch

import bench


def _batch(nb, segs, vec, seed):
    g = torch.Generator().manual_seed(seed)
    blocks = torch.randint(0, 256, (nb, segs, vec), dtype=torch.uint8, generator=g)
    status = torch.randint(0, 17, (nb,), dtype=torch.int32, generator=g)
    return blocks, status


def _load(path):
    return {p.name[:-4]: np.load(p) for p in path.iterdir()}


def test_dump_is_a_float_copy_of_a_fixed_sample(tmp_path):
    blocks, status = _batch(300, 6, 37, 1)
    bench.dump_outputs(str(tmp_path / "a"), blocks, status, 0)
    bench.dump_outputs(str(tmp_path / "b"), blocks.clone(), status.clone(), 0)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == ["block_sums", "blocks_sample", "blocks_sample_index", "status"]
    for name in a:
        assert a[name].dtype in (np.float32, np.float64) and np.array_equal(a[name], b[name]), name
    # a batch this small fits whole
    assert np.array_equal(a["blocks_sample_index"], np.arange(300))
    assert np.array_equal(a["blocks_sample"], blocks.numpy().astype(np.float32))
    assert np.array_equal(a["status"], status.numpy().astype(np.float32))
    assert np.array_equal(a["block_sums"], blocks.numpy().reshape(300, -1).sum(axis=1, dtype=np.int64))


def test_dump_samples_a_large_batch_within_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET", 200_000)
    blocks, status = _batch(1000, 4, 100, 2)  # 1,600 B per block as float32: ~116 blocks fit
    bench.dump_outputs(str(tmp_path), blocks, status, 3)
    assert sorted(p.name for p in tmp_path.iterdir()) == [
        "block_sums.rank3.npy", "blocks_sample.rank3.npy", "blocks_sample_index.rank3.npy", "status.rank3.npy"]
    assert sum(p.stat().st_size for p in tmp_path.iterdir()) <= 200_000
    d = {k.split(".")[0]: v for k, v in _load(tmp_path).items()}
    idx = d["blocks_sample_index"].astype(np.int64)
    assert 100 <= len(idx) < 1000 and (np.diff(idx) > 0).all() and idx.max() < 1000
    assert idx.max() - idx.min() > 500  # spread over the batch, not its head
    assert np.array_equal(d["blocks_sample"], blocks.numpy()[idx].astype(np.float32))
    assert d["status"].shape == d["block_sums"].shape == (1000,)
    # a different batch of the same shape: the same blocks are chosen
    other, st2 = _batch(1000, 4, 100, 5)
    bench.dump_outputs(str(tmp_path / "o"), other, st2, 0)
    assert np.array_equal(np.load(tmp_path / "o" / "blocks_sample_index.npy"), d["blocks_sample_index"])
