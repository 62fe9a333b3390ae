"""bench.py --dump-outputs helper: what lands on disk (no GPU needed).

Small tensors are written whole; a tensor over its share of the budget is
reduced to a fixed, seeded row sample, so two runs (two builds) dump the
same rows and can be compared output for output."""

import numpy as np
import torch

import bench


def test_dump_small_tensor_written_whole(tmp_path):
    t = torch.arange(2 * 5 * 3 * 8, dtype=torch.float32).reshape(2, 5, 3, 8).half()
    bench.dump_outputs(str(tmp_path), {"o": t}, rank=0, world=1)
    a = np.load(tmp_path / "o.npy")
    assert a.dtype == np.float32 and a.shape == (2, 5, 3, 8)
    np.testing.assert_array_equal(a, t.float().numpy())


def test_dump_large_tensor_sampled_within_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4096)
    rows, d = 1000, 16
    t = (torch.arange(rows, dtype=torch.float32)[:, None]
         + torch.arange(d, dtype=torch.float32) / 100).reshape(10, 100, d)
    bench.dump_outputs(str(tmp_path / "a"), {"o": t}, rank=0, world=1)
    bench.dump_outputs(str(tmp_path / "b"), {"o": t.clone()}, rank=0, world=1)
    a = np.load(tmp_path / "a" / "o.npy")
    b = np.load(tmp_path / "b" / "o.npy")
    assert a.dtype == np.float32
    assert a.shape == (4096 // (4 * d), d) and a.nbytes <= 4096
    np.testing.assert_array_equal(a, b)            # same rows every run
    picked = a[:, 0].astype(np.int64)              # column 0 is the row index
    assert np.all(np.diff(picked) > 0)             # distinct, ascending
    np.testing.assert_array_equal(a, t.reshape(rows, d).numpy()[picked])


def test_dump_per_rank_names_share_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4096)
    t = torch.randn(64, 4, 16, generator=torch.Generator().manual_seed(0))
    for r in range(2):
        bench.dump_outputs(str(tmp_path), {"o": t}, rank=r, world=2)
    files = sorted(p.name for p in tmp_path.iterdir())
    assert files == ["o_rank0.npy", "o_rank1.npy"]
    assert sum(np.load(tmp_path / f).nbytes for f in files) <= 4096
