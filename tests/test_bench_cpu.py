"""bench.py's output dump (--dump-outputs) and its option surface, on the host: what a dump holds, that large arrays become the same
seeded sample in every run, and that the whole dump stays under the size limit."""
import os

import numpy as np
import pytest
import torch


def test_named_tensors_flattens_step_results():
    import bench
    res = {"loss": torch.tensor(2.0), "terms": [torch.zeros(2), torch.ones(3)], "val/psnr": torch.ones(1), "step": 7, "lr": 1e-3}
    got = bench.named_tensors(res, "out")
    assert sorted(got) == ["out_loss", "out_terms_0", "out_terms_1", "out_val_psnr"]
    assert torch.equal(got["out_terms_1"], torch.ones(3))
    assert list(bench.named_tensors(torch.zeros(1), "loss")) == ["loss"]


def test_dump_outputs_dtypes_and_seeded_sample(tmp_path):
    import bench
    n = bench.SAMPLE_ELEMS * 3 + 5
    big = torch.randn(n, generator=torch.Generator().manual_seed(0))
    arrays = {"loss": torch.tensor(1.25, dtype=torch.float64), "small": torch.arange(6, dtype=torch.bfloat16).reshape(2, 3), "big": big}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["big.npy", "big_index.npy", "loss.npy", "small.npy"]
    loss, small = np.load(tmp_path / "a" / "loss.npy"), np.load(tmp_path / "a" / "small.npy")
    assert loss.dtype == np.float64 and loss == 1.25
    assert small.dtype == np.float32 and small.shape == (2, 3) and (small == np.arange(6).reshape(2, 3)).all()
    a, idx = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "a" / "big_index.npy")
    assert a.dtype == np.float32 and 0 < a.size <= bench.SAMPLE_ELEMS and idx.shape == a.shape
    assert (np.diff(idx) >= 0).all() and idx.max() < n
    assert (a == big.numpy()[idx.astype(np.int64)]).all()
    for f in files:                                     # the same sample in every run
        assert (np.load(tmp_path / "a" / f) == np.load(tmp_path / "b" / f)).all()
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in files)
    assert total <= bench.DUMP_LIMIT_BYTES


def test_dump_outputs_stays_under_the_limit_with_many_arrays(tmp_path):
    import bench
    arrays = {f"x{i}": torch.zeros(bench.SAMPLE_ELEMS + 1) for i in range(8)}
    bench.dump_outputs(str(tmp_path), arrays)
    total = sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path))
    assert len(os.listdir(tmp_path)) == 16 and total <= bench.DUMP_LIMIT_BYTES


@pytest.mark.parametrize("argv", [["--gpus", "1", "--steps", "3", "--warmup", "1", "--full", "--dump-outputs", "d"],
                                  ["--gpus", "1", "--steps", "3", "--warmup", "1"]])
def test_bench_options(argv, monkeypatch):
    """The plain line and --full / --dump-outputs parse; the parser is main()'s own (stopped before anything touches a device)."""
    import bench

    class Stop(Exception):
        pass

    def stop(*a, **k):
        raise Stop()

    monkeypatch.setattr(bench._lib, "require_gpu", stop)
    monkeypatch.setattr("sys.argv", ["bench.py"] + argv)
    with pytest.raises(Stop):
        bench.main()
