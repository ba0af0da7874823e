"""CPU tests of bench.py's output dump (``--dump-outputs``) and of its command line: no kernels run."""

import numpy as np
import torch


def test_dump_outputs_dtypes_and_values(tmp_path):
    import bench

    logits = torch.linspace(-3, 3, 1000).to(torch.bfloat16)
    token = torch.tensor([[31999]], dtype=torch.int32)
    hist = torch.arange(8, dtype=torch.int64) + 2 ** 40
    shapes = bench.dump_outputs(tmp_path / "out", {"logits": logits, "token": token, "chunk_tokens": hist})
    assert shapes == {"logits": [1000], "token": [1, 1], "chunk_tokens": [8]}
    lg = np.load(tmp_path / "out" / "logits.npy")
    assert lg.dtype == np.float32 and np.array_equal(lg, logits.float().numpy())  # bf16 -> float32 is exact
    tk = np.load(tmp_path / "out" / "token.npy")
    assert tk.dtype == np.float64 and tk.item() == 31999
    ch = np.load(tmp_path / "out" / "chunk_tokens.npy")
    assert ch.dtype == np.float64 and np.array_equal(ch.astype(np.int64), hist.numpy())


def test_dump_outputs_stays_within_the_limit_with_a_fixed_sample(tmp_path):
    import bench

    big = torch.arange(5000, dtype=torch.float32)
    small = np.arange(10, dtype=np.float64)
    for d in ("a", "b"):
        shapes = bench.dump_outputs(tmp_path / d, {"big": big, "small": small}, limit=4096)
        assert shapes == {"big": [512], "small": [10]}  # 2048-byte share each: 512 float32 of the 5000
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert np.array_equal(a, b) and np.all(np.diff(a) > 0)  # the same ascending sample every time
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) <= 4096 + 2 * 128
    assert np.array_equal(np.load(tmp_path / "a" / "small.npy"), small)


def test_bench_command_line_has_full_and_dump_outputs(monkeypatch, capsys):
    import bench
    import pytest

    monkeypatch.setattr("sys.argv", ["bench.py", "--help"])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 0
    text = capsys.readouterr().out
    assert "--full" in text and "--dump-outputs DIR" in text and "--steps" in text and "--warmup" in text
