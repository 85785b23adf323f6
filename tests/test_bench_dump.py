"""CPU: bench.py's command line (a plain run times the steps only, --full adds the checks) and the --dump-outputs format: exact 16-bit
digits of the u64 words, whole when small, a fixed sample within the size limit when large."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

DIGITS = np.array([1 << 48, 1 << 32, 1 << 16, 1], dtype=np.uint64)


def parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + list(argv))
    return bench.parse()


def test_plain_run_skips_the_extras_full_keeps_them(monkeypatch):
    a = parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
    assert a.no_cpu and a.no_verify and a.no_power
    a = parse(monkeypatch, "--full", "--steps", "7")
    assert a.full and not (a.no_cpu or a.no_verify or a.no_power)
    a = parse(monkeypatch, "--full", "--no-cpu", "--dump-outputs", "out")
    assert a.no_cpu and not a.no_verify and a.dump_outputs == "out"
    with pytest.raises(SystemExit):
        parse(monkeypatch, "--steps", "0")


def test_dump_small_output_whole_and_exact(tmp_path):
    q = bench.QI60[:3]
    rng = np.random.default_rng(3)
    w = np.stack([rng.integers(0, q_, size=(2, 64), dtype=np.uint64) for q_ in q], axis=1)      # (2, 3, 64)
    w[0, 0, :4] = [0, 1, (1 << 61) - 1, q[0] - 1]
    bench.dump_outputs(str(tmp_path), {"out": torch.from_numpy(w.view(np.int64))})
    x = np.load(str(tmp_path / "out.npy"))
    assert x.dtype == np.float32 and x.shape == (2, 3, 64, 4)
    assert np.array_equal(x.astype(np.uint64) @ DIGITS, w)


def test_dump_large_outputs_sampled_within_the_limit_and_fixed(tmp_path):
    n = 3 << 20
    t = [torch.arange(n, dtype=torch.int64) * 0x10001 + k for k in range(2)]     # word value tells its flat index
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"x": t[0], "y": t[1]})
    total = 0
    for name, k in (("x", 0), ("y", 1)):
        a, b = (np.load(str(tmp_path / d / (name + ".npy"))) for d in ("a", "b"))
        assert np.array_equal(a, b)                                              # the same sample on every run
        total += a.nbytes
        w = a.astype(np.uint64) @ DIGITS
        idx = (w - np.uint64(k)) // np.uint64(0x10001)
        assert np.all(np.diff(idx.astype(np.int64)) > 0) and idx[-1] < n        # sorted, distinct indices into the output
        assert len(idx) == bench.DUMP_MAX_WORDS // 2 and idx[0] < n // len(idx)                 # spread over the whole output
    assert total <= 64 * 10 ** 6
