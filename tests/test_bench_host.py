"""bench.py's output dump (--dump-outputs): names, dtypes, the size cap and the fixed sample of large gradients."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _outputs(big):
    g = torch.Generator().manual_seed(0)
    parts = {n: torch.randn(1, generator=g, dtype=torch.float64) for n in ("x", "z", "v")}
    grads = {"v": torch.randn(1, 50, 8, generator=g), "u": torch.randn(1, big, generator=g)}
    return parts, grads, torch.zeros(1, dtype=torch.float64)


def test_dump_writes_every_returned_array(tmp_path):
    parts, grads, nnf = _outputs(1000)
    bench.dump_outputs(str(tmp_path), parts, grads, nnf)
    names = sorted(os.listdir(tmp_path))
    assert names == sorted([f"part_{n}.npy" for n in parts] + [f"grad_{n}.npy" for n in grads] + ["n_nonfinite.npy"])
    for n, t in parts.items():
        a = np.load(tmp_path / f"part_{n}.npy")
        assert a.dtype == np.float64 and np.array_equal(a, t.numpy())
    for n, t in grads.items():
        a = np.load(tmp_path / f"grad_{n}.npy")
        assert a.dtype == np.float32 and np.array_equal(a, t.reshape(-1).numpy())


def test_large_gradients_are_a_fixed_sample_under_the_cap(tmp_path):
    big = bench.DUMP_MAX_ENTRIES * 3 + 7
    parts, grads, nnf = _outputs(big)
    bench.dump_outputs(str(tmp_path / "a"), parts, grads, nnf)
    bench.dump_outputs(str(tmp_path / "b"), parts, grads, nnf)
    a = np.load(tmp_path / "a" / "grad_u.npy")
    assert a.shape == (bench.DUMP_MAX_ENTRIES,) and a.dtype == np.float32
    assert np.array_equal(a, np.load(tmp_path / "b" / "grad_u.npy"))
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).integers(0, big, bench.DUMP_MAX_ENTRIES))
    assert np.array_equal(a, grads["u"].reshape(-1).numpy()[idx])
    # twelve gradients at the cap stay within the 64 MB a dump may take
    assert 12 * bench.DUMP_MAX_ENTRIES * 4 <= 64 * 2 ** 20
