"""bench.py --dump-outputs writes float32 / float64 .npy files and samples the same gradient positions in every run (the helper
runs on CPU tensors; the GPU line is tests/test_gpu_bench_contract.py), and a plain run offers --full and --dump-outputs."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _module_with_grads():
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Linear(96, 64), torch.nn.Linear(64, 3), torch.nn.Linear(3, 3))
    m[2].weight.requires_grad_(False)                     # a parameter without a gradient is left out
    m(torch.randn(5, 96)).square().sum().backward()
    return m


def test_dump_outputs_dtypes_names_and_a_fixed_sample(tmp_path):
    bench = _bench()
    m = _module_with_grads()
    arrays = {"loss": torch.tensor(1.5, dtype=torch.float64), "lm_loss": torch.tensor([0.25, 0.5], dtype=torch.bfloat16),
              "ranks": torch.tensor([[3, 1, 2]])}
    bench.dump_outputs(str(tmp_path / "a"), arrays, m)
    bench.dump_outputs(str(tmp_path / "b"), arrays, m)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["grad_norm.npy", "grad_sample.npy", "lm_loss.npy", "loss.npy", "ranks.npy"]
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype in (np.float32, np.float64) and a.dtype == b.dtype, (n, a.dtype)
        np.testing.assert_array_equal(a, b)
    assert np.load(tmp_path / "a" / "loss.npy").dtype == np.float64
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "ranks.npy"), [[3, 1, 2]])
    grads = [p.grad.reshape(-1) for p in m.parameters() if p.grad is not None]
    norms = np.load(tmp_path / "a" / "grad_norm.npy")
    np.testing.assert_allclose(norms, [float(g.double().norm()) for g in grads], rtol=1e-12)
    sample = np.load(tmp_path / "a" / "grad_sample.npy")
    n = bench.DUMP_GRAD_SAMPLE
    assert sample.size == sum(min(g.numel(), n) for g in grads)
    g0 = grads[0]                                          # 6144 elements > the sample: seeded positions, all of them real values
    assert g0.numel() > n and np.isin(sample[:n], g0.numpy()).all()
    np.testing.assert_array_equal(sample[n:n + 64], grads[1].numpy())   # smaller tensors are kept whole


def test_plain_run_offers_full_and_dump_outputs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout
