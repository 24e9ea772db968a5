"""-m "not gpu": bench.py's options and its output dump, on host tensors (no device needed)."""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _outs(B, N, samples, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, N, 100, generator=g)
    pcm = torch.randint(-32768, 32768, (B, samples), generator=g, dtype=torch.int16)
    pcm_len = torch.full((B,), samples, dtype=torch.int32)
    return x, pcm, pcm_len, {}


def test_dump_outputs_writes_the_returned_arrays_exactly(tmp_path):
    import bench
    o = _outs(3, 40, 512, 1)
    names = bench.dump_outputs(str(tmp_path), [o])
    assert names == ["mel", "pcm", "pcm_len"] and sorted(os.listdir(tmp_path)) == ["mel.npy", "pcm.npy", "pcm_len.npy"]
    mel, pcm, n = (np.load(tmp_path / f"{k}.npy") for k in names)
    assert mel.dtype == np.float32 and np.array_equal(mel, o[0].numpy())
    assert pcm.dtype == np.float32 and np.array_equal(pcm, o[1].numpy().astype(np.float32))          # int16 -> float32 is exact
    assert n.dtype == np.float64 and n.tolist() == [512.0] * 3


def test_dump_outputs_over_budget_writes_a_fixed_seeded_sample(tmp_path):
    """Several batches (mixed256) get `_b<i>` names; over the budget every batch keeps the same share of its items, the same
    items for all of its arrays, chosen by a fixed seed, and the item indices are written beside them."""
    import bench
    outs = [_outs(16, 400, 65536, 2), _outs(8, 500, 65536, 3)]
    total = sum(t.numel() * 4 * (2 if t.dtype == torch.int32 else 1) for o in outs for t in o[:3])
    budget = total // 2 + 2 ** 20
    d1, d2 = tmp_path / "a", tmp_path / "b"
    names = bench.dump_outputs(str(d1), outs, budget=budget)
    assert bench.dump_outputs(str(d2), outs, budget=budget) == names
    assert set(names) == {f"{k}_b{i}" for k in ("mel", "pcm", "pcm_len", "items") for i in (0, 1)}
    assert sum(os.path.getsize(d1 / f) for f in os.listdir(d1)) <= budget
    for i, o in enumerate(outs):
        items = np.load(d1 / f"items_b{i}.npy")
        assert items.dtype == np.float64 and 1 <= len(items) < o[0].shape[0] and np.all(np.diff(items) > 0)
        idx = items.astype(np.int64)
        assert np.array_equal(np.load(d1 / f"mel_b{i}.npy"), o[0].numpy()[idx])
        assert np.array_equal(np.load(d1 / f"pcm_b{i}.npy"), o[1].numpy()[idx].astype(np.float32))
        for n in names:                                                     # the same sample from run to run
            assert np.array_equal(np.load(d1 / f"{n}.npy"), np.load(d2 / f"{n}.npy"))


def test_bench_options():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout and "--steps" in r.stdout
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode != 0 and "--steps must be >= 1" in r.stderr
