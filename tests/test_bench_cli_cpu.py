"""bench.py's command line and its output dump (host logic only; CPU)."""
import os
import sys
import types

import numpy as np
import torch

import bench


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_the_default(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "3")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 3, False, None)
    a = _parse(monkeypatch, "--full", "--dump-outputs", "d")
    assert a.full and a.dump_outputs == "d"


def _trainer(n_params, n_ema):
    g = torch.Generator().manual_seed(3)
    ema = types.SimpleNamespace(shadow=[torch.randn(n_ema, generator=g, dtype=torch.float64)])
    return types.SimpleNamespace(params=[torch.randn(5, 7, generator=g), torch.randn(n_params - 35, generator=g)],
                                 ema=ema, loss_sum=torch.tensor(6.0, dtype=torch.float64), n_seen=4)


def test_dump_outputs_whole_arrays(tmp_path):
    tr = _trainer(1000, 300)
    written = bench.dump_outputs(str(tmp_path), tr)
    assert written == {"params": 1000, "ema": 300, "loss": 1}
    p = np.load(tmp_path / "params.npy")
    assert p.dtype == np.float32
    np.testing.assert_array_equal(p, torch.cat([t.reshape(-1) for t in tr.params]).numpy())
    e = np.load(tmp_path / "ema.npy")
    assert e.dtype == np.float32
    np.testing.assert_array_equal(e, tr.ema.shadow[0].float().numpy())
    loss = np.load(tmp_path / "loss.npy")
    assert loss.dtype == np.float64 and loss.tolist() == [1.5]
    assert float(tr.loss_sum) == 6.0 and tr.n_seen == 4       # the trainer's running loss is read, not reset


def test_dump_outputs_samples_past_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 4096 + 2 * 4 * 100)      # 100 float32 elements per array
    tr = _trainer(1000, 60)
    a, b = tmp_path / "a", tmp_path / "b"
    assert bench.dump_outputs(str(a), tr) == {"params": 100, "ema": 60, "loss": 1}
    bench.dump_outputs(str(b), tr)
    pa, pb = np.load(a / "params.npy"), np.load(b / "params.npy")
    np.testing.assert_array_equal(pa, pb)                     # the same sample every time
    flat = torch.cat([t.reshape(-1) for t in tr.params]).numpy()
    idx = np.sort(np.random.default_rng(0).choice(1000, 100, replace=False))
    np.testing.assert_array_equal(pa, flat[idx])
    total = sum(os.path.getsize(a / f) for f in os.listdir(a))
    assert total <= bench.DUMP_MAX_BYTES
