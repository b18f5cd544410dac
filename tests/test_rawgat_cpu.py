"""RawGAT-ST plugin (models/RawNetGatSpoofST.py) on the CPU: conf, state_dict, the float64 module path against the
reference fixture (tests/golden/legacy_RawNetGatSpoofST.npz from make_golden_rawgat.py), optimizer and scheduler, and
GraphPool's floor of two nodes. The GPU side (fused graph attention, HIP front end, CLI) is in
tests/test_rawgat_gpu.py."""
import json
from importlib import import_module

import numpy as np
import pytest
import torch

from seeded import seeded_array, seeded_fill_

ARCH, CONF = "RawNetGatSpoofST", "RawGATST_baseline.conf"


def test_conf_parses_and_matches_the_fixture(golden):
    import main  # noqa: F401
    from radhip.build import load_config
    g = golden(f"legacy_{ARCH}.npz")
    cfg = load_config(CONF)
    assert cfg["model_config"] == json.loads(str(g["model_config"]))
    assert cfg["model_config"]["architecture"] == ARCH
    assert (cfg["batch_size"], cfg["num_epochs"], cfg["loss"], cfg["track"]) == (24, 100, "CCE", "LA")
    assert "model_path" not in cfg and "scheduler_config" not in cfg["optim_config"] and "training_config" not in cfg


def test_plugin_state_dict_matches_reference(golden):
    import main  # noqa: F401
    from radhip.build import get_model, legacy_plugin, load_config
    g = golden(f"legacy_{ARCH}.npz")
    mc = load_config(CONF)["model_config"]
    assert legacy_plugin(import_module(f"models.{ARCH}").Model)
    before = json.dumps(mc)
    m = get_model(mc, "cpu")
    assert json.dumps(mc) == before
    sd = m.state_dict()
    assert list(sd.keys()) == [str(k) for k in g["keys"]]
    assert [json.dumps(list(v.shape)) for v in sd.values()] == [str(s) for s in g["shapes"]]
    assert sum(p.numel() for p in m.parameters()) == int(g["n_params"])


@pytest.mark.parametrize("mode", ["eval", "train"])
def test_float64_module_path_matches_fixture(golden, mode):
    """The product model in float64 on the CPU, seeded like the fixture: the same arithmetic in the same precision,
    so only summation order differs. Outputs and running statistics at rtol 1e-9 (largest deviation observed:
    2.4e-12 and 3.4e-11), gradients at rtol 1e-7. A bare relative bound cannot hold for the gradient elements that
    cancellation leaves near zero (GAT_layer_S.att_weight has one at 1e-13 of its tensor's maximum), so, on summation
    order alone, each gradient element also gets an absolute allowance of 3e-11 of its tensor's largest magnitude:
    10 x the largest deviation observed, 2.32e-12 (train mode; eval 9.4e-13). A bias that feeds a batch-statistics
    BatchNorm has an exactly-zero true gradient; both sides hold a rounding residue there (reference at most 9.5e-15
    of the mode's largest gradient, this model 1.2e-14), bounded by 2e-13 of the mode's largest gradient, 10 x that.
    The fixture's top-k gaps are >= 1e-3, so both sides keep the same nodes."""
    import main  # noqa: F401
    from radhip.build import get_model, load_config
    g = golden(f"legacy_{ARCH}.npz")
    assert min(g["eval:topk_gap"].min(), g["train:topk_gap"].min()) >= 1e-3
    m = get_model(load_config(CONF)["model_config"], "cpu")
    seeded_fill_(m, seed=int(g["seed"]))
    m = m.double()
    assert m.conv_time.band_pass.dtype == torch.float64
    if mode == "train":
        for d in m.modules():
            if isinstance(d, torch.nn.Dropout):
                d.p = 0.0
        m.train()
    else:
        m.eval()
    x = torch.from_numpy(seeded_array(f"{ARCH}.x", (2, 64600), scale=0.1).astype(np.float32)).double()
    hid, out = m(x, Freq_aug=False)
    assert hid.shape == (2, 7) and out.shape == (2, 2)
    for got, key in ((hid, "hidden"), (out, "out")):
        ref = g[f"{mode}:{key}"]
        np.testing.assert_allclose(got.detach().numpy(), ref, rtol=1e-9, atol=0, err_msg=key)
    rh, ro = torch.from_numpy(g[f"{mode}:rh"]).double(), torch.from_numpy(g[f"{mode}:ro"]).double()
    ((hid * rh).sum() + (out * ro).sum()).backward()
    gmax = max(np.abs(g[k]).max() for k in g if k.startswith(f"{mode}:grad:"))
    n = 0
    for k, p in m.named_parameters():
        if f"{mode}:grad:{k}" in g:
            ref = g[f"{mode}:grad:{k}"]
            if np.abs(ref).max() < 1e-12 * gmax:            # exactly-zero true gradient
                assert np.abs(p.grad.numpy()).max() < 2e-13 * gmax, (k, np.abs(p.grad.numpy()).max() / gmax)
            else:
                np.testing.assert_allclose(p.grad.numpy(), ref, rtol=1e-7, atol=3e-11 * np.abs(ref).max(), err_msg=k)
            n += 1
        elif f"{mode}:gradsum:{k}" in g:
            s = g[f"{mode}:gradsum:{k}"]
            got = p.grad.numpy()
            np.testing.assert_allclose((got * got).sum(), s[1], rtol=1e-7, err_msg=k)
            assert abs(got.sum() - s[0]) <= 3e-11 * np.sqrt(s[1] * got.size), k      # the plain sum cancels
            head = g[f"{mode}:gradhead:{k}"]
            np.testing.assert_allclose(got.reshape(-1)[:64], head, rtol=1e-7, atol=3e-11 * np.abs(got).max(), err_msg=k)
            n += 1
        else:       # the dead bn1 affine weights: no gradient in the reference either
            assert p.grad is None or not p.grad.any(), k
    assert n >= 90, n
    if mode == "train":
        sd = m.state_dict()
        stats = [k for k in g if k.startswith("stat:")]
        assert len(stats) >= 50
        for k in stats:
            np.testing.assert_allclose(sd[k[5:]].numpy(), g[k], rtol=1e-9, atol=0, err_msg=k)


def test_conf_optimizer_and_schedule():
    import main  # noqa: F401
    from radhip.build import get_model, load_config
    from radhip.train import Trainer
    cfg = load_config(CONF)
    m = get_model(cfg["model_config"], "cpu")
    tr = Trainer(m, cfg, "cpu", total_steps=100, amp_dtype=torch.float32)
    assert tr.sched._schedulers[1].eta_min == cfg["optim_config"]["lr_min"]
    assert tr.accum == 1 and tr.fgm is None and tr.ema is None and not tr.use_mixup
    assert len(tr.opt.param_groups[0]["params"]) == 0
    assert sum(p.numel() for p in tr.opt.param_groups[1]["params"]) == sum(p.numel() for p in m.parameters())
    assert tr.opt.param_groups[1]["lr"] == pytest.approx(0.1 * cfg["optim_config"]["base_lr"])


def test_graph_pool_keeps_two_nodes_in_descending_order():
    from models.RawNetGatSpoofST import GraphPool
    pool = GraphPool(0.3, 4, 0.0)             # int(3 * 0.3) = 0 and int(5 * 0.3) = 1: both below the floor of 2
    with torch.no_grad():
        pool.proj.weight.copy_(torch.tensor([[1.0, 0.0, 0.0, 0.0]]))
        pool.proj.bias.zero_()
    for n in (3, 5):
        h = torch.zeros(2, n, 4)
        h[0, :, 0] = torch.arange(n, dtype=torch.float32)               # scores ascending: the last node is first
        h[1, :, 0] = -torch.arange(n, dtype=torch.float32)
        h[..., 1] = 1.0
        out = pool(h)
        assert out.shape == (2, 2, 4)
        s = torch.sigmoid(h[..., 0])
        assert torch.allclose(out[0, :, 1], torch.stack([s[0, n - 1], s[0, n - 2]]))     # scaled by its score
        assert torch.allclose(out[1, :, 1], torch.stack([s[1, 0], s[1, 1]]))
        assert (out[:, 0, 1] > out[:, 1, 1]).all()
    assert GraphPool(0.64, 4, 0.0)(torch.randn(1, 23, 4)).shape[1] == 14
    assert GraphPool(0.81, 4, 0.0)(torch.randn(1, 29, 4)).shape[1] == 23
