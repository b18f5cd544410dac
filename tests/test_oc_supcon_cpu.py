"""OC-Softmax and SupCon criteria (radhip.train.OCSoftmax / SupConLoss, src/loss.py:5-152) on the CPU: values and
gradients against tests/golden/oc_supcon.npz (written by the reference's own classes in float64,
tests/golden/make_golden_losses.py), the centre's draw, the config quirks of src/main.py:181-184,278-296,1020, and
how radhip.train.Trainer and main.py carry the learnable centre (optimizer group 3, outside the clip, no gradient
for the classifier, checkpoint sibling files, train-state round trip)."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from radhip.train import (FocalLoss, OCSoftmax, SupConLoss, Trainer, build_criterion, build_supcon, criterion_loss,
                          feats_loss)

SETS = ("mixed", "bonafide", "singleton")
OC_CFG = {"loss": "OCSoftmax", "model_config": {"architecture": "DualStreamSEMamba", "emb_size": 144},
          "training_config": {}}


def _close(got, want, rtol):
    want = np.asarray(want, dtype=np.float64)
    np.testing.assert_allclose(np.asarray(got, dtype=np.float64), want, rtol=rtol,
                               atol=rtol * float(np.abs(want).max()))


@pytest.mark.parametrize("dtype,rtol", [(torch.float64, 1e-12), (torch.float32, 1e-5)], ids=["fp64", "fp32"])
@pytest.mark.parametrize("B", [2, 3, 8])
def test_modules_match_reference_fixture(golden, B, dtype, rtol):
    g = golden("oc_supcon.npz")
    oc = OCSoftmax(144)
    with torch.no_grad():
        oc.center.copy_(torch.from_numpy(g["center_seed1234"]))
    oc = oc.to(dtype)
    sc = SupConLoss(0.07)
    f0 = torch.from_numpy(g[f"f{B}"]).to(dtype)
    for name in SETS:
        y = torch.from_numpy(g[f"y{B}_{name}"])
        f = f0.clone().requires_grad_(True)
        oc.center.grad = None
        v = oc(f, y)
        v.backward()
        _close(v.item(), g[f"oc{B}_{name}"], rtol)
        _close(f.grad, g[f"oc_df{B}_{name}"], rtol)
        _close(oc.center.grad, g[f"oc_dc{B}_{name}"], rtol)
        f = f0.clone().requires_grad_(True)
        v = sc(F.normalize(f, dim=1), y)
        v.backward()
        _close(v.item(), g[f"sc{B}_{name}"], rtol)
        _close(f.grad, g[f"sc_df{B}_{name}"], rtol)
    # the mixup total, through the trainer's own combination (module path) with accumulation 1
    ya, yb = torch.from_numpy(g[f"mix{B}_ya"]), torch.from_numpy(g[f"mix{B}_yb"])
    lam = torch.tensor([float(g[f"mix{B}_lam"])], dtype=dtype)
    f = f0.clone().requires_grad_(True)
    oc.center.grad = None
    tot = feats_loss(oc, sc, float(g[f"mix{B}_lambda"]), 1, f, ya, yb, lam, B)
    tot.backward()
    _close(tot.item(), g[f"mix{B}_total"], rtol)
    _close(f.grad, g[f"mix{B}_df"], rtol)
    _close(oc.center.grad, g[f"mix{B}_dc"], rtol)
    one = lambda y: criterion_loss(oc, sc, float(g[f"mix{B}_lambda"]), None, f0, y)
    _close((lam[0] * one(ya) + (1 - lam[0]) * one(yb)).item(), g[f"mix{B}_total"], rtol)


def test_centre_draw_is_the_references(golden):
    """randn(1, D) then kaiming_uniform_(center, 0.25) on the global generator, at build_criterion's call."""
    torch.manual_seed(1234)
    c = build_criterion(OC_CFG, "cpu")
    assert isinstance(c, OCSoftmax) and c.center.shape == (1, 144) and c.center.dtype == torch.float32
    assert np.array_equal(c.center.detach().numpy().astype(np.float64), golden("oc_supcon.npz")["center_seed1234"])
    after = torch.rand(1)
    torch.manual_seed(1234)
    x = torch.randn(1, 144)
    torch.nn.init.kaiming_uniform_(x, 0.25)
    assert torch.equal(torch.rand(1), after)          # the generator stands where the reference's would


def test_supcon_singleton_row_contributes_zero():
    torch.manual_seed(0)
    z = F.normalize(torch.randn(3, 16, dtype=torch.float64), dim=1)
    y = torch.tensor([0, 1, 1])
    logits = z @ z.t() / 0.07
    rows = []
    for i in (1, 2):                                   # rows with one positive each (the other of {1, 2})
        j = 3 - i
        others = [k for k in range(3) if k != i]
        m = logits[i].max()
        rows.append(-((logits[i, j] - m) - torch.log(torch.exp(logits[i, others] - m).sum() + 1e-8)))
    want = (rows[0] + rows[1]) / 3                     # row 0 (no positive) adds 0 to the mean over 3 rows
    got = SupConLoss(0.07)(z, y)
    assert float(got) == pytest.approx(float(want), rel=1e-12)
    zz = z.clone().requires_grad_(True)
    SupConLoss(0.07)(zz, torch.tensor([0, 1, 2])).backward()        # no positives at all: 0, zero gradient
    assert float(SupConLoss(0.07)(z, torch.tensor([0, 1, 2]))) == 0.0 and not zz.grad.any()


def test_large_alpha_stays_finite():
    torch.manual_seed(0)
    oc = OCSoftmax(8, alpha=200.0)
    x = torch.randn(6, 8, requires_grad=True)
    loss = oc(x, torch.tensor([1, 0, 1, 0, 1, 0]))
    loss.backward()
    assert torch.isfinite(loss) and torch.isfinite(x.grad).all() and torch.isfinite(oc.center.grad).all()
    assert float(loss) > 20.0                          # past softplus's linear threshold: the overflow-safe branch


def test_build_criterion_selects_oc_softmax():
    cfg = copy.deepcopy(OC_CFG)
    cfg["training_config"] = {"ocsoftmax_r_real": 0.8, "ocsoftmax_r_fake": 0.3, "ocsoftmax_alpha": 10.0,
                              "use_focal_loss": True}
    c = build_criterion(cfg, "cpu")                    # 'OCSoftmax' wins over use_focal_loss (src/main.py:278,297)
    assert isinstance(c, OCSoftmax) and (c.r_real, c.r_fake, c.alpha) == (0.8, 0.3, 10.0)
    d = build_criterion(OC_CFG, "cpu")
    assert (d.r_real, d.r_fake, d.alpha, d.feat_dim) == (0.9, 0.5, 20.0, 144)
    cfg["model_config"] = {"architecture": "DualStreamSEMamba", "emb_size": 96}
    assert build_criterion(cfg, "cpu").center.shape == (1, 96)
    cfg["model_config"] = {"architecture": "AASIST"}
    assert build_criterion(cfg, "cpu").center.shape == (1, 160)
    assert isinstance(build_criterion({"loss": "Focal", "training_config": {}}, "cpu"), FocalLoss)


def test_supcon_config_quirks():
    """use_supcon: top level OR training_config; lambda_supcon: top level only, default 0.1."""
    assert build_supcon({"training_config": {}}) == (None, 0.0)
    s, lam = build_supcon({"use_supcon": True, "training_config": {}})
    assert isinstance(s, SupConLoss) and (s.temperature, s.base_temperature, lam) == (0.07, 0.07, 0.1)
    s, lam = build_supcon({"training_config": {"use_supcon": True, "lambda_supcon": 0.5}})
    assert isinstance(s, SupConLoss) and lam == 0.1    # the training_config value is never read
    s, lam = build_supcon({"lambda_supcon": 0.25, "training_config": {"use_supcon": True, "lambda_supcon": 0.5}})
    assert lam == 0.25


class Toy(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.body = torch.nn.Linear(6, 144)
        self.classifier = torch.nn.Linear(144, 2)

    def logit_only_parameters(self):
        return list(self.classifier.parameters())

    def forward(self, x, Freq_aug=False):
        h = torch.tanh(self.body(x))
        return h, self.classifier(h)


CFG = {"loss": "OCSoftmax", "use_supcon": True, "freq_aug": "False",
       "model_config": {"architecture": "DualStreamSEMamba", "emb_size": 144},
       "optim_config": {"base_lr": 5e-3, "wavlm_lr": 1e-4, "weight_decay": 1e-2, "scheduler": "cosine",
                        "scheduler_config": {"eta_min": 1e-6}},
       "training_config": {"use_mixup": False, "accumulation_steps": 1, "use_ema": True, "use_fgm": False,
                           "warmup_steps": 1, "freeze_bn": True}}


def _trainer(seed=3):
    torch.manual_seed(seed)
    m = Toy()
    return m, Trainer(m, CFG, "cpu", total_steps=8, amp_dtype=torch.float32)


def test_trainer_carries_the_centre():
    m, tr = _trainer()
    centre = tr.criterion.center
    g3 = tr.opt.param_groups[2]
    assert len(g3["params"]) == 1 and g3["params"][0] is centre and g3["initial_lr"] == CFG["optim_config"]["base_lr"]
    assert any(p is centre for p in tr.params) and not any(p is centre for p in tr.model_params)
    assert tr.grads.clipped.numel() == sum(p.numel() for p in m.body.parameters())
    assert tr.ema is not None and all("center" not in n for n in tr.ema.names)
    # the clip: the centre's gradient neither enters the norm nor is scaled
    for p in m.body.parameters():
        p.grad.fill_(1e-3)
    centre.grad.fill_(1e3)
    before = [p.grad.clone() for p in m.body.parameters()]
    tr.grads.clip_norm_(3.0)
    assert all(torch.equal(a, p.grad) for a, p in zip(before, m.body.parameters())) and float(centre.grad[0, 0]) == 1e3
    tr.grads.zero()
    # one step: centre and body move, the classifier (no gradient under OC-Softmax) does not, despite weight decay
    w0 = [p.detach().clone() for p in m.classifier.parameters()]
    c0, b0 = centre.detach().clone(), m.body.weight.detach().clone()
    x = torch.randn(4, 6)
    loss = tr.micro_step(x, torch.tensor([1, 0, 0, 1]), last_in_epoch=True)
    assert torch.isfinite(loss)
    assert all(p.grad is None for p in m.classifier.parameters())
    assert all(torch.equal(a, p.detach()) for a, p in zip(w0, m.classifier.parameters()))
    assert not torch.equal(c0, centre.detach()) and not torch.equal(b0, m.body.weight.detach())
    # the loss is the module combination of both criteria
    tr2m, tr2 = _trainer()
    f, out = tr2m(x)
    want = criterion_loss(tr2.criterion, tr2.supcon, 0.1, out, f, torch.tensor([1, 0, 0, 1]))
    assert float(loss) == pytest.approx(float(want), rel=1e-6)


def test_train_state_round_trips_the_centre():
    m, tr = _trainer()
    tr.micro_step(torch.randn(4, 6), torch.tensor([1, 0, 0, 1]), last_in_epoch=True)
    st = copy.deepcopy(tr.state_dict())
    assert torch.equal(st["criterion"]["center"], tr.criterion.center.detach())
    m2, tr2 = _trainer(seed=9)                           # another draw of the centre
    assert not torch.equal(tr2.criterion.center.detach(), tr.criterion.center.detach())
    ptr = tr2.criterion.center.data_ptr()
    tr2.load_state_dict(st)
    assert torch.equal(tr2.criterion.center.detach(), tr.criterion.center.detach())
    assert tr2.criterion.center.data_ptr() == ptr        # in place: captured graphs keep reading this storage
    st["criterion"] = None
    with pytest.raises(ValueError):
        tr2.load_state_dict(st)


def test_criterion_sibling_files(tmp_path):
    import main as cli
    torch.manual_seed(1)
    crit = build_criterion(OC_CFG, "cpu")
    model = Toy()
    path = tmp_path / "epoch_3_1.250.pth"
    cli.save_weights(model.state_dict(), path, crit)
    sib = tmp_path / "epoch_3_1.250.criterion.pt"
    assert cli.criterion_sibling(path) == sib and sib.exists()
    assert set(torch.load(path, weights_only=True)) == set(model.state_dict())      # the .pth stays model-only
    fresh = build_criterion(OC_CFG, "cpu")
    assert not torch.equal(fresh.center, crit.center)
    lines = []
    assert cli.load_criterion(fresh, path, lines.append) and torch.equal(fresh.center, crit.center)
    # without the sibling: one loud line, the drawn centre stays
    other = tmp_path / "best.pth"
    torch.save(model.state_dict(), other)
    fresh2 = build_criterion(OC_CFG, "cpu")
    keep = fresh2.center.detach().clone()
    lines.clear()
    assert not cli.load_criterion(fresh2, other, lines.append)
    assert len(lines) == 1 and "FRESHLY DRAWN" in lines[0] and torch.equal(fresh2.center.detach(), keep)
    # a criterion without parameters writes and reads nothing, says nothing
    cli.save_weights(model.state_dict(), tmp_path / "swa.pth", FocalLoss())
    assert not (tmp_path / "swa.criterion.pt").exists()
    lines.clear()
    assert not cli.load_criterion(FocalLoss(), other, lines.append) and not lines
    cli.remove_weights(path)
    assert not path.exists() and not sib.exists()
