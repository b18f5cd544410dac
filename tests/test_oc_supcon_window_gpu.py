"""OC-Softmax + SupCon through the accumulation window (radhip/window.py): the HIP-graph window with the fused
criterion launch (csrc/ocsupcon.hip) against the reference-order eager micro-steps with the module criteria
(Trainer.micro_step), on the 2-layer tiny model of tests/test_window_gpu.py: one window, K = 2, B = 2, FGM on, fp32,
"loss": "OCSoftmax" with use_supcon.

Compared: every stepped parameter (the centre included) after one optimizer step, as the relative L2 difference of
the two runs' parameter UPDATES. Bound, measured in the same run: the identical comparison with "loss": "Focal" (the
code path before OC-Softmax existed) gives the discrepancy the window has against the sequential order today; OC +
SupCon may show at most 4x that, plus an fp32 floor: a stored fp32 parameter is rounded by up to half an ulp, so two
runs whose updates differ at all can differ by 0.5 * eps32 * |p| in L2, taken relative to the update's norm
(parameters are O(1), one AdamW step moves them by about their learning rate). Both figures go to
profiles/ocsupcon_errors.json.

The tiny model is built ONCE for the module: every run starts
from the same saved values of its parameters and buffers, written back in place, with its own Trainer (own optimizer
state, own flat gradient buffer, the centre drawn from the same seed); the runs assert that they started equal.
What the module costs is MIOpen's first-use solver search for the fp32 convolutions at N = 2 and N = 4 utterances
(measured alone: 54 s; once the shapes are known the four runs take 1 s together); a process that has already run
fp32 passes at those sizes (tests/test_graph_gpu.py runs N = 4 earlier in the suite) does not search again.

The x3 scoring stream is ineligible on this tiny model (its reduced-width WavLM, as in the existing scoring tests), so
the scoring check runs the fp32 scoring pass; the cosine score itself does not depend on which stream produced the
features."""
import copy
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_oc_supcon_gpu import record
from test_window_gpu import _batches, _model

pytestmark = pytest.mark.gpu
DEV = "cuda"
K, B = 2, 2
EPS32 = float(np.finfo(np.float32).eps)


class World:
    """The shared tiny model, its config and the values every run starts from."""

    def __init__(self, golden):
        self.model, self.cfg = _model(golden, K)
        self.tensors = list(self.model.parameters()) + list(self.model.buffers())
        self.saved = [t.detach().clone() for t in self.tensors]
        self.trainable = [p.requires_grad for p in self.model.parameters()]

    def reset(self):
        with torch.no_grad():
            torch._foreach_copy_(self.tensors, self.saved)
        for p, r in zip(self.model.parameters(), self.trainable):   # FGM unfreezes feature_projection per trainer
            p.requires_grad_(r)
        self.model.zero_grad(set_to_none=True)   # no .grad left from the run before (the classifier's under OC-Softmax)

    def trainer(self, loss, supcon):
        from radhip.train import Trainer
        self.reset()
        cfg = copy.deepcopy(self.cfg)
        cfg["loss"] = loss
        cfg["use_supcon"] = supcon
        cfg["model_config"] = {"architecture": "DualStreamSEMamba", "emb_size": 144}
        assert cfg["training_config"]["use_fgm"]
        torch.manual_seed(77)                      # the centre's draw, the same in every run
        return Trainer(self.model, cfg, DEV, total_steps=10, amp_dtype=torch.float32)


def _flat(tr):
    return torch.cat([p.detach().reshape(-1) for p in tr.params]).clone()


def _sequential(world, loss, supcon):
    tr = world.trainer(loss, supcon)
    p0 = _flat(tr)
    xs, ys, lams, perms = _batches(K, B)
    for k in range(K):
        tr.micro_step(xs[k], torch.from_numpy(ys[k]), lams[k], perms[k])
    torch.cuda.synchronize()
    return tr, p0, _flat(tr), float(tr.loss_sum)


def _stage(w):
    xs, ys, lams, perms = _batches(K, B)
    for k in range(K):
        w.xslot(k).copy_(xs[k])
        w.add(k, ys[k], lams[k], perms[k])


def _window(world, loss, supcon):
    from radhip.window import WindowStep
    tr = world.trainer(loss, supcon)
    p0 = _flat(tr)
    w = WindowStep(tr, B, graphs=True)
    _stage(w)
    w.run()                                    # captures, replays once, steps the optimizer
    torch.cuda.synchronize()
    return tr, w, p0, _flat(tr), float(tr.loss_sum)


def _discrepancy(p0, seq, win):
    d_seq = seq - p0
    return float((win - seq).norm() / d_seq.norm()), 0.5 * EPS32 * float(seq.norm() / d_seq.norm())


@pytest.fixture(scope="module")
def world(golden):
    t0 = time.perf_counter()
    w = World(golden)
    torch.cuda.synchronize()
    print(f"[window oc+supcon setup] model: {time.perf_counter() - t0:.1f} s")
    return w


@pytest.fixture(scope="module")
def focal_pair(world):
    """(trainer of "loss": "Focal", trainer of "loss": "Focal" with use_supcon), both from the config, on the shared
    model. The launch tests run no model pass, so they need nothing of the model but these trainers; `runs` asks for
    this fixture too, so the pair is always built before the runs, whatever order the tests come in."""
    return world.trainer("Focal", False), world.trainer("Focal", True)


@pytest.fixture(scope="module")
def runs(world, focal_pair):
    out, t = {}, [time.perf_counter()]

    def lap(name):
        torch.cuda.synchronize()
        t.append(time.perf_counter())
        print(f"[window oc+supcon setup] {name}: {t[-1] - t[-2]:.1f} s")
    _, p0, seq, lseq = _sequential(world, "Focal", False)
    lap("focal sequential")
    trf, _, q0, win, lwin = _window(world, "Focal", False)
    lap("focal window")
    assert torch.equal(p0, q0)
    out["focal"] = dict(d=_discrepancy(p0, seq, win), lseq=lseq, lwin=lwin, tr=trf)
    trs, p0, seq, lseq = _sequential(world, "OCSoftmax", True)
    lap("oc+supcon sequential")
    tro, wo, q0, win, lwin = _window(world, "OCSoftmax", True)     # the last run: the model keeps its trained values
    lap("oc+supcon window")
    assert torch.equal(p0, q0)
    nc = tro.criterion.center.numel()
    head = list(world.model.classifier.parameters())
    head0 = [s for t_, s in zip(world.tensors, world.saved) if any(t_ is h for h in head)]
    out["oc"] = dict(d=_discrepancy(p0, seq, win), lseq=lseq, lwin=lwin, tr=tro, w=wo, tr_seq=trs,
                     d_center=_discrepancy(p0[-nc:], seq[-nc:], win[-nc:]), p0=p0, win=win, head=head, head0=head0)
    return out


# ---- "loss": "Focal" with use_supcon: the launches of a pass, on given logits and features (no model pass) ----
LABELS = (([1, 0, 1, 0], [1, 1, 0, 0], [0.3, 0.8]), ([0, 0, 1, 1], [1, 0, 1, 0], [0.6, 0.1]))
# the window's own shape (K = 2 micro-batches of B = 2: SupCon of two rows is 0 up to its 1e-8 terms), and the same
# four rows as ONE micro-batch of four, where every row has a positive and the term is far from 0
SHAPES = [(B, K), (K * B, 1)]


def _set_labels(w, which):
    ya, yb, lam = LABELS[which]
    w.ya.copy_(torch.tensor(ya))
    w.yb.copy_(torch.tensor(yb))
    w.lam.copy_(torch.tensor(lam[:w.K]))


def _given():
    g = torch.Generator().manual_seed(3)
    return (torch.randn(K * B, 2, generator=g).to(DEV).requires_grad_(True),
            torch.randn(K * B, 144, generator=g).to(DEV).requires_grad_(True))


def _supcon_module(tr, feats, which, wb, wk):
    """lambda * SupCon / accum of the module path on label set `which`, and its feature gradient."""
    from radhip.train import SupConLoss, feats_loss
    ya, yb, lam = (torch.tensor(v, device=DEV) for v in LABELS[which])
    ref = feats.detach().clone().requires_grad_(True)
    extra = feats_loss(tr.criterion, SupConLoss(0.07), 0.1, tr.accum, ref, ya, yb, lam[:wk], wb, fused=False)
    extra.backward()
    return float(extra.detach()), ref.grad


def _recorded(monkeypatch):
    from radhip import ops
    calls = []
    real_focal, real_oc = ops.mixup_focal, ops.mixup_ocsupcon
    monkeypatch.setattr(ops, "mixup_focal", lambda *a: calls.append(("focal", a)) or real_focal(*a))
    monkeypatch.setattr(ops, "mixup_ocsupcon", lambda *a: calls.append(("ocsupcon", a)) or real_oc(*a))
    return calls


@pytest.mark.parametrize("wb,wk", SHAPES)
def test_focal_launch_unchanged_and_supcon_added(focal_pair, monkeypatch, wb, wk):
    """Read from the config (build_supcon -> Trainer -> WindowStep._pass_loss): the pass issues the focal launch that
    the plain Focal config issues (same arguments, same loss and logit gradient, once) and one more launch that adds
    lambda * SupCon alone (no centre)."""
    from radhip.train import FocalLoss, SupConLoss
    from radhip.window import WindowStep
    trf, trs = focal_pair
    assert isinstance(trs.criterion, FocalLoss) and isinstance(trs.supcon, SupConLoss) and trs.lambda_supcon == 0.1
    assert trs.feats_criteria() and not trf.feats_criteria() and trs.crit_params == [] and trf.supcon is None
    calls = _recorded(monkeypatch)
    out, feats = _given()
    wf, ws = WindowStep(trf, wb, K=wk), WindowStep(trs, wb, K=wk)
    _set_labels(wf, 0)
    _set_labels(ws, 0)
    plain = wf._pass_loss(out, feats)
    assert [c[0] for c in calls] == ["focal"]
    focal_args = calls[0][1]
    plain.backward()
    assert feats.grad is None
    dout_plain, out.grad = out.grad, None
    calls.clear()
    both = ws._pass_loss(out, feats)
    assert [c[0] for c in calls] == ["focal", "ocsupcon"]
    same = lambda a, b: torch.equal(a, b) if torch.is_tensor(a) else a is b or a == b
    assert len(calls[0][1]) == len(focal_args) and calls[0][1][0] is out
    assert all(same(a, b) for a, b in zip(calls[0][1][1:-2], focal_args[1:-2]))     # labels, lam, rows per lam
    assert calls[0][1][-2] is trs.criterion and calls[0][1][-1] == focal_args[-1] == trs.accum
    assert (trs.criterion.alpha, trs.criterion.gamma, trs.criterion.alpha_mode) == \
           (trf.criterion.alpha, trf.criterion.gamma, trf.criterion.alpha_mode)
    assert calls[1][1][5] is None and calls[1][1][6] is trs.supcon               # SupCon alone, no OC-Softmax
    extra, dref = _supcon_module(trs, feats, 0, wb, wk)
    both.backward()
    assert torch.equal(out.grad, dout_plain)                                     # the focal launch's own output
    assert float(both.detach()) == pytest.approx(float(plain.detach()) + extra, rel=1e-5)
    scale = float(dref.abs().max())
    assert torch.allclose(feats.grad, dref, rtol=1e-4, atol=1e-5 * scale + 1e-12)
    if wb == K * B:
        assert extra > 1e-3 and scale > 1e-6


@pytest.mark.parametrize("wb,wk", SHAPES)
def test_focal_supcon_pass_loss_captured_replays_on_new_labels(focal_pair, monkeypatch, wb, wk):
    """The same pass loss and its backward captured in a HIP graph, as the window captures them: a replay on other
    labels and lam (read through the window's buffers) equals the focal launch plus the module SupCon on those.

    The leaves are made and first used on the warm-up's side stream: autograd runs a leaf's AccumulateGrad node on
    the stream the node was made on, and one made on the default stream (by an eager use whose graph is still alive)
    would pull the default stream into the capture."""
    from radhip.window import WindowStep
    trf, trs = focal_pair
    calls = _recorded(monkeypatch)
    out, feats = _given()
    wf, ws = WindowStep(trf, wb, K=wk), WindowStep(trs, wb, K=wk)
    _set_labels(ws, 0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out_g = out.detach().clone().requires_grad_(True)
        feats_g = feats.detach().clone().requires_grad_(True)
        ws._pass_loss(out_g, feats_g).backward()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    out_g.grad = feats_g.grad = None
    graph = torch.cuda.CUDAGraph()
    calls.clear()
    with torch.cuda.graph(graph):
        cap = ws._pass_loss(out_g, feats_g)
        cap.backward()
    assert [c[0] for c in calls] == ["focal", "ocsupcon"]
    seen = []
    for which in (0, 1):
        _set_labels(ws, which)
        _set_labels(wf, which)
        graph.replay()
        torch.cuda.synchronize()
        extra, dref = _supcon_module(trs, feats, which, wb, wk)
        plain = float(wf._pass_loss(out.detach(), feats.detach()))
        assert float(cap.detach()) == pytest.approx(plain + extra, rel=1e-5)
        scale = float(dref.abs().max())
        assert torch.allclose(feats_g.grad, dref, rtol=1e-4, atol=1e-5 * scale + 1e-12)
        seen.append(extra)
    if wb == K * B:
        assert abs(seen[1] - seen[0]) > 1e-3                                         # the replay saw the new labels


def test_window_oc_supcon_matches_sequential_within_todays_discrepancy(runs):
    (d_f, _), (d_o, floor) = runs["focal"]["d"], runs["oc"]["d"]
    d_c, floor_c = runs["oc"]["d_center"]
    bound = 4.0 * d_f + floor
    record("window[K2,B2,fp32,fgm]", {"focal_window_vs_sequential": d_f, "oc_supcon_window_vs_sequential": d_o,
                                      "floor": floor, "bound": bound, "centre_window_vs_sequential": d_c,
                                      "centre_floor": floor_c,
                                      "loss_sequential": runs["oc"]["lseq"], "loss_window": runs["oc"]["lwin"]})
    print(f"[window oc+supcon] update discrepancy: focal {d_f:.3e}, oc+supcon {d_o:.3e} (bound {bound:.3e}), "
          f"centre alone {d_c:.3e}")
    tr = runs["oc"]["tr"]
    nc = tr.criterion.center.numel()
    assert tr.params[-1] is tr.criterion.center
    assert not torch.equal(runs["oc"]["p0"][-nc:], runs["oc"]["win"][-nc:])         # the centre took its step
    # the classifier: no gradient, so the HIP AdamW of the window's step neither moved nor decayed it
    assert len(runs["oc"]["head"]) == len(runs["oc"]["head0"]) > 0
    assert all(p.grad is None for p in runs["oc"]["head"])
    assert all(any(p is q for g in tr.opt.param_groups for q in g["params"]) for p in runs["oc"]["head"])
    assert all(torch.equal(p.detach(), p0) for p, p0 in zip(runs["oc"]["head"], runs["oc"]["head0"]))
    assert runs["oc"]["lwin"] == pytest.approx(runs["oc"]["lseq"], rel=1e-5)
    assert d_o <= bound, (d_o, d_f, floor)
    assert d_c <= 4.0 * d_f + floor_c, (d_c, d_f, floor_c)


def test_graph_replay_reads_the_live_centre(runs):
    """The captured criterion launch holds the centre's pointer: a replay after the step sees the updated centre
    (its loss differs from a replay with the centre put back), and the same centre gives the same loss again."""
    tr, w = runs["oc"]["tr"], runs["oc"]["w"]
    nc = tr.criterion.center.numel()
    c_before = runs["oc"]["p0"][-nc:].view_as(tr.criterion.center)
    c_after = tr.criterion.center.detach().clone()
    step = tr.optimizer_step
    tr.optimizer_step = tr.grads.zero           # replays only: keep every parameter where it is
    try:
        def replay():
            tr.loss_sum.zero_()
            _stage(w)
            w.run()
            torch.cuda.synchronize()
            return float(tr.loss_sum)
        l_after = replay()
        with torch.no_grad():
            tr.criterion.center.copy_(c_before)
        l_before = replay()
        with torch.no_grad():
            tr.criterion.center.copy_(c_after)
        l_again = replay()
    finally:
        tr.optimizer_step = step
    # one AdamW step moves the centre by about base_lr per element, so the two losses differ by a small but
    # systematic amount: it must stand clear of what the same centre gives twice (the fp32 passes' run-to-run noise,
    # measured here) by 10x, and of 4 fp32 ulps of the loss
    noise = abs(l_again - l_after)
    record("window_replay_centre", {"loss_updated_centre": l_after, "loss_restored_centre": l_before,
                                    "loss_updated_centre_again": l_again})
    assert abs(l_after - l_before) > 10.0 * noise + 4.0 * EPS32 * abs(l_after), (l_after, l_before, l_again)
    assert l_again == pytest.approx(l_after, rel=1e-5)


def test_dev_scoring_uses_the_trained_centre(runs, tmp_path):
    """produce_evaluation_file_sharded with the OC-Softmax criterion writes the cosine to the (trained) centre."""
    from radhip.infer import _scores, produce_evaluation_file_sharded
    tr = runs["oc"]["tr"]
    xs, _, _, _ = _batches(1, B)
    x = xs[0]

    class DS:
        def __len__(self):
            return B

        def __getitem__(self, i):
            return x[i].cpu(), f"utt{i}"

    trial = tmp_path / "trial.txt"
    trial.write_text("".join(f"spk utt{i} - A0{i} bonafide\n" for i in range(B)))
    save = tmp_path / "dev_score.txt"
    produce_evaluation_file_sharded(DS(), tr.model, DEV, save, trial, batch_size=B, criterion=tr.criterion)
    got = np.array([float(line.split()[-1]) for line in save.read_text().splitlines()], dtype=np.float32)
    with torch.no_grad():
        feats, logits = tr.model(x)
        hand = (F.normalize(feats.float(), dim=1) * F.normalize(tr.criterion.center, dim=1)).sum(1)
        s = _scores(tr.model, x, tr.criterion)
    np.testing.assert_allclose(got, hand.cpu().numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(s.cpu().numpy(), hand.cpu().numpy(), rtol=1e-5, atol=1e-6)
    assert not np.allclose(got, logits[:, 1].float().cpu().numpy(), atol=1e-3)      # not the logit score
