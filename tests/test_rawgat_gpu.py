"""RawGAT-ST plugin (models/RawNetGatSpoofST.py) on the GPU.

  * the product model with seeded weights, fp32, against the reference module's outputs, gradients and BatchNorm
    running statistics (tests/golden/legacy_RawNetGatSpoofST.npz from make_golden_rawgat.py), in eval mode and in
    train mode with every Dropout at p = 0, with the checks and tolerances tests/test_legacy_gpu.py applies to AASIST
    (its _close_grads, replicated here), once with the fused graph attention (csrc/gat.hip, RADHIP_GAT=1) and once
    with RADHIP_GAT=0 (the module path, the default);
  * the fused path is taken: three ops.gat_att calls per forward with RADHIP_GAT=1, none with RADHIP_GAT=0;
  * the front end is the HIP kernel, run once for both encoders;
  * the CLI on RawGATST_baseline.conf: --eval of saved weights, in protocol order, equal to a direct forward."""
import json

import numpy as np
import pytest
import torch

from flac_writer import encode
from seeded import seeded_array, seeded_fill_

pytestmark = pytest.mark.gpu
DEV = "cuda"
ARCH, CONF = "RawNetGatSpoofST", "RawGATST_baseline.conf"


def _product(mode, seed):
    from radhip.build import get_model, load_config
    m = get_model(load_config(CONF)["model_config"], "cpu")
    seeded_fill_(m, seed=seed)
    m = m.to(DEV)
    if mode == "train":
        for d in m.modules():
            if isinstance(d, torch.nn.Dropout):
                d.p = 0.0
        m.train()
    else:
        m.eval()
    return m


def _rel_l2(got, ref, floor):
    return float(np.linalg.norm(got - ref)) / (float(np.linalg.norm(ref)) + floor * np.sqrt(ref.size))


def _close_grads(m, g, mode, tol=None, tol_bn=0.15):
    """tests/test_legacy_gpu.py::_close_grads: per-tensor relative L2 error against the float64 reference gradients,
    1 % in eval mode, 5 % in train mode (15 % for the affine weights of a batch-statistics BatchNorm), exactly-zero
    true gradients bounded by 1e-2 of the largest gradient; the reasons are written there."""
    tol = tol if tol is not None else (1e-2 if mode == "eval" else 5e-2)
    floor = 1e-5 * max(np.abs(g[k]).max() for k in list(g) if k.startswith(f"{mode}:grad:"))
    n = 0
    for k, p in m.named_parameters():
        got = None if p.grad is None else p.grad.detach().double().cpu().numpy()
        is_bn = any(q.startswith("bn") or q.endswith("_bn") for q in k.split(".")[:-1])
        t = tol_bn if mode == "train" and is_bn else tol
        if f"{mode}:grad:{k}" in g:
            ref = g[f"{mode}:grad:{k}"].astype(np.float64)
            assert got is not None, k
            if np.abs(ref).max() < 1e-4 * floor:        # exactly-zero true gradient (float64 holds ~1e-13)
                assert np.abs(got).max() < 1e3 * floor, (k, np.abs(got).max())
            else:
                assert _rel_l2(got, ref, floor) < t, (k, _rel_l2(got, ref, floor))
            n += 1
        elif f"{mode}:gradsum:{k}" in g:
            assert got is not None, k
            s = g[f"{mode}:gradsum:{k}"]
            assert abs(got.sum() - s[0]) < 5 * t * np.sqrt(abs(s[1])) + floor, (k, got.sum(), s[0])
            np.testing.assert_allclose((got * got).sum(), s[1], rtol=2 * t, err_msg=k)
            head = g[f"{mode}:gradhead:{k}"].astype(np.float64)
            assert _rel_l2(got.reshape(-1)[:64], head, floor) < t, k
            n += 1
        else:
            assert got is None or not np.any(got), f"{k}: gradient the reference does not have"
    return n


def _count_gat(monkeypatch):
    import radhip.ops as ops
    calls = []
    real = ops.gat_att
    monkeypatch.setattr(ops, "gat_att", lambda *a, **k: calls.append(1) or real(*a, **k))
    return calls


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "module"])
@pytest.mark.parametrize("mode", ["eval", "train"])
def test_model_matches_reference_fixture(golden, monkeypatch, mode, fused):
    g = golden(f"legacy_{ARCH}.npz")
    monkeypatch.setenv("RADHIP_GAT", "1" if fused else "0")
    calls = _count_gat(monkeypatch)
    m = _product(mode, int(g["seed"]))
    x = torch.from_numpy(seeded_array(f"{ARCH}.x", (2, 64600), scale=0.1).astype(np.float32)).to(DEV)
    hid, out = m(x, Freq_aug=False)
    assert len(calls) == (3 if fused else 0)
    assert hid.dtype == out.dtype == torch.float32
    np.testing.assert_allclose(hid.detach().cpu().numpy(), g[f"{mode}:hidden"], rtol=1e-3,
                               atol=1e-4 * np.abs(g[f"{mode}:hidden"]).max())
    np.testing.assert_allclose(out.detach().cpu().numpy(), g[f"{mode}:out"], rtol=1e-3,
                               atol=1e-4 * np.abs(g[f"{mode}:out"]).max())
    rh = torch.from_numpy(g[f"{mode}:rh"]).to(DEV)
    ro = torch.from_numpy(g[f"{mode}:ro"]).to(DEV)
    ((hid * rh).sum() + (out * ro).sum()).backward()
    n = _close_grads(m, g, mode)
    assert n >= 90, n
    if mode == "train":
        sd = m.state_dict()
        stats = [k for k in list(g) if k.startswith("stat:")]
        assert stats
        for k in stats:
            np.testing.assert_allclose(sd[k[5:]].cpu().numpy(), g[k], rtol=1e-4, atol=1e-6, err_msg=k)


def test_front_end_is_the_hip_kernel_run_once(monkeypatch):
    """conv_time runs rdx_sincconv_absmaxpool_fwd (no torch conv1d on the way), once for both encoders."""
    import radhip.ops as ops
    import radhip.sinc as S
    calls = []
    real = ops.sincconv_absmaxpool
    monkeypatch.setattr(S, "sincconv_absmaxpool", lambda *a, **k: calls.append(1) or real(*a, **k))

    def no_conv1d(*a, **k):
        raise AssertionError("torch conv1d in the RawGAT-ST front end")
    monkeypatch.setattr(torch.nn.functional, "conv1d", no_conv1d)
    monkeypatch.setenv("RADHIP_GAT", "1")
    gat = _count_gat(monkeypatch)
    m = _product("eval", 41)
    with torch.no_grad():
        hid, out = m(torch.zeros(1, 64600, device=DEV))
    assert calls == [1] and len(gat) == 3
    assert hid.shape == (1, 7) and out.shape == (1, 2)


# ------------------------------------------------------------------------------- CLI --------
def _write(path, n, seed):
    rng = np.random.default_rng(seed)
    x = np.clip(np.round(3000 * rng.standard_normal(n)), -32768, 32767).astype(np.int64)
    path.write_bytes(encode(x, plan=lambda f, c, b: {"kind": "verbatim"}))


def _database(root, golden, n_train):
    """The recipe of tests/test_legacy_gpu.py::_database: n_train train, 6 dev and 15 eval utterances."""
    proto = root / "ASVspoof2019_LA_cm_protocols"
    proto.mkdir(parents=True)
    attacks = [f"A{i:02d}" for i in range(7, 20)]
    rows = {"train": [("LA_T_%07d" % i, "-" if i % 5 == 0 else "A0%d" % (1 + i % 6),
                       "bonafide" if i % 5 == 0 else "spoof") for i in range(n_train)],
            "dev": [("LA_D_%07d" % i, "-" if i % 2 == 0 else "A02", "bonafide" if i % 2 == 0 else "spoof")
                    for i in range(6)],
            "eval": [("LA_E_%07d" % i, "-", "bonafide") for i in range(2)]
            + [("LA_E_%07d" % (i + 2), a, "spoof") for i, a in enumerate(attacks)]}
    names = {"train": "train.trn", "dev": "dev.trl", "eval": "eval.trl"}
    lens = [16000, 24000, 9000, 30000]
    for split, rs in rows.items():
        d = root / f"ASVspoof2019_LA_{split}" / "flac"
        d.mkdir(parents=True)
        lines = []
        for i, (utt, att, key) in enumerate(rs):
            _write(d / f"{utt}.flac", lens[i % len(lens)], seed=sum(map(ord, utt)))
            lines.append(f"LA_00{i % 100:02d} {utt} - {att} {key}")
        (proto / f"ASVspoof2019.LA.cm.{names[split]}.txt").write_text("\n".join(lines) + "\n")
    asv = root / "ASVspoof2019_LA_asv_scores"
    asv.mkdir()
    (asv / "ASVspoof2019.LA.asv.eval.gi.trl.scores.txt").write_text(
        "\n".join(golden("eval_golden.json")["tdcf"]["asv_lines"]) + "\n")
    return rows


def test_cli_eval_of_saved_weights(tmp_path, golden):
    """main.py --eval on RawGATST_baseline.conf: a reference-format state_dict (saved from the seeded model) loads
    strictly, the score file is in protocol order and equals a direct forward. The training half of the CLI (one
    epoch of one step at batch 24, dev / eval scoring, SWA) passed when measured but took 170 s, most of it in
    MIOpen's solver search, so it is not part of the suite."""
    import main as cli
    from radhip import audio
    from radhip.build import get_model, load_config, load_weights
    from radhip.data import pad
    db = tmp_path / "LA"
    rows = _database(db, golden, 24)
    cfg = load_config(CONF)
    cfg.update(database_path=str(db), num_epochs=1, eval_output="eval_scores.txt")
    assert cfg["batch_size"] == 24
    stem = CONF.split(".")[0]
    p = tmp_path / CONF
    p.write_text(json.dumps(cfg, indent=2))
    w = tmp_path / "seeded.pth"
    torch.save(_product("eval", 41).state_dict(), w)
    out = tmp_path / "exp"
    cli.main(cli.parse_args(["--config", str(p), "--output_dir", str(out), "--eval", "--eval_model_weights",
                             str(w), "--comment", "ev"]))
    lines = (out / f"LA_{stem}_ep1_bs24_ev" / "eval_scores.txt").read_text().splitlines()
    assert [ln.split()[0] for ln in lines] == [u for u, _, _ in rows["eval"]]
    got = np.array([float(ln.split()[3]) for ln in lines])
    assert np.isfinite(got).all()
    m = get_model(cfg["model_config"], DEV)
    load_weights(m, w, DEV, strict=True)
    m.eval()
    paths = [db / "ASVspoof2019_LA_eval" / "flac" / f"{u}.flac" for u, _, _ in rows["eval"]]
    x = np.stack([pad(audio.read(q)[0]) for q in paths]).astype(np.float32)
    with torch.no_grad():
        _, o = m(torch.from_numpy(x).to(DEV))
    np.testing.assert_allclose(got, o[:, 1].float().cpu().numpy(), rtol=1e-4, atol=1e-5)
