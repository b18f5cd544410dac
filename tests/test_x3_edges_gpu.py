"""The x3 scoring stream (radhip/wavlm_x3.py, csrc/x3.hip, csrc/hgemm.hip rdx_hgemm_x3) away from the one state
tests/test_x3_gpu.py runs it in: after the weights change, with adapters outside q / v, and at the shapes where its
kernels change path.

Everything runs on a 2-layer WavLM-Large-geometry stream (`eligible()` does not look at depth, so every x3 kernel and
GEMM policy runs at a twelfth of the weights). The references are fp64 and share no code with the kernels:
  A, B  the Phase-6 model of test_x3_gpu._model_and_oracle at depth 2 against the LoRA-free fp64 oracle
        (transformers' WavLM), loaded with every applied adapter folded into its Linear in fp64 (_oracle_state).
        Bound: the project's 1e-3 on the logits, with the classifier scaled so that max |logit| is about 10. Every
        case first shows on the reference alone that the change under test moves the logits by >= 1e-2, so a stream
        that ignores the change misses the bound tenfold.
  C     wavlm_x3.forward against the same module's torch path in fp64, every hidden state, max |x3 - ref| <=
        1e-3 max |ref|: the sum of the per-kernel relative bounds test_x3_gpu.py asserts along the 2-layer chain
        (CNN 1e-4, 6 LayerNorms 1e-5, 9 GEMMs 5e-5, posconv 2e-5, 2 attentions 1e-5: about 6.5e-4); a wrong tail row
        or tile is an O(1) error. The measured maxima go to profiles/x3_edge_errors.json.
  D     the kernel forms the stream uses and no other test calls, at the tolerances test_x3_gpu.py holds each
        kernel to.
"""
import copy
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from test_x3_gpu import DEV, PROFILES, _gemm_err, _model_and_oracle, _oracle_state, _planes

pytestmark = pytest.mark.gpu
N2 = 1e-3        # the logit bound
POWER = 1e-2     # what a change under test has to move the fp64 logits by
QV = ("q_proj", "v_proj")
# sizes of the changes, chosen in fp64 on the oracle alone so that each moves the logits by >= POWER
LORA_STEP = 3e-3     # per element of the LoRA factors (their size is about 0.03): moves the logits by about 0.3
FGM_EPS = 1.0        # the reference's epsilon: about 0.4
REL_STEP = 1.0       # N(0, 1) on rel_attn_embed (N(0, 1))
LORA_B_STD = {"gru_rel_pos_linear": 1.0}     # 0.02 moves the logits by 3e-3 only through the 8 x 8 gate adapter
_CACHE = {}


def _wave(B, L, seed=21):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(np.clip(0.1 * rng.standard_normal((B, L)), -1, 1).astype(np.float32)).to(DEV)


# ------------------------------------------------------------------------------------- A / B fixtures ----------
def _base():
    """Built once: the 2-layer Phase-6 model without LoRA, the fp64 oracle every layout reloads, three utterances;
    the classifier scaled so that the oracle's max |logit| is 10."""
    if "base" not in _CACHE:
        m, o = _model_and_oracle("reference", depth=2, targets=[])
        x = _wave(3, 64600)
        with torch.no_grad():
            s = 10.0 / float(o(x.double())[1][:, 1].abs().max())
            m.classifier.weight.mul_(s)
            m.classifier.bias.mul_(s)
        _CACHE["base"] = (m, o, x)
    return _CACHE["base"]


def _ref(m, adapters=None):
    """fp64 logits[:, 1] of the oracle reloaded from m's present state."""
    _, o, x = _base()
    o.load_state_dict(_oracle_state(m, adapters), strict=True)
    with torch.no_grad():
        return o(x.double())[1][:, 1]


def _base_logits():
    if "base_logits" not in _CACHE:
        _CACHE["base_logits"] = _ref(_base()[0])
    return _CACHE["base_logits"]


def _layout(lora_mode, targets):
    """Built once per adapter layout: a copy of the base model with those adapters injected, every lora_B
    N(0, 0.02) (peft's zero would leave the adapters without a part to play; LORA_B_STD where that is too little
    for the power condition)."""
    key = (lora_mode, tuple(targets))
    if key not in _CACHE:
        from radhip.build import apply_lora_to_wavlm
        m = _drop(copy.deepcopy(_base()[0]))
        torch.manual_seed(99)
        m = apply_lora_to_wavlm(m, {"use_lora": True, "lora_mode": lora_mode, "lora_target_modules": list(targets),
                                    "lora_r": 8, "lora_alpha": 32, "lora_dropout": 0.1})
        with torch.no_grad():
            for n, p in m.named_parameters():
                if "lora_B" in n:
                    p.normal_(0, next((v for k, v in LORA_B_STD.items() if k in n), 0.02))
        _CACHE[key] = m.eval()
    return _CACHE[key]


def _fresh(lora_mode="active", targets=QV):
    """A private copy of a layout for a test that changes weights."""
    return _drop(copy.deepcopy(_layout(lora_mode, targets) if targets else _base()[0])).eval()


def _core(m):
    return m.wavlm_stream._core()


def _drop(m):
    """Without the planes its source had cached."""
    _core(m).__dict__.pop("_x3w", None)
    return m


def _planes_of(m):
    cur = _core(m).__dict__.get("_x3w")
    return None if cur is None else cur[1]


def _x3(m):
    from radhip.infer import _scores
    with torch.no_grad():
        return _scores(m, _base()[2], None, "x3").double()


def _lora_params(m):
    return [p for n, p in m.named_parameters() if "lora_" in n]


def _seeded_like(ps, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return [torch.randn(p.shape, generator=g).to(DEV) for p in ps]


def _tracks(m, ref_before, what):
    """x3 scores of m's present weights: within N2 of the reloaded oracle, which itself moved by >= POWER."""
    s, r = _x3(m), _ref(m)
    err, moved = float((s - r).abs().max()), float((r - ref_before).abs().max())
    print(f"[x3 {what}] reference moved {moved:.3e}, x3 max abs err {err:.3e}")
    assert _planes_of(m) is not None, "the x3 stream did not run"
    assert moved >= POWER, (what, moved)
    assert err < N2, (what, err)
    return s, r


# --------------------------------------------------------------------------- A: scoring after a weight change ----
def test_x3_planes_reused_while_nothing_changes():
    m = _layout("active", QV)
    s0 = _x3(m)
    w0 = _planes_of(m)
    s1 = _x3(m)
    assert w0 is not None and _planes_of(m) is w0, "the planes were rebuilt with no weight change in between"
    assert torch.equal(s0, s1)


@pytest.mark.parametrize("path", ["rdx_adamw_many", "torch_step"])
def test_x3_scores_follow_adamw_step(path):
    """radhip.optim.AdamW writes the parameters through raw pointers (the covered path) or torch's fused step
    (amsgrad is outside the kernel's cover). lr = LORA_STEP: a first Adam step moves every LoRA element by about lr, a
    tenth of their size."""
    from radhip.optim import AdamW
    m = _fresh()
    r0 = _ref(m)
    assert float((_x3(m) - r0).abs().max()) < N2
    ps = _lora_params(m)
    opt = AdamW(ps, lr=LORA_STEP, weight_decay=0.0, amsgrad=(path == "torch_step"))
    for p, g in zip(ps, _seeded_like(ps, 5)):
        p.grad = g
    covered = opt._covered(opt.param_groups[0], ps)
    assert covered == (path == "rdx_adamw_many")
    opt.step()
    _tracks(m, r0, f"AdamW.step ({path})")


def test_x3_scores_follow_ema_swap():
    """EMA.swap exchanges live and shadow values through p.data: after the swap the scores are the shadow's, after
    a second swap the live ones again."""
    from radhip.optim import AdamW
    from radhip.train import EMA
    m = _fresh()
    ema = EMA(m)
    ema.update()                                   # shadow = the present weights
    r_shadow = _ref(m)
    s_shadow = _x3(m)
    assert float((s_shadow - r_shadow).abs().max()) < N2
    ps = _lora_params(m)
    opt = AdamW(ps, lr=LORA_STEP, weight_decay=0.0)
    for p, g in zip(ps, _seeded_like(ps, 6)):
        p.grad = g
    opt.step()
    s_live, r_live = _tracks(m, r_shadow, "EMA: optimizer step")
    ema.swap()
    s, _ = _tracks(m, r_live, "EMA.swap (shadow in)")
    assert float((s - r_shadow).abs().max()) < N2
    ema.swap()
    s, _ = _tracks(m, r_shadow, "EMA.swap (live back)")
    assert float((s - r_live).abs().max()) < N2


def test_x3_scores_follow_fgm_attack_and_restore():
    """FGM writes feature_projection through p.data (no LoRA freeze on the stream, feature_projection trainable).
    The scores track the attacked weights and, after the restore, equal the clean ones bit for bit."""
    from radhip.train import FGM
    m = _fresh(targets=())
    fp = _core(m).feature_projection
    fp.requires_grad_(True)
    ps = list(fp.parameters())
    for p, g in zip(ps, _seeded_like(ps, 7)):
        p.grad = g
    r0 = _ref(m)
    s0 = _x3(m)
    assert float((s0 - r0).abs().max()) < N2
    fgm = FGM(m, emb_name="feature_projection", epsilon=FGM_EPS)
    fgm.attack()
    _tracks(m, r0, "FGM.attack")
    fgm.restore()
    s2 = _x3(m)
    assert torch.equal(s2, s0), float((s2 - s0).abs().max())


def test_x3_scores_follow_load_state_dict():
    m = _fresh()
    r0 = _ref(m)
    assert float((_x3(m) - r0).abs().max()) < N2
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    names = [k for k in sd if "lora_" in k]
    for k, d in zip(names, _seeded_like([sd[k] for k in names], 8)):
        sd[k] += LORA_STEP * d.sign()
    m.load_state_dict(sd, strict=True)
    _tracks(m, r0, "load_state_dict")


class _Utterances:
    def __init__(self, x):
        self.x = x.cpu()

    def __len__(self):
        return len(self.x)

    def __getitem__(self, i):
        return self.x[i], f"utt{i}"


def test_x3_scoring_pass_sees_foreign_writes(tmp_path, monkeypatch):
    """A write no hook of the project sees (p.data.add_ on the LoRA factors, then on rel_attn_embed.weight) between
    two passes of produce_evaluation_file_sharded(amp="x3"), the trainer's entry: three utterances in batches of two
    (the second batch is the one-utterance tail of an eval, M = 201 < 256)."""
    from radhip import wavlm_x3
    from radhip.infer import produce_evaluation_file_sharded
    m = _fresh()
    ds = _Utterances(_base()[2])
    ran = []
    fwd = wavlm_x3.forward
    monkeypatch.setattr(wavlm_x3, "forward", lambda model, x: (ran.append(x.shape[0]), fwd(model, x))[1])

    def one_pass(tag):
        path = str(tmp_path / f"{tag}.txt")
        produce_evaluation_file_sharded(ds, m, DEV, path, None, batch_size=2, fmt="2021", amp="x3")
        with open(path) as f:
            rows = [ln.split() for ln in f]
        assert [r[0] for r in rows] == ["utt0", "utt1", "utt2"]
        return torch.tensor([float(r[1]) for r in rows], dtype=torch.float64, device=DEV)

    r0 = _ref(m)
    assert float((one_pass("clean") - r0).abs().max()) < N2
    assert ran == [2, 1], "the pass did not take the x3 stream"
    ps = _lora_params(m)
    for p, d in zip(ps, _seeded_like(ps, 9)):
        p.data.add_(LORA_STEP * d.sign())
    r1 = _ref(m)
    s1 = one_pass("lora")
    emb = _core(m).encoder.layers[0].attention.rel_attn_embed.weight
    emb.data.add_(REL_STEP * _seeded_like([emb], 10)[0])
    r2 = _ref(m)
    s2 = one_pass("rel")
    for what, s, r, before in (("LoRA factors", s1, r1, r0), ("rel_attn_embed", s2, r2, r1)):
        err, moved = float((s - r).abs().max()), float((r - before).abs().max())
        print(f"[x3 foreign write: {what}] reference moved {moved:.3e}, x3 max abs err {err:.3e}")
        assert moved >= POWER, (what, moved)
        assert err < N2, (what, err)
    assert ran == [2, 1] * 3
    assert _planes_of(m) is None, "the planes stay resident after the pass"


# ------------------------------------------------------------------------------------- B: adapter layouts ----------
LAYOUTS = [QV, QV + ("intermediate_dense", "output_dense"), ("k_proj", "out_proj"), ("projection",),
           ("gru_rel_pos_linear",)]


@pytest.mark.parametrize("lora_mode", ["reference", "active"])
@pytest.mark.parametrize("targets", LAYOUTS, ids="+".join)
def test_x3_adapter_layouts(lora_mode, targets):
    """x3 logits within 1e-3 of the fp64 oracle for adapters on every Linear of the stream, in both modes. Power, on
    the reference alone: where the layout has an applied adapter, the logits with the adapters differ from those
    without by >= 1e-2 (dropping one fails); where every adapter is bypassed (attention projections in "reference"
    mode) the reference is the base model's, and applying them anyway would move it by >= 1e-2 (merging one
    fails)."""
    from radhip.wavlm import LoraLinear
    m = _layout(lora_mode, targets)
    ref = _ref(m)
    adapters = [mod for mod in m.modules() if isinstance(mod, LoraLinear)]
    assert len(adapters) == (1 if targets == ("projection",) else 2 * len(targets))      # 2 layers
    if any(a.active for a in adapters):
        power = float((ref - _base_logits()).abs().max())
    else:
        assert float((ref - _base_logits()).abs().max()) == 0.0
        power = float((_ref(m, adapters=True) - ref).abs().max())
    got = _x3(m)
    err = float((got - ref).abs().max())
    print(f"[x3 adapters {lora_mode} {'+'.join(targets)}] power {power:.3e}, x3 max abs err {err:.3e}, "
          f"x3 stream {'ran' if _planes_of(m) is not None else 'refused'}")
    assert power >= POWER, power
    assert err < N2, err
    if targets == QV:
        assert _planes_of(m) is not None, "the x3 stream fell back for the default q / v layout"


# ------------------------------------------------------------------------------- C: shape edges of the stream ----
def _stream():
    """Built once: the 2-layer stream on the GPU in eval mode and its fp64 copy (the module path)."""
    if "stream" not in _CACHE:
        from radhip.wavlm import WavLMConfigLite, WavLMEncoderModel
        torch.manual_seed(7)
        model = WavLMEncoderModel(WavLMConfigLite(num_hidden_layers=2)).to(DEV).eval()
        for p in model.parameters():
            p.requires_grad_(False)
        _CACHE["stream"] = (model, copy.deepcopy(model).double())
    return _CACHE["stream"]


def _record(key, row):
    """Merge one shape's measured maxima into profiles/x3_edge_errors.json."""
    path = os.path.join(PROFILES, "x3_edge_errors.json")
    try:
        with open(path) as f:
            res = json.load(f)
    except (OSError, ValueError):
        res = {}
    res[key] = row
    os.makedirs(PROFILES, exist_ok=True)
    with open(path, "w") as f:
        json.dump(dict(sorted(res.items())), f, indent=1)
        f.write("\n")


# L, T, B: one token; nt = 1 exactly; nt = 3 (<4>); nt = 5 (first of <8>); posconv block + 2 rows; the one-utterance
# eval tail (M = 201 < 256); nt = 14 (first of <16>); the limit T = 256 with B * H >= 256 (qsplit 1)
SHAPES = [(400, 1, 1), (5200, 16, 3), (10640, 33, 2), (20880, 65, 1), (41680, 130, 2), (64600, 201, 1),
          (66960, 209, 2), (82000, 256, 17)]


@pytest.mark.parametrize("L,T,B", SHAPES)
def test_x3_stream_shape_edges(L, T, B):
    from radhip import wavlm_x3
    model, ref = _stream()
    x = _wave(B, L, seed=L)
    with torch.no_grad():
        _, want = ref(x.double())
        # the fp32 torch path beside it (the native convolutions: no solver search per new shape)
        with torch.backends.cudnn.flags(enabled=False):
            _, t32 = model(x)
        model.__dict__.pop("_x3w", None)
        with wavlm_x3.scoring():
            assert wavlm_x3.eligible(model, x)
            _, got = model(x)
    torch.cuda.synchronize()
    assert "_x3w" in model.__dict__, "the x3 stream did not run"
    assert len(got) == len(want) == len(t32) == 3
    row = {"L": L, "T": T, "B": B, "x3_rel_err": [], "fp32_torch_rel_err": [], "ref_absmax": []}
    for g, w, t in zip(got, want, t32):
        assert g.shape == w.shape == (B, T, 1024) and g.dtype == torch.float32
        assert bool(torch.isfinite(g).all())
        scale = float(w.abs().max())
        row["ref_absmax"].append(scale)
        row["x3_rel_err"].append(float((g.double() - w).abs().max()) / scale)
        row["fp32_torch_rel_err"].append(float((t.double() - w).abs().max()) / scale)
    print(f"[x3 stream L {L} T {T} B {B}] max |x3 - ref| / max |ref| per state "
          f"{['%.2e' % e for e in row['x3_rel_err']]}, fp32 torch {['%.2e' % e for e in row['fp32_torch_rel_err']]}")
    _record(f"L{L}_T{T}_B{B}", row)
    assert max(row["x3_rel_err"]) <= 1e-3, row["x3_rel_err"]


def test_x3_stream_longer_than_256_tokens_takes_the_module_path():
    """L = 82320 makes T = 257, past rdx_x3_attn_fwd: under scoring() the call does not raise and returns the
    module path's result, with no planes built."""
    from radhip import wavlm_x3
    model, _ = _stream()
    x = _wave(1, 82320, seed=3)
    model.__dict__.pop("_x3w", None)
    with torch.no_grad(), torch.backends.cudnn.flags(enabled=False):
        _, want = model(x)
        with wavlm_x3.scoring():
            assert wavlm_x3.active() and not wavlm_x3.eligible(model, x)
            _, got = model(x)
    assert "_x3w" not in model.__dict__
    assert len(got) == len(want) == 3 and got[0].shape == (1, 257, 1024)
    for g, w in zip(got, want):
        assert torch.equal(g, w)
    assert wavlm_x3.tokens(model.config, 82320) == 257 and wavlm_x3.tokens(model.config, 82319) == 256
    assert wavlm_x3.tokens(model.config, 400) == 1 and wavlm_x3.tokens(model.config, 399) == 0


# ------------------------------------------------------------------------------------------ D: kernel forms ----------
SENTINEL = -1.5          # exact in bf16 and fp32


def _ln_args(M, E, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    a = torch.randn(M, E, generator=g).to(DEV)
    b = torch.randn(M, E, generator=g).to(DEV)
    gm = (1 + 0.1 * torch.randn(E, generator=g)).to(DEV)
    bt = (0.1 * torch.randn(E, generator=g)).to(DEV)
    return a, b, gm, bt


@pytest.mark.parametrize("M", [1, 2, 5])
@pytest.mark.parametrize("ldo", [512, 520])
def test_x3_ln_split_e512_planes(M, ldo):
    """feature_projection's form: E = 512 into planes (M not a multiple of the 4 rows of a block, ldo > E into a
    wider buffer). hi + lo is LN(x); hi is bf16 of the fp32 result and lo the bf16 of what hi leaves."""
    from radhip._lib import check
    from radhip.ops import _p
    from radhip.wavlm_x3 import lib
    E = 512
    a, _, gm, bt = _ln_args(M, E, 100 + M)
    hi = torch.full((M, ldo), SENTINEL, device=DEV, dtype=torch.bfloat16)
    lo = torch.full_like(hi, SENTINEL)
    y32 = torch.empty(M, E, device=DEV)
    check(lib().rdx_x3_ln_split(_p(a), None, None, _p(gm), _p(bt), 1e-5, _p(hi), _p(lo), ldo, _p(y32), None, None,
                                None, None, M, E, None), "x3_ln_split")
    torch.cuda.synchronize()
    ref = torch.nn.functional.layer_norm(a.double(), (E,), gm.double(), bt.double(), 1e-5)
    assert float((hi[:, :E].double() + lo[:, :E].double() - ref).abs().max()) < 1e-5 * float(ref.abs().max())
    assert float((y32.double() - ref).abs().max()) < 1e-5 * float(ref.abs().max())
    assert torch.equal(hi[:, :E], y32.to(torch.bfloat16))
    assert torch.equal(lo[:, :E], (y32 - hi[:, :E].float()).to(torch.bfloat16))
    assert bool((hi[:, E:] == SENTINEL).all()) and bool((lo[:, E:] == SENTINEL).all())


@pytest.mark.parametrize("M", [1, 2, 5])
def test_x3_ln_split_e1024_sum_into_fp32(M):
    """The final LayerNorm's form: E = 1024, x = a + b, fp32 out, no planes."""
    from radhip.wavlm_x3 import _ln
    E = 1024
    a, b, gm, bt = _ln_args(M, E, 200 + M)
    y32 = torch.full((M + 1, E), SENTINEL, device=DEV)
    hi, lo = _ln(a, (gm, bt, 1e-5), out_planes=False, b=b, y32=y32)
    torch.cuda.synchronize()
    assert hi is None and lo is None
    ref = torch.nn.functional.layer_norm((a + b).double(), (E,), gm.double(), bt.double(), 1e-5)
    assert float((y32[:M].double() - ref).abs().max()) < 1e-5 * float(ref.abs().max())
    assert bool((y32[M] == SENTINEL).all()), "a row past M was written"


@pytest.mark.parametrize("rows,cols", [(5, 12), (403, 1024)])
def test_x3_split(rows, cols):
    from radhip._lib import check
    from radhip.ops import _p
    from radhip.wavlm_x3 import lib
    g = torch.Generator(device="cpu").manual_seed(rows + cols)
    ldx, ldo = cols + 4, cols + 8
    x = torch.randn(rows, ldx, generator=g).to(DEV)
    hi = torch.full((rows, ldo), SENTINEL, device=DEV, dtype=torch.bfloat16)
    lo = torch.full_like(hi, SENTINEL)
    check(lib().rdx_x3_split(_p(x), ldx, rows, cols, _p(hi), _p(lo), ldo, None), "x3_split")
    torch.cuda.synchronize()
    v = x[:, :cols]
    assert torch.equal(hi[:, :cols], v.to(torch.bfloat16))
    resid = (v.double() - hi[:, :cols].double() - lo[:, :cols].double()).abs()
    assert bool((resid <= 2.0 ** -17 * v.double().abs()).all())
    assert bool((hi[:, cols:] == SENTINEL).all()) and bool((lo[:, cols:] == SENTINEL).all())


def _attn_case(B, T, qsplit, ld=None, ldo=1024):
    """rdx_x3_attn_fwd against fp64 at 1e-5 of the output scale. ld None: q | k | v interleaved rows of 3E (the
    stream's form); else three separate buffers of row stride ld."""
    from radhip import _lib
    from radhip.ops import _p
    from radhip.wavlm_x3 import lib
    H, E = 16, 1024
    g = torch.Generator(device="cpu").manual_seed(1000 * B + T)
    if ld is None:
        qkv = torch.randn(B * T, 3 * E, generator=g).to(DEV)
        q, k, v, ld = qkv[:, :E], qkv[:, E:2 * E], qkv[:, 2 * E:], 3 * E
    else:
        q, k, v = (torch.randn(B * T, ld, generator=g).to(DEV) for _ in range(3))
    gate = (1 + 0.5 * torch.rand(B * T, H, generator=g)).to(DEV)
    rel = torch.randn(H, 2 * T - 1, generator=g).to(DEV)
    oh = torch.full((B * T, ldo), SENTINEL, device=DEV, dtype=torch.bfloat16)
    ol = torch.full_like(oh, SENTINEL)
    _lib.check(lib().rdx_x3_attn_fwd(_p(q), _p(k), _p(v), ld, _p(gate), _p(rel), 0.125, _p(oh), _p(ol), ldo, B, T, H,
                                     qsplit, None), "x3_attn")
    torch.cuda.synchronize()
    q6, k6, v6 = (t[:, :E].double().reshape(B, T, H, 64).permute(0, 2, 1, 3) for t in (q, k, v))
    i = torch.arange(T, device=DEV)
    bias = rel.double()[:, (i[None, :] - i[:, None] + T - 1)]                       # [H, T(i), T(j)]
    gb = gate.double().view(B, T, H).permute(0, 2, 1)[..., None] * bias[None]       # [B, H, T, T]
    p = torch.softmax(0.125 * q6 @ k6.transpose(-1, -2) + gb, dim=-1)
    ref = (p @ v6).permute(0, 2, 1, 3).reshape(B * T, E)
    got = oh[:, :E].double() + ol[:, :E].double()
    assert float((got - ref).abs().max()) < 1e-5 * float(ref.abs().max())
    assert bool((oh[:, E:] == SENTINEL).all()) and bool((ol[:, E:] == SENTINEL).all())


@pytest.mark.parametrize("T", [1, 16, 17, 64, 65, 208, 209])
def test_x3_attention_instantiation_boundaries(T):
    """nt = ceil(T / 16) at and just past the <4>, <8>, <13> / <16> instantiations, and one token."""
    _attn_case(2, T, 2)


@pytest.mark.parametrize("B,T,qsplit,ld,ldo", [(2, 33, 16, None, 1024),       # more splits than tiles
                                               (1, 201, 5, None, 1024),       # the last block holds a single tile
                                               (2, 50, 2, 1032, 1024),        # q, k, v apart, ld != 3E
                                               (2, 50, 1, None, 1040)])       # out rows wider than E
def test_x3_attention_forms(B, T, qsplit, ld, ldo):
    _attn_case(B, T, qsplit, ld, ldo)


def _posconv_weights():
    if "posconv" not in _CACHE:
        g = torch.Generator(device="cpu").manual_seed(13)
        W = (torch.randn(1024, 64, 128, generator=g) / (64 * 128) ** 0.5).to(DEV)
        bias = (0.1 * torch.randn(1024, generator=g)).to(DEV)
        _CACHE["posconv"] = (W, bias, _planes(W.reshape(16, 64, 64, 128).permute(0, 3, 1, 2).contiguous()))
    return _CACHE["posconv"]


@pytest.mark.parametrize("T", [1, 127, 128, 129, 256])
def test_x3_posconv_row_block_edges(T):
    """Around the 128-row block of a workgroup, at B = 2; a guard row past the output stays untouched."""
    from radhip import _lib
    from radhip.ops import _p
    from radhip.wavlm_x3 import lib
    B = 2
    W, bias, (wh, wl) = _posconv_weights()
    g = torch.Generator(device="cpu").manual_seed(T)
    h = torch.randn(B, T, 1024, generator=g).to(DEV)
    out = torch.full((B * T + 1, 1024), SENTINEL, device=DEV)
    _lib.check(lib().rdx_x3_posconv_fwd(_p(h), _p(wh), _p(wl), _p(bias), _p(out), B, T, None), "x3_posconv")
    torch.cuda.synchronize()
    y = torch.nn.functional.conv1d(h.double().transpose(1, 2), W.double(), bias.double(), padding=64, groups=16)
    ref = h.double() + torch.nn.functional.gelu(y[..., :T].transpose(1, 2))
    assert float((out[:B * T].view(B, T, 1024).double() - ref).abs().max()) < 2e-5 * float(ref.abs().max())
    assert bool((out[B * T] == SENTINEL).all())


@pytest.mark.parametrize("L,layers", [(400, 7), (330, 2)])
def test_x3_feature_encoder_token_block_edges(L, layers):
    """rdx_x3_fe_conv0 through feature_encoder: L = 400 (79 conv0 tokens, the second 64-token block partly filled,
    one token out of the whole CNN) and L = 330 (65 conv0 tokens: one past a block), the latter through conv0 and
    the first strided GEMM layer only, as seven layers leave no token of it."""
    from radhip import wavlm_x3
    model, ref = _stream()
    W = copy.copy(wavlm_x3.weights(model))
    W.fe = W.fe[:layers - 1]
    x = _wave(3, L, seed=L)
    with torch.no_grad():
        got = wavlm_x3.feature_encoder(W, x)
        y = x.double()[:, None]
        for layer in ref.feature_extractor.conv_layers[:layers]:
            y = layer(y)
    want = y.transpose(1, 2)
    assert (L - 10) // 5 + 1 == (79 if L == 400 else 65)
    assert got.shape == want.shape == (3, 1 if L == 400 else 32, 512)
    assert float((got.double() - want).abs().max()) < 1e-4 * float(want.abs().max())


@pytest.mark.parametrize("fp32_out", [False, True])
def test_x3_fe_ln_gelu_row_tail_and_bias(fp32_out):
    from radhip._lib import check
    from radhip.ops import _p
    from radhip.wavlm_x3 import lib
    R, C = 5, 512
    g = torch.Generator(device="cpu").manual_seed(17)
    x = torch.randn(R, C, generator=g).to(DEV)
    bias = torch.randn(C, generator=g).to(DEV)
    gm = (1 + 0.1 * torch.randn(C, generator=g)).to(DEV)
    bt = (0.1 * torch.randn(C, generator=g)).to(DEV)
    hi = torch.full((R + 1, C), SENTINEL, device=DEV, dtype=torch.bfloat16)
    lo = torch.full_like(hi, SENTINEL)
    o32 = torch.full((R + 1, C), SENTINEL, device=DEV)
    check(lib().rdx_x3_fe_ln_gelu(_p(x), R, _p(bias), _p(gm), _p(bt), 1e-5, None if fp32_out else _p(hi),
                                  None if fp32_out else _p(lo), _p(o32) if fp32_out else None, None), "x3_fe_ln_gelu")
    torch.cuda.synchronize()
    ref = torch.nn.functional.gelu(torch.nn.functional.layer_norm(x.double() + bias.double(), (C,), gm.double(),
                                                                  bt.double(), 1e-5))
    got = o32[:R].double() if fp32_out else hi[:R].double() + lo[:R].double()
    assert float((got - ref).abs().max()) < 1e-5 * float(ref.abs().max())
    assert bool((o32[R] == SENTINEL).all()) and bool((hi[R] == SENTINEL).all()) and bool((lo[R] == SENTINEL).all())
    if not fp32_out:       # lo is what hi leaves, not a second copy
        assert float((hi[:R].double() - ref).abs().max()) > 10 * float((got - ref).abs().max())


@pytest.mark.parametrize("M,N,K,pol", [(201, 3072, 1024, "qkv"), (201, 1024, 4096, "ffn2")])
def test_x3_gemm_one_utterance_rows(M, N, K, pol):
    """The 256-row tiles at M = 201 < 256, the last one-utterance batch of an eval."""
    from radhip import wavlm_x3
    g = torch.Generator(device="cpu").manual_seed(M + N + K)
    a = torch.randn(M, K, generator=g).to(DEV)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(DEV)
    bias = (0.1 * torch.randn(N, generator=g)).to(DEV)
    ah, al = _planes(a)
    got = wavlm_x3.gemm(ah, al, _planes(w), bias, pol=pol)
    ref = a.double() @ w.double().t() + bias.double()
    assert got.dtype == torch.float32 and got.shape == (M, N)
    assert _gemm_err(got, a.double(), w.double(), ref) < 5e-5


def test_x3_gemm_gelu_split_one_row():
    """FFN1 + GELU into planes at M = 1 (one token, L = 400)."""
    from radhip import _lib, wavlm_x3
    g = torch.Generator(device="cpu").manual_seed(19)
    a = torch.randn(1, 1024, generator=g).to(DEV)
    w = (torch.randn(4096, 1024, generator=g) / 32).to(DEV)
    bias = (0.1 * torch.randn(4096, generator=g)).to(DEV)
    ah, al = _planes(a)
    vh, vl = wavlm_x3.gemm(ah, al, _planes(w), bias, epilogue=_lib.EPI_F32_GELU_SPLIT, pol="ffn1")
    assert vh.shape == vl.shape == (1, 4096) and vh.dtype == vl.dtype == torch.bfloat16
    ref = torch.nn.functional.gelu(a.double() @ w.double().t() + bias.double())
    got = vh.double() + vl.double()
    assert float((got - ref).abs().max()) < 5e-5 * float(ref.abs().max())
    assert float((vh.double() - ref).abs().max()) > 10 * float((got - ref).abs().max())


def test_x3_gemm_batched_conv_short():
    """The CNN's batched strided form with fewer output rows than a tile: B = 2, T = 9, k = 3, s = 2 (To = 4)."""
    from radhip import wavlm_x3
    g = torch.Generator(device="cpu").manual_seed(23)
    B, T, C, k, s = 2, 9, 512, 3, 2
    x = torch.randn(B, T, C, generator=g).to(DEV)
    w = (torch.randn(C, C, k, generator=g) / (C * k) ** 0.5).to(DEV)
    To = (T - k) // s + 1
    xh, xl = _planes(x)
    y = torch.full((B * To + 1, C), float(SENTINEL), device=DEV)
    wavlm_x3.gemm(xh, xl, _planes(w.permute(0, 2, 1).reshape(C, k * C)), None, out=y[:B * To].view(B, To, C), M=To,
                  lda=s * C, sa=T * C, batch=B, sc=To * C, K=k * C, pol="cnn")
    torch.cuda.synchronize()
    ref = torch.nn.functional.conv1d(x.double().transpose(1, 2), w.double(), stride=s).transpose(1, 2)
    assert float((y[:B * To].view(B, To, C).double() - ref).abs().max()) < 5e-5 * float(ref.abs().max())
    assert bool((y[B * To] == SENTINEL).all())


def test_x3_c_abi_rejections():
    """T = 257, E = 768 and a misaligned pointer come back as the error code (check() raises) without a launch:
    the outputs keep their fill. The fp16-storage library refuses x3 altogether."""
    from radhip import _lib
    from radhip.ops import _p
    from radhip.wavlm_x3 import lib
    H, E = 16, 1024
    T = 257
    qkv = torch.zeros(T, 3 * E, device=DEV)
    gate = torch.ones(T, H, device=DEV)
    rel = torch.zeros(H, 2 * T - 1, device=DEV)
    oh = torch.full((T, E), SENTINEL, device=DEV, dtype=torch.bfloat16)
    ol = torch.full_like(oh, SENTINEL)

    def attn(q, t):
        return lib().rdx_x3_attn_fwd(q, _p(qkv[:, E:]), _p(qkv[:, 2 * E:]), 3 * E, _p(gate), _p(rel), 0.125, _p(oh),
                                     _p(ol), E, 1, t, H, 2, None)
    with pytest.raises(RuntimeError, match="x3_attn"):
        _lib.check(attn(_p(qkv), 257), "x3_attn")
    with pytest.raises(RuntimeError, match="x3_attn"):
        _lib.check(attn(ctypes.c_void_p(qkv.data_ptr() + 4), 256), "x3_attn")
    a = torch.zeros(4, 768, device=DEV)
    gm = torch.ones(768, device=DEV)
    y32 = torch.full((4, 768), SENTINEL, device=DEV)
    with pytest.raises(RuntimeError, match="x3_ln_split"):
        _lib.check(lib().rdx_x3_ln_split(_p(a), None, None, _p(gm), _p(gm), 1e-5, None, None, 768, _p(y32), None,
                                         None, None, None, 4, 768, None), "x3_ln_split")
    code = _lib.lib16().rdx_x3_split(_p(a), 768, 4, 768, _p(oh), _p(ol), 768, None)
    assert code == -1                               # RDX_EINVAL
    torch.cuda.synchronize()
    assert bool((oh == SENTINEL).all()) and bool((ol == SENTINEL).all()) and bool((y32 == SENTINEL).all())
