"""WavLM encoder (HF-checkpoint compatible) tuned for the MI355X training step, plus peft-style LoRA.

The reference runs HF transformers' WavLMModel (src/models/DualStreamSEMamba.py:288-336,392-439)
wrapped by peft LoRA (src/main.py:103-158). This module re-implements that forward with identical
parameter names (so `microsoft/wavlm-large` / reference checkpoints load unchanged) and the same
train-mode semantics (dropouts, LayerDrop, SpecAugment time masks, gated relative position bias),
laid out for MI355X:
  * frozen base projections are pre-cast once to the autocast dtype and q/k/v are fused into ONE
    [3*H, H] GEMM per layer (hipBLASLt through PyTorch) — the reference re-casts 315 M frozen
    weights every forward and issues three GEMMs;
  * attention runs through F.scaled_dot_product_attention with the gated position bias as the
    additive mask (the reference goes through F.multi_head_attention_forward);
  * LoRA (r=8, alpha=32, q/v) adds its rank-8 update next to the fused GEMM.
The 25 hidden states are returned as a list (no stack); the layer-weighted sum is the HIP kernel
radhip.ops.layer_weighted_sum.
"""
import json
import math
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import featproj, wavlm_fused, wavlm_x3
from .ops import HALF, GatedAttention, PosConv, fe_conv_weights, feature_encoder_fused, half_dtype, posconv_weights

# microsoft/wavlm-large architecture (published config.json; dropout / SpecAugment values are
# restated, not verifiable offline: parity unpinned for those regularisers)
WAVLM_LARGE = dict(
    hidden_size=1024, num_hidden_layers=24, num_attention_heads=16, intermediate_size=4096, hidden_act="gelu",
    hidden_dropout=0.1, attention_dropout=0.1, activation_dropout=0.0, feat_proj_dropout=0.1, layerdrop=0.1,
    conv_dim=[512] * 7, conv_kernel=[10, 3, 3, 3, 3, 2, 2], conv_stride=[5, 2, 2, 2, 2, 2, 2], conv_bias=False,
    feat_extract_norm="layer", feat_extract_activation="gelu", do_stable_layer_norm=True,
    num_conv_pos_embeddings=128, num_conv_pos_embedding_groups=16, num_buckets=320, max_bucket_distance=800,
    layer_norm_eps=1e-5, apply_spec_augment=True, mask_time_prob=0.075, mask_time_length=10, mask_time_min_masks=2,
    mask_feature_prob=0.0, mask_feature_length=10, mask_feature_min_masks=0)


class WavLMConfigLite:
    def __init__(self, **kw):
        d = dict(WAVLM_LARGE)
        d.update({k: v for k, v in kw.items() if not k.startswith("_")})
        d["conv_dim"] = list(d["conv_dim"])
        self.__dict__.update(d)

    @classmethod
    def from_dir(cls, path):
        with open(os.path.join(path, "config.json")) as f:
            return cls(**json.load(f))

    def to_dict(self):
        return dict(self.__dict__)


def _act(name):
    if name == "gelu":
        return lambda x: F.gelu(x)
    if name in ("gelu_new", "gelu_pytorch_tanh"):
        return lambda x: F.gelu(x, approximate="tanh")
    if name == "relu":
        return F.relu
    raise ValueError(name)


# ----------------------------------------------------------------------------- caching -------
class _CastCache:
    """Holds autocast-dtype copies of FROZEN weights (re-made only when a source tensor changes)."""

    def __init__(self):
        self.key = None
        self.val = None

    def get(self, tensors, dtype, build):
        key = (dtype,) + tuple((t.data_ptr(), t._version, t.device) for t in tensors)
        if self.key != key:
            with torch.no_grad():
                self.val = build().to(dtype)
            self.key = key
        return self.val


def _compute_dtype(x):
    if torch.is_autocast_enabled(x.device.type):
        return torch.get_autocast_dtype(x.device.type)
    return x.dtype


def frozen_linear(x, lin, cache):
    """F.linear with a cached cast of a frozen nn.Linear (falls back to the live weight if trainable). A LoraLinear's
    `weight` / `bias` are its base layer's, so an active adapter's part is added here."""
    if isinstance(lin, LoraLinear):
        y = frozen_linear(x, lin.base_layer, cache)
        return y + lin.delta(x).to(y.dtype) if lin.active else y
    w, b = lin.weight, lin.bias
    if w.requires_grad or (b is not None and b.requires_grad):
        return F.linear(x, w, b)
    dt = _compute_dtype(x)
    if dt == w.dtype:
        return F.linear(x, w, b)
    ws = cache.get([w] + ([b] if b is not None else []), dt,
                   lambda: torch.cat([w.reshape(-1)] + ([b.reshape(-1)] if b is not None else [])))
    wc = ws[:w.numel()].view_as(w)
    bc = ws[w.numel():] if b is not None else None
    return F.linear(x.to(dt), wc, bc)


# ------------------------------------------------------------------------------- LoRA -------
class LoraLinear(nn.Module):
    """peft lora.Linear look-alike: base_layer + lora_A/lora_B/lora_dropout ModuleDicts keyed by
    adapter name ('default'); y = base(x) + (alpha/r) * B(A(dropout(x))). A ~ kaiming_uniform(a=sqrt 5),
    B = 0 (peft's init). Like peft's layer it exposes the base layer's `weight` / `bias`.

    active=False reproduces what the reference actually computes: transformers' WavLMAttention never calls
    q_proj / v_proj as modules, it hands `q_proj.weight` and the concatenated `.bias` to
    F.multi_head_attention_forward (modeling_wavlm.py, torch_multi_head_self_attention), and on a peft layer
    those are the base layer's tensors. So the adapters injected by src/main.py:103-158 never enter the
    forward: the outputs are the base model's and the LoRA weights get no gradient (AdamW skips them).
    active=True applies the adapter (what LoRA is meant to do; training_config "lora_mode": "active")."""

    def __init__(self, base, r=8, alpha=32, dropout=0.1, adapter="default", active=True):
        super().__init__()
        self.active = bool(active)
        self.base_layer = base
        self.in_features, self.out_features = base.in_features, base.out_features
        self.adapter = adapter
        self.r = {adapter: r}
        self.lora_alpha = {adapter: alpha}
        self.scaling = {adapter: alpha / r}
        dev = base.weight.device
        self.lora_A = nn.ModuleDict({adapter: nn.Linear(self.in_features, r, bias=False, device=dev)})
        self.lora_B = nn.ModuleDict({adapter: nn.Linear(r, self.out_features, bias=False, device=dev)})
        self.lora_dropout = nn.ModuleDict({adapter: nn.Dropout(dropout) if dropout > 0 else nn.Identity()})
        nn.init.kaiming_uniform_(self.lora_A[adapter].weight, a=math.sqrt(5))
        nn.init.zeros_(self.lora_B[adapter].weight)

    @property
    def weight(self):
        return self.base_layer.weight

    @property
    def bias(self):
        return self.base_layer.bias

    def delta(self, x):
        a = self.adapter
        return self.lora_B[a](self.lora_A[a](self.lora_dropout[a](x))) * self.scaling[a]

    def forward(self, x):
        return self.base_layer(x) + self.delta(x) if self.active else self.base_layer(x)


def _base(lin):
    return lin.base_layer if isinstance(lin, LoraLinear) else lin


# ---------------------------------------------------------------------------- modules -------
class ConvLayer(nn.Module):
    def __init__(self, cfg, i):
        super().__init__()
        cin = cfg.conv_dim[i - 1] if i > 0 else 1
        cout = cfg.conv_dim[i]
        self.conv = nn.Conv1d(cin, cout, cfg.conv_kernel[i], stride=cfg.conv_stride[i], bias=cfg.conv_bias)
        self.mode = cfg.feat_extract_norm
        if self.mode == "layer":
            self.layer_norm = nn.LayerNorm(cout, elementwise_affine=True)
        elif self.mode == "group" and i == 0:
            self.layer_norm = nn.GroupNorm(cout, cout, affine=True)
        else:
            self.layer_norm = None
        self.act = _act(cfg.feat_extract_activation)

    def forward(self, x):
        x = self.conv(x)
        if self.mode == "layer":
            x = self.layer_norm(x.transpose(-2, -1)).transpose(-2, -1)
        elif self.layer_norm is not None:
            x = self.layer_norm(x)
        return self.act(x)


class FeatureEncoder(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.conv_layers = nn.ModuleList([ConvLayer(cfg, i) for i in range(len(cfg.conv_dim))])
        self.cfg = cfg

    def _fused_ok(self, x):
        """bf16 / fp16 CUDA pass with the WavLM-Large CNN geometry and frozen weights -> csrc/featconv.hip (token-major
        conv0+LN+GELU kernel, implicit-GEMM convs, LN+GELU passes) instead of MIOpen convs plus transposes,
        casts and separate LayerNorm/GELU launches."""
        c = self.cfg
        return (x.is_cuda and x.dim() == 2 and torch.is_autocast_enabled("cuda")
                and torch.get_autocast_dtype("cuda") in HALF and len(c.conv_dim) >= 2
                and all(d == 512 for d in c.conv_dim) and c.conv_kernel[0] == 10
                and c.feat_extract_norm == "layer" and c.feat_extract_activation == "gelu"
                and all(k * 512 % 8 == 0 for k in c.conv_kernel)
                and os.environ.get("RADHIP_FUSED_FE", "1") != "0"
                and not any(p.requires_grad for p in self.parameters()))

    def forward(self, x):
        if self._fused_ok(x):
            hd = half_dtype()
            key = (hd,) + tuple((p.data_ptr(), p._version) for p in self.parameters())
            if getattr(self, "_fe_key", None) != key:
                self._fe_ops = fe_conv_weights(self.conv_layers, hd)
                self._fe_key = key
            return feature_encoder_fused(x, self._fe_ops).transpose(1, 2)     # [B, 512, T] view, as the modules
        x = x[:, None]
        for layer in self.conv_layers:
            x = layer(x)
        return x


class FeatureProjection(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.layer_norm = nn.LayerNorm(cfg.conv_dim[-1], eps=cfg.layer_norm_eps)
        self.projection = nn.Linear(cfg.conv_dim[-1], cfg.hidden_size)
        self.dropout = nn.Dropout(cfg.feat_proj_dropout)

    def forward(self, x):
        return self.dropout(self.projection(self.layer_norm(x)))


class PositionalConvEmbedding(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        k = cfg.num_conv_pos_embeddings
        conv = nn.Conv1d(cfg.hidden_size, cfg.hidden_size, kernel_size=k, padding=k // 2,
                         groups=cfg.num_conv_pos_embedding_groups)
        self.conv = nn.utils.parametrizations.weight_norm(conv, name="weight", dim=2)
        self.remove = 1 if k % 2 == 0 else 0
        self.act = _act(cfg.feat_extract_activation)
        self.act_name = cfg.feat_extract_activation

    def _weight(self):
        """weight_norm(v, g, dim=2). The WavLM encoder is frozen in Phase 6, so the normalised weight is
        cached and recomputed only when g or v change (the parametrization otherwise recomputes it on
        every call: ~0.8 ms per pass for the 1024x64x128 kernel)."""
        pz = self.conv.parametrizations.weight
        g, v = pz.original0, pz.original1
        if g.requires_grad or v.requires_grad:
            return self.conv.weight
        key = (g.data_ptr(), g._version, v.data_ptr(), v._version)
        if getattr(self, "_wkey", None) != key:
            with torch.no_grad():
                self._w = self.conv.weight.detach().clone()
            self._wkey = key
        return self._w

    def _fused_ok(self, x):
        """bf16 / fp16 CUDA step with the WavLM-Large geometry and frozen weights -> csrc/posconv.hip (one MFMA launch
        each way instead of MIOpen's per-utterance im2col + GEMM + col2im)."""
        c = self.conv
        return (x.is_cuda and x.dim() == 3 and torch.is_autocast_enabled("cuda")
                and torch.get_autocast_dtype("cuda") in HALF and c.in_channels == 1024
                and c.out_channels == 1024 and c.groups == 16 and c.kernel_size[0] == 128 and self.remove == 1
                and self.act_name == "gelu" and os.environ.get("RADHIP_FUSED_POSCONV", "1") != "0"
                and not any(p.requires_grad for p in c.parameters()))

    def forward(self, x):
        c = self.conv
        if self._fused_ok(x):
            w = self._weight()
            hd = half_dtype()
            key = (w.data_ptr(), getattr(self, "_wkey", None), hd)
            if getattr(self, "_pc_key", None) != key:
                self._pc = posconv_weights(w, hd)
                self._pc_key = key
            return PosConv.apply(x, self._pc[0], self._pc[1], c.bias)
        y = F.conv1d(x.transpose(1, 2), self._weight(), c.bias, c.stride, c.padding, c.dilation, c.groups)
        if self.remove:
            y = y[:, :, :-self.remove]
        return self.act(y).transpose(1, 2)


class Attention(nn.Module):
    def __init__(self, cfg, has_rel_bias):
        super().__init__()
        E, H = cfg.hidden_size, cfg.num_attention_heads
        self.embed_dim, self.num_heads, self.head_dim = E, H, E // H
        self.dropout = cfg.attention_dropout
        self.num_buckets, self.max_distance = cfg.num_buckets, cfg.max_bucket_distance
        self.k_proj = nn.Linear(E, E)
        self.v_proj = nn.Linear(E, E)
        self.q_proj = nn.Linear(E, E)
        self.out_proj = nn.Linear(E, E)
        self.gru_rel_pos_const = nn.Parameter(torch.ones(1, H, 1, 1))
        self.gru_rel_pos_linear = nn.Linear(self.head_dim, 8)
        if has_rel_bias:
            self.rel_attn_embed = nn.Embedding(self.num_buckets, H)
        self._qkv_cache = _CastCache()
        self._out_cache = _CastCache()

    def _buckets(self, T, device):
        pos = torch.arange(T, device=device)
        rel = pos[None, :] - pos[:, None]
        nb = self.num_buckets // 2
        buckets = (rel > 0).long() * nb
        rel = rel.abs()
        exact = nb // 2
        small = rel < exact
        large = exact + (torch.log(rel.float() / exact) / math.log(self.max_distance / exact) * (nb - exact)).long()
        large = torch.clamp(large, max=nb - 1)
        return buckets + torch.where(small, rel, large)

    def compute_bias(self, T, device):
        """[H, T, T] relative position bias (HF WavLMAttention.compute_bias), contiguous."""
        return self.rel_attn_embed(self._buckets(T, device)).permute(2, 0, 1).contiguous()

    def _qkv(self, h):
        q, k, v = self.q_proj, self.k_proj, self.v_proj
        bq, bk, bv = _base(q), _base(k), _base(v)
        frozen = not any(p.requires_grad for m in (bq, bk, bv) for p in m.parameters())
        if frozen:
            dt = _compute_dtype(h)
            ts = [bq.weight, bk.weight, bv.weight, bq.bias, bk.bias, bv.bias]
            wb = self._qkv_cache.get(ts, dt, lambda: torch.cat([t.reshape(-1) for t in ts]))
            E = self.embed_dim
            w = wb[:3 * E * E].view(3 * E, E)
            b = wb[3 * E * E:]
            qkv = F.linear(h.to(dt), w, b)
            qq, kk, vv = qkv.split(E, dim=-1)
        else:
            qq, kk, vv = bq(h), bk(h), bv(h)
        if isinstance(q, LoraLinear) and q.active:
            qq = qq + q.delta(h)
        if isinstance(k, LoraLinear) and k.active:
            kk = kk + k.delta(h)
        if isinstance(v, LoraLinear) and v.active:
            vv = vv + v.delta(h)
        return qq, kk, vv

    def forward(self, h, position_bias):
        B, T, E = h.shape
        H, Dh = self.num_heads, self.head_dim
        if position_bias is None:
            position_bias = self.compute_bias(T, h.device)                      # [H, T, T]
        # gate from the attention input (HF WavLMAttention.forward steps 1-4)
        g = self.gru_rel_pos_linear(h.view(B, T, H, Dh))                       # [B, T, H, 8]
        g = torch.sigmoid(g.view(B, T, H, 2, 4).sum(-1))                        # [B, T, H, 2]
        gate = g[..., 0] * (g[..., 1] * self.gru_rel_pos_const.view(1, 1, H) - 1.0) + 2.0   # [B, T, H]
        qq, kk, vv = self._qkv(h)
        dt = qq.dtype
        if (qq.is_cuda and dt in HALF and kk.dtype == dt and vv.dtype == dt and Dh == 64
                and not position_bias.requires_grad):
            # fused MFMA kernel (csrc/attention.hip): bias formed in registers, dropout mask from a device
            # seed (HIP-graph replayable), output already [B, T, E] for out_proj
            p = self.dropout if self.training else 0.0
            seed = getattr(self, "_seed", None) if p > 0 else None
            if p > 0 and seed is None:
                raise RuntimeError("attention dropout needs the encoder's device seed (Encoder.forward sets it)")
            o = GatedAttention.apply(qq, kk, vv, gate, position_bias, seed, p, getattr(self, "_salt", 0))
            return frozen_linear(o, self.out_proj, self._out_cache), position_bias
        bias = (gate.permute(0, 2, 1).unsqueeze(-1) * position_bias.unsqueeze(0)).to(dt)   # [B, H, T, T]
        qh = qq.view(B, T, H, Dh).transpose(1, 2)
        kh = kk.view(B, T, H, Dh).transpose(1, 2)
        vh = vv.view(B, T, H, Dh).transpose(1, 2)
        o = F.scaled_dot_product_attention(qh, kh, vh, attn_mask=bias,
                                           dropout_p=self.dropout if self.training else 0.0)
        o = o.transpose(1, 2).reshape(B, T, E)
        return frozen_linear(o, self.out_proj, self._out_cache), position_bias


class FeedForward(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.intermediate_dropout = nn.Dropout(cfg.activation_dropout)
        self.intermediate_dense = nn.Linear(cfg.hidden_size, cfg.intermediate_size)
        self.output_dense = nn.Linear(cfg.intermediate_size, cfg.hidden_size)
        self.output_dropout = nn.Dropout(cfg.hidden_dropout)
        self.act = _act(cfg.hidden_act)
        self._c1, self._c2 = _CastCache(), _CastCache()

    def forward(self, h):
        h = self.intermediate_dropout(self.act(frozen_linear(h, self.intermediate_dense, self._c1)))
        return self.output_dropout(frozen_linear(h, self.output_dense, self._c2))


class EncoderLayer(nn.Module):
    def __init__(self, cfg, has_rel_bias, stable):
        super().__init__()
        self.stable = stable
        self.attention = Attention(cfg, has_rel_bias)
        self.dropout = nn.Dropout(cfg.hidden_dropout)
        self.layer_norm = nn.LayerNorm(cfg.hidden_size, eps=cfg.layer_norm_eps)
        self.feed_forward = FeedForward(cfg)
        self.final_layer_norm = nn.LayerNorm(cfg.hidden_size, eps=cfg.layer_norm_eps)

    def forward(self, h, position_bias):
        if self.stable:  # HF WavLMEncoderLayerStableLayerNorm
            a, position_bias = self.attention(self.layer_norm(h), position_bias)
            h = h + self.dropout(a)
            h = h + self.feed_forward(self.final_layer_norm(h))
        else:            # HF WavLMEncoderLayer (post-LN)
            a, position_bias = self.attention(h, position_bias)
            h = self.layer_norm(h + self.dropout(a))
            h = self.final_layer_norm(h + self.feed_forward(h))
        return h, position_bias


class Encoder(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        self.stable = bool(cfg.do_stable_layer_norm)
        self.pos_conv_embed = PositionalConvEmbedding(cfg)
        self.layer_norm = nn.LayerNorm(cfg.hidden_size, eps=cfg.layer_norm_eps)
        self.dropout = nn.Dropout(cfg.hidden_dropout)
        self.layers = nn.ModuleList([EncoderLayer(cfg, i == 0, self.stable) for i in range(cfg.num_hidden_layers)])
        # device-side dropout seed of the fused attention kernel: advanced on the device once per forward,
        # so a captured HIP graph draws fresh masks on every replay; initialised from torch's CPU RNG
        self.register_buffer("_attn_rng", torch.randint(0, 2 ** 62, (1,), dtype=torch.int64), persistent=False)
        # HIP-graph mode: LayerDrop decisions come from this device bool [num_layers] (True = run the
        # layer); the layer is computed and torch.where selects, which is exact in value and gradient.
        self.keep_dev = None

    def forward(self, h, layerdrop=None):
        p = self.cfg.layerdrop if layerdrop is None else layerdrop
        h = h + self.pos_conv_embed(h)
        if not self.stable:
            h = self.layer_norm(h)
        h = self.dropout(h)
        states = []
        pos = None
        seed = None
        if self.training and h.is_cuda:
            self._attn_rng.add_(1)
            seed = self._attn_rng.clone()          # the value this forward (and its backward) uses
            for i, layer in enumerate(self.layers):
                layer.attention._seed, layer.attention._salt = seed, i
        fused = wavlm_fused.eligible(self, h)
        if fused:
            # fused bf16 layers (radhip/wavlm_fused.py) on an fp32 residual stream
            runner = self.__dict__.get("_fused")
            if runner is None:
                runner = self.__dict__["_fused"] = wavlm_fused.FusedEncoderRunner(self)
            loras = runner.prepare(h.device)
            pb = runner.position_bias(h.shape[1], h.device)
            h = h.float()
        # fused layers that always run back to back (no LayerDrop skip / select) chain their residuals and
        # gradients through each other (wavlm_fused.EncoderChain); the frontend's layer-weighted sum reads it
        chain = wavlm_fused.EncoderChain(len(self.layers)) if fused and (p == 0 or not self.training) else None
        self.state_defer = chain

        def run(i, layer, h, pos):
            if fused:
                return runner.layer(i, h, pb, loras, seed, chain), None
            return layer(h, pos)
        for i, layer in enumerate(self.layers):
            states.append(h)
            if self.training and self.keep_dev is not None and i > 0 and p > 0:
                hn, pos = run(i, layer, h, pos)
                # keep_dev: [num_layers] (one draw for the batch) or [B, num_layers] (one row per utterance)
                kp = self.keep_dev[i] if self.keep_dev.dim() == 1 else self.keep_dev[:, i].view(-1, 1, 1)
                h = torch.where(kp, hn, h)
                continue
            # HF draws torch.rand([]) for EVERY layer (train or eval) and skips when training, i > 0 and
            # draw < layerdrop; the same CPU-RNG consumption is kept here
            # (graph mode with layerdrop 0 keeps every layer: no select, no draw needed)
            r = float(torch.rand([])) if self.keep_dev is None else 1.0
            skip = self.training and i > 0 and p > 0 and r < p
            if not skip:
                h, pos = run(i, layer, h, pos)
        if self.stable:
            h = self.layer_norm(h)
        states.append(h)
        return h, states


def compute_time_mask(B, T, prob, length, min_masks):
    """SpecAugment time-span mask (restates transformers' _compute_mask_indices, no padding mask)."""
    eps = np.random.rand(1).item()

    def nspan(n):
        k = max(int(prob * n / length + eps), min_masks)
        if k * length > T:
            k = T // length
        if n - (length - 1) < k:
            k = max(n - (length - 1), 0)
        return k
    k = nspan(T)
    mask = np.zeros((B, T), dtype=bool)
    if k == 0:
        return mask
    for b in range(B):
        starts = np.random.choice(np.arange(T - (length - 1)), k, replace=False)
        idx = (starts[:, None] + np.arange(length)[None, :]).reshape(-1)
        idx = np.minimum(idx, T - 1)
        mask[b, idx] = True
    return mask


class WavLMEncoderModel(nn.Module):
    """HF WavLMModel parameter layout: feature_extractor, feature_projection, masked_spec_embed, encoder."""

    def __init__(self, cfg=None, **kw):
        super().__init__()
        self.config = cfg if isinstance(cfg, WavLMConfigLite) else WavLMConfigLite(**(cfg or {}), **kw)
        c = self.config
        self.feature_extractor = FeatureEncoder(c)
        self.feature_projection = FeatureProjection(c)
        for p in self.feature_projection.parameters():   # radhip/featproj.py accumulates their gradients into .grad
            p._radhip_direct_grad = True
        if c.mask_time_prob > 0 or c.mask_feature_prob > 0:
            self.masked_spec_embed = nn.Parameter(torch.Tensor(c.hidden_size).uniform_())
        self.encoder = Encoder(c)
        self.time_mask_dev = None   # HIP-graph mode: SpecAugment time mask [B, T] bool on the device
        # FGM: the adversarial pass feeds the same waveform through the frozen, eval-mode CNN, so its
        # features equal the clean pass's. cnn_reuse = "store" keeps them, "use" reuses them (exact).
        self.cnn_reuse = None
        self._cnn_feats = None
        # window mode (radhip/window.py): a frozen-CNN feature tensor handed in for this call, and
        # per-group leaf copies of the feature_projection parameters (K tuples (ln_w, ln_b, proj_w,
        # proj_b)); group k of the batch goes through copy k, so the batched clean pass yields each
        # micro-batch's own feature_projection gradient (the FGM attack needs the running sums)
        self.cnn_feats_given = None
        self.fp_groups = None
        self.fp_nocache = True

    def _cnn_frozen(self):
        return not self.feature_extractor.training and not any(p.requires_grad for p in self.feature_extractor.parameters())

    def forward(self, input_values, output_hidden_states=True, layerdrop=None):
        x = input_values
        if wavlm_x3.eligible(self, x):
            # the fp32 scoring pass on the split-precision kernels (radhip/wavlm_x3.py)
            self.encoder.state_defer = None
            return wavlm_x3.forward(self, x)
        frozen = self._cnn_frozen()
        if frozen and self.cnn_feats_given is not None:
            feats = self.cnn_feats_given
        elif frozen and self.cnn_reuse == "use" and self._cnn_feats is not None:
            if self._cnn_feats[0] != (x.data_ptr(), tuple(x.shape), x.dtype):
                raise RuntimeError("WavLM CNN feature reuse: the adversarial pass got a different input")
            feats = self._cnn_feats[1]
        elif frozen:
            with torch.no_grad():
                feats = self.feature_extractor(x)
            if self.cnn_reuse == "store":
                self._cnn_feats = ((x.data_ptr(), tuple(x.shape), x.dtype), feats)
        else:
            feats = self.feature_extractor(x)
        feats = feats.transpose(1, 2)
        if featproj.eligible(self.feature_projection, feats, self.fp_groups):
            h = featproj.feature_projection(self.feature_projection, feats, self.fp_groups)
        elif self.fp_groups is not None:
            fp = self.feature_projection
            K = len(self.fp_groups)
            parts = []
            for xk, (lw, lb, pw, pb) in zip(feats.chunk(K, dim=0), self.fp_groups):
                parts.append(F.linear(F.layer_norm(xk, xk.shape[-1:], lw, lb, fp.layer_norm.eps), pw, pb))
            h = fp.dropout(torch.cat(parts, dim=0))
        elif self.fp_nocache and torch.is_autocast_enabled("cuda"):
            # the FGM target changes between the passes of one autocast region: cast it afresh each time
            with torch.autocast("cuda", dtype=torch.get_autocast_dtype("cuda"), cache_enabled=False):
                h = self.feature_projection(feats)
        else:
            h = self.feature_projection(feats)
        c = self.config
        if self.training and getattr(c, "apply_spec_augment", True) and c.mask_time_prob > 0:
            B, T, _ = h.shape
            if self.time_mask_dev is not None:
                m = self.time_mask_dev
            else:
                m = torch.from_numpy(compute_time_mask(B, T, c.mask_time_prob, c.mask_time_length,
                                                       c.mask_time_min_masks)).to(h.device, non_blocking=True)
            h = torch.where(m[..., None], self.masked_spec_embed.to(h.dtype), h)
        last, states = self.encoder(h, layerdrop=layerdrop)
        return last, states


# --------------------------------------------------------------------------- peft wrapper ----
class _LoraModel(nn.Module):
    def __init__(self, model):
        super().__init__()
        self.model = model

    def __getattr__(self, name):
        try:
            return super().__getattr__(name)
        except AttributeError:
            return getattr(self.model, name)


class PeftWrapped(nn.Module):
    """State-dict layout of peft's PeftModel(LoraModel(model)): keys `base_model.model.<...>`."""

    def __init__(self, model):
        super().__init__()
        self.base_model = _LoraModel(model)

    def __getattr__(self, name):
        try:
            return super().__getattr__(name)
        except AttributeError:
            return getattr(self.base_model, name)

    def forward(self, *a, **k):
        return self.base_model.model(*a, **k)


# The attention projections HF WavLMAttention hands to F.multi_head_attention_forward by their .weight / .bias
# instead of calling them (so a peft adapter on them never runs in the reference); every other Linear is called.
ATTN_PROJECTIONS = ("q_proj", "k_proj", "v_proj", "out_proj")


def inject_lora(model, r=8, alpha=32, dropout=0.1, targets=("q_proj", "v_proj"), active=True):
    """Replace every nn.Linear whose attribute name is in `targets` by a LoraLinear (peft semantics:
    base frozen by the caller, LoRA trainable). Returns the wrapped model and the adapter count.
    active=False (lora_mode "reference") bypasses only the adapters the reference's HF WavLM never calls: the
    attention module's q/k/v/out projections; an adapter on any other Linear (e.g. the FFN's intermediate_dense /
    output_dense, which HF calls as modules) stays active, as peft applies it there."""
    n = 0
    for mod in list(model.modules()):
        for name, child in list(mod.named_children()):
            if name in targets and isinstance(child, nn.Linear):
                bypassed = isinstance(mod, Attention) and name in ATTN_PROJECTIONS
                setattr(mod, name, LoraLinear(child, r, alpha, dropout, active=active or not bypassed))
                n += 1
    return PeftWrapped(model), n


def inert_lora_params(model):
    """Parameters of adapters that never enter the forward (LoraLinear.active False): trainable in name, like
    the reference's, but they receive no gradient, so the optimizer and the gradient buffer leave them out."""
    out = []
    for mod in model.modules():
        if isinstance(mod, LoraLinear) and not mod.active:
            out += list(mod.lora_A.parameters()) + list(mod.lora_B.parameters())
    return out


def remap_peft_keys(state_dict, model_keys):
    """Accept both peft key layouts: new (`q_proj.base_layer.weight`) and old (`q_proj.weight`)."""
    out = dict(state_dict)
    for k in list(state_dict.keys()):
        for leaf in ("weight", "bias"):
            suf = "." + leaf
            if k.endswith(suf):
                alt = k[:-len(suf)] + ".base_layer" + suf
                if alt in model_keys and k not in model_keys:
                    out[alt] = out.pop(k)
    return out
