"""OC-Softmax + SupCon on csrc/ocsupcon.hip (radhip.ops.mixup_ocsupcon) against the module criteria.

Reference: the fp64 module path (radhip.train.feats_loss(..., fused=False) over OCSoftmax / SupConLoss, which
tests/test_oc_supcon_cpu.py pins against the reference's own classes) on the CPU, on inputs already rounded to the
storage dtype. Bound, per output (loss, dfeats, dcentre), MEASURED per case: the fp32 module path's own max error
against fp64 on the same inputs, on the GPU; the kernel may be at most 4x that (the two sum in different orders),
plus a floor of 4 fp32 ulps of the output's largest magnitude, plus, for dfeats written in a 16-bit dtype, half an ulp
of that dtype at each element. Every measured error and bound goes to profiles/ocsupcon_errors.json.

Cases: (K, B, D) in CASES (B = 2 and 3, several micro-batches, B = 64 = one lane per column, D = 1, D not a
multiple of 64, D = 256, and B = 64 with D = 256, the LDS limit), crossed with row stride D and D + 8, fp32 / bf16 /
fp16 features, OC only / SupCon only / both, and every variant of VARIANTS (mixup with distinct ya / yb and lam 0.3;
yb and lam absent with an incoming gradient of 1024, a GradScaler value; lam 0 with all rows of one class; lam 1
with a singleton class)."""
import json
import os

import numpy as np
import pytest
import torch

from seeded import seeded_array

pytestmark = pytest.mark.gpu
DEV = "cuda"
PROFILES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles")
RECORD = os.path.join(PROFILES, "ocsupcon_errors.json")

CASES = [(1, 2, 144), (1, 3, 144), (4, 8, 144), (2, 64, 144), (1, 8, 1), (1, 8, 130), (1, 8, 256),
         (1, 64, 256)]     # the last: 83.8 KiB of LDS, the one shape class above the 64 KiB a launch gets by default
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
MODES = ["oc", "supcon", "both"]
VARIANTS = ["mixup", "no_yb_grad1024", "lam0_same_class", "lam1_singleton"]
ACCUM, LAMBDA = 4, 0.1
EPS32 = float(np.finfo(np.float32).eps)


def record(key, obj):
    """Merge one entry into profiles/ocsupcon_errors.json (the record of the measured errors and bounds)."""
    os.makedirs(PROFILES, exist_ok=True)
    cur = {}
    if os.path.exists(RECORD):
        with open(RECORD) as f:
            cur = json.load(f)
    cur[key] = obj
    cur["_format"] = ("kernel[...] rows: per output [fp32 module path's max error against fp64, the kernel's (less half "
                      "a 16-bit ulp for 16-bit dfeats), the bound 4 x module + 4 fp32 ulps of the output's magnitude]")
    with open(RECORD, "w") as f:          # one entry per line
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(cur[k], sort_keys=True)}" for k in sorted(cur))
                + "\n}\n")


def _criteria(mode, center):
    """(criterion, supcon, lambda) whose OC-Softmax centre is `center` (a leaf of the wanted dtype and device)."""
    from radhip.train import FocalLoss, OCSoftmax, SupConLoss
    crit = FocalLoss()
    if mode in ("oc", "both"):
        crit = OCSoftmax(center.shape[1])
        crit.center = torch.nn.Parameter(center)
    return crit, (SupConLoss(0.07) if mode in ("supcon", "both") else None), LAMBDA


def _labels(variant, K, B, tag):
    ya = (seeded_array(f"ya{tag}", (K * B,), scale=1.0) > 0).astype(np.int64)
    if variant == "lam0_same_class":
        ya[:] = 1
    if variant == "lam1_singleton":
        ya[:] = 0
        ya[::B] = 1                      # one bona fide row per micro-batch
    yb = ya.reshape(K, B)[:, ::-1].reshape(-1).copy()
    lam = {"mixup": 0.3, "lam0_same_class": 0.0, "lam1_singleton": 1.0}.get(variant)
    if variant == "no_yb_grad1024":
        return ya, None, None, 1024.0
    return ya, yb, np.full(K, lam, np.float32) * (1.0 if variant != "mixup" else np.linspace(1.0, 0.5, K)), 1.0


def _module(mode, feats, center, ya, yb, lam, B, g, device, dtype):
    """Module path in `dtype` on `device`: (loss, dfeats, dcentre or None) for an incoming gradient g."""
    from radhip.train import feats_loss
    f = feats.to(device=device, dtype=dtype).requires_grad_(True)
    c = center.to(device=device, dtype=dtype).requires_grad_(True)
    crit, sc, lsc = _criteria(mode, c)
    t = lambda a, dt=None: None if a is None else torch.as_tensor(a).to(device=device, dtype=dt)
    loss = feats_loss(crit, sc, lsc, ACCUM, f, t(ya), t(yb), t(lam, dtype), B, fused=False)
    (loss * g).backward()
    dc = crit.center.grad if mode != "supcon" else None
    return loss.detach().double().cpu(), f.grad.double().cpu(), None if dc is None else dc.double().cpu()


def _kernel(mode, feats, center, ya, yb, lam, B, g, ld):
    from radhip.ops import mixup_ocsupcon
    R, D = feats.shape
    buf = torch.zeros(R, ld, dtype=feats.dtype, device=DEV)
    buf[:, :D] = feats.to(DEV)
    buf.requires_grad_(True)
    crit, sc, lsc = _criteria(mode, center.float().to(DEV).requires_grad_(True))
    t = lambda a, dt=None: None if a is None else torch.as_tensor(a).to(device=DEV, dtype=dt)
    oc = crit if mode != "supcon" else None
    loss = mixup_ocsupcon(buf[:, :D], t(ya), t(yb), t(lam, torch.float32), B, oc, sc, lsc, ACCUM)
    (loss * g).backward()
    assert loss.dtype == torch.float32 and buf.grad.dtype == feats.dtype
    assert not buf.grad[:, D:].any()
    dc = None if oc is None else oc.center.grad.double().cpu()
    return loss.detach().double().cpu(), buf.grad[:, :D].double().cpu(), dc, buf.grad[:, :D].clone(), loss.detach().clone()


def _half_ulp(ref, dtype):
    """Half an ulp of a 16-bit dtype at each element of ref (0 for fp32 outputs)."""
    if dtype == torch.float32:
        return torch.zeros_like(ref)
    fi = torch.finfo(dtype)
    return 0.5 * fi.eps * ref.abs().clamp(min=fi.smallest_normal)


def _sig(x):
    return float(f"{x:.4g}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("K,B,D", CASES)
def test_kernel_within_measured_module_error(K, B, D, dtype):
    """Every variant for every mode at both row strides: the fp64 reference and the fp32 module error are computed
    once per (variant, mode) and serve both strides (neither depends on the stride)."""
    rows, fails = [], []
    tag = f"{K}_{B}_{D}"
    feats = torch.from_numpy(seeded_array(f"f{tag}", (K * B, D), scale=1.0)).to(dtype)            # rounded first
    center = torch.from_numpy(seeded_array(f"c{D}", (1, D), scale=0.2)).float()
    for variant in VARIANTS:
        ya, yb, lam, g = _labels(variant, K, B, tag)
        for mode in MODES:
            ref = _module(mode, feats, center, ya, yb, lam, B, g, "cpu", torch.float64)
            mod = _module(mode, feats, center, ya, yb, lam, B, g, DEV, torch.float32)
            for ld in (D, D + 8):
                got = _kernel(mode, feats, center, ya, yb, lam, B, g, ld)
                row = {"ld": ld, "mode": mode, "variant": variant}
                for name, r, m, k, dt in (("loss", ref[0], mod[0], got[0], torch.float32),
                                          ("dfeats", ref[1], mod[1], got[1], dtype),
                                          ("dcenter", ref[2], mod[2], got[2], torch.float32)):
                    if r is None:
                        continue
                    e_mod = float((m - r).abs().max())
                    e_ker = float(((k - r).abs() - _half_ulp(r, dt)).clamp(min=0).max())
                    bound = 4.0 * e_mod + 4.0 * EPS32 * float(r.abs().max())
                    row[name] = [_sig(e_mod), _sig(e_ker), _sig(bound)]
                    print(f"[ocsupcon {tag} {variant} ld {ld} {mode} {dtype}] {name}: module {e_mod:.3e} "
                          f"kernel {e_ker:.3e} bound {bound:.3e}")
                    if not e_ker <= bound:
                        fails.append((variant, mode, ld, name, e_ker, bound))
                rows.append(row)
    record(f"kernel[K{K},B{B},D{D},{str(dtype).split('.')[-1]}]", rows)
    assert not fails, (tag, fails)


def test_launch_counts_recorded():
    """Not a gate: device kernels per pass (forward + backward) of the module criteria against the fused launch,
    counted with the torch profiler, for the record in profiles/ocsupcon_errors.json."""
    from torch.profiler import ProfilerActivity, profile
    K, B, D = 4, 8, 144
    feats = torch.from_numpy(seeded_array("pf", (K * B, D), scale=1.0)).float()
    center = torch.from_numpy(seeded_array("pc", (1, D), scale=0.2)).float()
    ya, yb, lam, g = _labels("mixup", K, B, "prof")
    counts = {}
    for name, fn in (("module", lambda: _module("both", feats, center, ya, yb, lam, B, g, DEV, torch.float32)),
                     ("fused", lambda: _kernel("both", feats, center, ya, yb, lam, B, g, D))):
        fn()                                     # warm-up outside the profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        kern = [e for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower()
                and "memset" not in e.name.lower()]
        counts[name] = {"kernels": len(kern),
                        "ocsupcon_kernels": sum("ocsupcon" in e.name for e in kern)}
    counts["note"] = ("K = 4 micro-batches of B = 8, D = 144, OC-Softmax + SupCon, forward + backward, including the "
                      "test helper's own copies and casts on both sides")
    print("[ocsupcon launches]", counts)
    record("launches_per_pass[K4,B8,D144]", counts)


def test_two_runs_are_bit_identical():
    K, B, D = 4, 8, 144
    feats = torch.from_numpy(seeded_array("bitf", (K * B, D), scale=1.0)).to(torch.bfloat16)
    center = torch.from_numpy(seeded_array("bitc", (1, D), scale=0.2)).float()
    ya, yb, lam, g = _labels("mixup", K, B, "bit")
    a = _kernel("both", feats, center, ya, yb, lam, B, 3.0, D)
    b = _kernel("both", feats, center, ya, yb, lam, B, 3.0, D)
    assert torch.equal(a[4], b[4]) and torch.equal(a[3], b[3]) and torch.equal(a[2], b[2])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_all_zero_row_is_finite(dtype):
    """A zero row is normalised by the eps clamp (its derivative is ~1e12 there, so values are not compared). fp32
    and bf16 storage hold such a gradient; fp16 storage cannot (its largest value is 65504: the row's gradient is
    inf there, as the module path's is under fp16 autocast, and GradScaler skips that step)."""
    B, D = 8, 144
    feats = torch.from_numpy(seeded_array("zf", (B, D), scale=1.0)).to(dtype)
    feats[3] = 0
    center = torch.from_numpy(seeded_array("zc", (1, D), scale=0.2)).float()
    ya, yb, lam, g = _labels("mixup", 1, B, "z")
    loss, df, dc, _, _ = _kernel("both", feats, center, ya, yb, lam, B, 1.0, D)
    assert torch.isfinite(loss) and torch.isfinite(df).all() and torch.isfinite(dc).all()


def test_ineligible_shapes_error_in_c_and_take_the_module_path():
    """B = 1, B = 65, D = 257 and an unaligned base: the C entry answers RDX_EUNSUPPORTED (-2), ops.mixup_ocsupcon
    raises, ops.ocsupcon_eligible is False and radhip.train.feats_loss computes the same loss through the modules."""
    from radhip import _lib, ops
    from radhip.train import feats_loss
    L = _lib.lib()
    for R, B, D, shift in ((4, 1, 144, 0), (65, 65, 144, 0), (8, 8, 257, 0), (8, 8, 144, 1)):
        base = torch.from_numpy(seeded_array(f"in{R}{B}{D}", (R * D + 4,), scale=1.0)).float().to(DEV)
        feats = base[shift:shift + R * D].view(R, D)
        center = torch.from_numpy(seeded_array(f"inc{D}", (1, D), scale=0.2)).float().to(DEV).requires_grad_(True)
        ya = torch.arange(R, device=DEV) % 2
        loss = torch.zeros((), device=DEV)
        d32 = torch.zeros(R, D, device=DEV)
        dcp = torch.zeros(max(R // B, 1), D, device=DEV)
        rc = L.rdx_ocsupcon_mixup_fwd(feats.data_ptr(), 0, D, R, D, center.data_ptr(), ya.data_ptr(), None, None, B,
                                      0.9, 0.5, 20.0, 0.1, 0.07, 0.07, 1.0, loss.data_ptr(), dcp.data_ptr(),
                                      d32.data_ptr(), dcp.data_ptr(), None)
        assert rc == -2, (R, B, D, shift, rc)
        assert not L.rdx_ocsupcon_eligible(feats.data_ptr(), D, R, D, B)
        assert not ops.ocsupcon_eligible(feats, B, center)
        crit, sc, lsc = _criteria("both", center)
        with pytest.raises(RuntimeError, match="unsupported"):
            ops.mixup_ocsupcon(feats, ya, None, None, B, crit, sc, lsc, 1)
        f = feats.clone().requires_grad_(True)
        got = feats_loss(crit, sc, lsc, 1, f, ya, None, None, B)
        want = feats_loss(crit, sc, lsc, 1, f, ya, None, None, B, fused=False)
        got.backward()
        assert torch.equal(got, want) and torch.isfinite(f.grad).all()
    torch.cuda.synchronize()
