"""Writes tests/golden/legacy_RawNetGatSpoofST.npz from the reference's models/RawNetGatSpoofST.py.

    python tests/golden/make_golden_rawgat.py --ref <reference checkout>

Same scheme as make_golden.gen_legacy (which stays as it is): the reference Model built from its own
src/config/RawGATST_baseline.conf, float64 throughout (conv_time.band_pass included), weights from
seeded_fill_(m, seed), input seeded_array("RawNetGatSpoofST.x", (2, 64600), scale=0.1) (recomputed by the tests, not
stored), two modes: eval, and train with every Dropout at p = 0. Stored per mode: {mode}:hidden, {mode}:out, the
backward weights {mode}:rh / {mode}:ro, every parameter gradient of sum(hidden * rh) + sum(out * ro) ({mode}:grad:*,
or gradsum / gradhead above 4096 elements); stat:* the running statistics after the train-mode forward; the
state_dict keys and shapes; the model_config as a JSON string; the seed. Outputs, gradients and statistics are kept in
float64: tests/test_rawgat_cpu.py compares a float64 run at rtol 1e-9.

Top-k pooling is discontinuous: a run in another precision that ranks two nodes differently keeps another node set.
So for the three pools and both modes the smallest gap between the last kept and the first dropped sigmoid score
is recorded ({mode}:topk_gap, order pool_T, pool_S, pool_ST), and the file is written only if every gap is >= 1e-3;
otherwise the next seed is tried.

Only recorded arrays and the settings string go into the file, no program text of the reference."""
import argparse
import copy
import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from seeded import seeded_array, seeded_fill_  # noqa: E402

ARCH = "RawNetGatSpoofST"
MIN_GAP = 1e-3
POOLS = ("pool_T", "pool_S", "pool_ST")


def grads_of(module, full_max=4096):
    """Full float64 gradients for small tensors; (sum, sum of squares, first 64 values) for large ones."""
    out = {}
    for k, p in module.named_parameters():
        if p.grad is None:
            continue
        g = p.grad.detach().numpy().astype(np.float64)
        if g.size <= full_max:
            out[f"grad:{k}"] = g
        else:
            out[f"gradsum:{k}"] = np.array([g.sum(), (g * g).sum()])
            out[f"gradhead:{k}"] = g.reshape(-1)[:64].copy()
    return out


def run(mod, mc, seed):
    """The arrays of one seed and the smallest top-k gap over pools and modes."""
    arrays = {"seed": np.array(seed), "model_config": np.array(json.dumps(mc))}
    x = seeded_array(f"{ARCH}.x", (2, 64600), scale=0.1).astype(np.float32)
    worst = np.inf
    for mode in ("eval", "train"):
        torch.manual_seed(0)
        m = mod.Model(copy.deepcopy(mc))
        seeded_fill_(m, seed=seed)
        m = m.double()
        m.conv_time.band_pass = m.conv_time.band_pass.double()
        if mode == "train":
            for d in m.modules():
                if isinstance(d, torch.nn.Dropout):
                    d.p = 0.0
            m.train()
        else:
            m.eval()
        gaps = {}
        hooks = []
        for name in POOLS:
            pool = getattr(m, name)

            def hook(_mod, _inp, scores, name=name, pool=pool):
                n = max(int(scores.size(1) * pool.k), 2)
                s = torch.sort(scores.detach().squeeze(-1), dim=1, descending=True)[0]
                gaps[name] = float((s[:, n - 1] - s[:, n]).min()) if n < s.size(1) else np.inf
            hooks.append(pool.sigmoid.register_forward_hook(hook))
        hid, out = m(torch.from_numpy(x).double(), Freq_aug=False)
        for h in hooks:
            h.remove()
        arrays[f"{mode}:topk_gap"] = np.array([gaps[n] for n in POOLS])
        worst = min(worst, min(gaps.values()))
        rh = seeded_array(f"{ARCH}.rh", tuple(hid.shape)).astype(np.float32)
        ro = seeded_array(f"{ARCH}.ro", tuple(out.shape)).astype(np.float32)
        ((hid * torch.from_numpy(rh).double()).sum() + (out * torch.from_numpy(ro).double()).sum()).backward()
        arrays[f"{mode}:hidden"] = hid.detach().numpy()
        arrays[f"{mode}:out"] = out.detach().numpy()
        arrays[f"{mode}:rh"] = rh
        arrays[f"{mode}:ro"] = ro
        for k, v in grads_of(m).items():
            arrays[f"{mode}:{k}"] = v
        sd = m.state_dict()
        if mode == "train":
            for k, v in sd.items():
                if k.endswith("running_mean") or k.endswith("running_var"):
                    arrays[f"stat:{k}"] = v.numpy()
        else:
            arrays["keys"] = np.array(list(sd.keys()))
            arrays["shapes"] = np.array([json.dumps(list(v.shape)) for v in sd.values()])
            arrays["n_params"] = np.array(sum(p.numel() for p in m.parameters()))
    return arrays, worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="root of the reference checkout")
    ap.add_argument("--seed", type=int, default=41, help="first seed tried")
    ap.add_argument("--tries", type=int, default=8)
    a = ap.parse_args()
    spec = importlib.util.spec_from_file_location(f"ref_{ARCH}", os.path.join(a.ref, "models", ARCH + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(os.path.join(a.ref, "src", "config", "RawGATST_baseline.conf")) as f:
        mc = json.load(f)["model_config"]
    for seed in range(a.seed, a.seed + a.tries):
        arrays, gap = run(mod, mc, seed)
        print(f"seed {seed}: smallest top-k gap {gap:.3e}", {k: v.tolist() for k, v in arrays.items()
                                                              if k.endswith("topk_gap")})
        if gap >= MIN_GAP:
            path = os.path.join(HERE, f"legacy_{ARCH}.npz")
            np.savez_compressed(path, **arrays)
            print("wrote", os.path.relpath(path, HERE), f"{os.path.getsize(path) / 1024:.1f} KB")
            return
    raise SystemExit(f"no seed in [{a.seed}, {a.seed + a.tries}) keeps every top-k gap >= {MIN_GAP}")


if __name__ == "__main__":
    main()
