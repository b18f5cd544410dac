"""Generate tests/golden/oc_supcon.npz by running the REFERENCE's own criteria (its src/loss.py, imported, not
copied): OC-Softmax and SupCon values and gradients in float64 on the CPU, and the centre the reference draws after
torch.manual_seed(1234).

    python tests/golden/make_golden_losses.py --ref <reference checkout>

Contents (float64 unless noted), D = 144:
  center_seed1234 [1, D]   OCSoftmax(feat_dim=D).center drawn right after torch.manual_seed(1234) (fp32 values)
  for B in 2, 3, 8:  f{B} [B, D] features, and for each label set S in mixed / bonafide / singleton:
      y{B}_{S} int64 [B];  oc{B}_{S}, sc{B}_{S} scalars (SupCon on F.normalize(f), as train_epoch calls it);
      oc_df{B}_{S} [B, D], oc_dc{B}_{S} [1, D], sc_df{B}_{S} [B, D] gradients
      mix{B}_ya, mix{B}_yb int64 [B], mix{B}_lam scalar, mix{B}_lambda (0.1): the mixup total
      lam (P(ya) + lambda S(ya)) + (1 - lam) (P(yb) + lambda S(yb)) as mix{B}_total, mix{B}_df, mix{B}_dc
The OC-Softmax constants are the reference's defaults (r_real 0.9, r_fake 0.5, alpha 20), SupCon's temperature 0.07.
"""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
D = 144
LABELS = {
    2: {"mixed": [1, 0], "bonafide": [1, 1], "singleton": [0, 1]},
    3: {"mixed": [1, 0, 1], "bonafide": [1, 1, 1], "singleton": [0, 1, 1]},
    8: {"mixed": [1, 0, 0, 1, 0, 1, 1, 0], "bonafide": [1] * 8, "singleton": [0, 0, 0, 1, 0, 0, 0, 0]},
}
MIX = {2: ([1, 0], [0, 1], 0.3), 3: ([1, 0, 1], [0, 1, 1], 0.3), 8: ([1, 0, 0, 1, 0, 1, 1, 0], [0, 0, 1, 1, 1, 0, 1, 0], 0.3)}
LAMBDA = 0.1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="the reference checkout (its src/loss.py is imported)")
    ap.add_argument("--out", default=os.path.join(HERE, "oc_supcon.npz"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(args.ref, "src"))
    from loss import OCSoftmax, SupConLoss

    out = {}
    torch.manual_seed(1234)
    oc = OCSoftmax(feat_dim=D)
    out["center_seed1234"] = oc.center.detach().double().numpy()
    oc = oc.double()
    sc = SupConLoss(temperature=0.07)
    rng = np.random.default_rng(20240)

    def grads(fn, f):
        f = f.clone().requires_grad_(True)
        oc.center.grad = None
        v = fn(f)
        v.backward()
        dc = oc.center.grad.clone().numpy() if oc.center.grad is not None else None
        return float(v.detach()), f.grad.numpy(), dc

    for B, sets in LABELS.items():
        f = torch.from_numpy(rng.standard_normal((B, D)))
        out[f"f{B}"] = f.numpy()
        for name, y in sets.items():
            y = torch.tensor(y, dtype=torch.int64)
            out[f"y{B}_{name}"] = y.numpy()
            out[f"oc{B}_{name}"], out[f"oc_df{B}_{name}"], out[f"oc_dc{B}_{name}"] = grads(lambda t: oc(t, y), f)
            out[f"sc{B}_{name}"], out[f"sc_df{B}_{name}"], _ = grads(lambda t: sc(F.normalize(t, dim=1), y), f)
        ya, yb, lam = MIX[B]
        ya, yb = torch.tensor(ya, dtype=torch.int64), torch.tensor(yb, dtype=torch.int64)

        def total(t):
            def one(y):
                return oc(t, y) + LAMBDA * sc(F.normalize(t, dim=1), y)
            return lam * one(ya) + (1 - lam) * one(yb)
        out[f"mix{B}_ya"], out[f"mix{B}_yb"] = ya.numpy(), yb.numpy()
        out[f"mix{B}_lam"], out[f"mix{B}_lambda"] = np.float64(lam), np.float64(LAMBDA)
        out[f"mix{B}_total"], out[f"mix{B}_df"], out[f"mix{B}_dc"] = grads(total, f)
    np.savez_compressed(args.out, **{k: np.asarray(v) for k, v in out.items()})
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
