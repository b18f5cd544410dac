"""Rounding-faithful fp64 restatement of the gated-attention kernels (csrc/attention.hip through radhip/ops.py:
rdx_attn_fwd, rdx_attn_bwd_fused, rdx_attn_bwd_fused_split, rdx_attn_bwd), forward AND backward, hand-written in
plain torch. TEST INFRASTRUCTURE, in the manner of oracle/head16.py.

    s[b,h,i,j] = scale q_i . k_j + gate[b,h,i] rel[h, j - i + T - 1]          P = softmax_j(s)
    mk = keep inv_keep     Pk = P mk     o = Pk v     lse = logsumexp_j(s)     D = rowsum(dO o)
    dP = dO v^T     dS = P (dP mk - D)     dq = scale dS k     dk = scale dS^T q     dv = Pk^T dO
    dgate = sum_j dS rel[h, j - i + T - 1]

Inputs are tensors [B, H, T, 64] (q, k, v, dO), [B, H, T] (gate), [H, 2T - 1] (rel) holding values the storage types
represent (16-bit q / k / v / dO, fp32 gate / rel, widened), `keep` a {0, 1} array [B, H, T, T] or None, and p the
dropout probability the kernels are given: inv_keep is 1 / (1 - p) as the host computes it in fp32.

`faithful=True` rounds to the storage type `dt` where the kernels do, as read from csrc/attention.hip:
  forward   Pu = exp(s - m_run) mk goes to 16 bits (pack8 of sv) before O^T += V^T Pu^T. m_run is the ONLINE maximum:
            the largest score of the row over the 32-key tiles swept so far. The key-split kernel (`fwd_split`) keeps
            one running maximum per half of the key tiles (the first ceil(nt / 2) tiles, the rest). The accumulators
            are rescaled in fp32 (alpha) to the final maximum, so o = sum_j Pu_ij exp(m_run - m) v_j / l.
            l = sum_j exp(s - m) is summed BEFORE the keep factor, in fp32 (here fp64, unrounded).
            o goes to 16 bits; lse = m + log l stays fp32.
  backward  D = rowsum(dO o) from the ROUNDED o, in fp32.
            Pk = exp(s - lse) mk goes to 16 bits before dv = Pk^T dO (normalised here: the backward has no running max).
            dS goes to 16 bits before dq = dS k and dk = dS^T q. dq, dk (after the scale) and dv go to 16 bits.
            dgate sums the 16-bit dS on the fused routes (phase 2 reads the dS image) and the fp32 dS on the dQ + dK/dV
            pair (`dgate16`).
With `faithful=False` it is the plain formula (equal to autograd, tests/test_attn_ref_cpu.py). `work` is the type the
arithmetic runs in: float64 for the reference; float32 on the device gives the 16-bit torch restatement of the same
roundings that tests/test_attn_edges_gpu.py measures its faithful-tier constants on.

Beside each result the dict carries, in fp64 terms of the same run, the sum of the magnitudes of the terms of the
contraction that produced each element (A_o = sum_j |Pk_ij| |v_jd|, A_dv, A_dq, A_dk, A_dgate, A_D), the same sums with
dS replaced by its uncancelled size G = P (mk |dO|.|v| + A_D) (F_dq, F_dk, F_dgate: the scale of dS's fp32 errors), the
weights a D error reaches each result with (W_dq = scale sum_j P |k|, W_dgate = sum_j P |rel|; dk's is formed in
`tolerances_plain` as it needs D's tolerance per row), and the plain sums of the other operand (S_v, S_do, S_k, S_q, S_rel:
what an absolute, subnormal rounding error of P or dS is multiplied by).

`mutate` names one deliberate error (MUTATIONS); tests/test_attn_ref_cpu.py checks that each exceeds the criterion.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle.head16 import EPS, identity, ulp

TILE = 32
SCALE = 0.125
U32 = 2.0 ** -24                                                          # unit roundoff of fp32
ETA = {torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25}           # half the subnormal spacing
MUTATIONS = ["mask_last_key", "tab_pos", "tab_neg", "gate_last", "keep_flip", "l_after_keep", "no_D", "swap_heads"]
RES16 = ["o", "dq", "dk", "dv"]
RES32 = ["lse", "D", "dgate"]


def inv_keep(p):
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p))) if p > 0 else 1.0


def fwd_is_split(B, T, H):
    """rdx_attn_fwd's choice: the key-split kernel while the unsplit grid has at most 512 workgroups."""
    nt = (T + TILE - 1) // TILE
    return B * H * ((nt + 3) // 4) <= 512


def rel_matrix(rel, T):
    """[H, 2T - 1] table -> bias [H, T(query), T(key)]."""
    i = torch.arange(T, device=rel.device)
    return rel[:, i[None, :] - i[:, None] + T - 1]


def mutation_applies(name, B, T, H, p, st="plain"):
    """Whether a mutation changes anything a test could see on a case of input set `st`."""
    if name in ("gate_last", "mask_last_key"):
        return T >= 2              # one key: nothing to take the gate from, no key left
    if name in ("keep_flip", "l_after_keep"):
        return p > 0 and T > 2
    if name == "swap_heads":
        return H >= 16
    if name == "tab_neg":
        return T >= 2              # at T = 1 both ends are the one entry d = 0, which tab_pos zeroes
    return True


def _run_max(s, split):
    """Online maximum of each row at each key: over the 32-key tiles up to the key's own, per half when split."""
    T = s.shape[-1]
    nt = (T + TILE - 1) // TILE
    tm = F.pad(s, (0, nt * TILE - T), value=float("-inf")).unflatten(-1, (nt, TILE)).amax(-1)
    kmid = (nt + 1) // 2 if split else nt
    run = tm[..., :kmid].cummax(-1).values
    if kmid < nt:
        run = torch.cat([run, tm[..., kmid:].cummax(-1).values], -1)
    return run.repeat_interleave(TILE, -1)[..., :T]


def reference(q, k, v, gate, rel, keep, p, do, dt, faithful=True, fwd_split=False, dgate16=True,
              work=torch.float64, mutate=None):
    rnd = (lambda x: x.to(dt).to(work)) if faithful else identity
    q, k, v, do, gate, rel = (x.to(work) for x in (q, k, v, do, gate, rel))
    B, H, T, _ = q.shape
    ik = inv_keep(p)
    if mutate == "tab_pos":
        rel = rel.clone()
        rel[:, 2 * T - 2] = 0
    if mutate == "tab_neg":
        rel = rel.clone()
        rel[:, 0] = 0
    if mutate == "gate_last":
        gate = gate.clone()
        gate[..., T - 1] = gate[..., T - 2]
    pb = rel_matrix(rel, T)                                                # [H, T, T]
    s = SCALE * (q @ k.transpose(-1, -2)) + gate[..., None] * pb[None]
    if keep is not None and mutate == "keep_flip":                         # in the row that weighs the last key most
        keep = keep.clone()
        j0, row = 2 * ((T - 1) // 2), int(torch.softmax(s[0, 0], -1)[:, T - 1].argmax())
        keep[0, 0, row, j0:] = 1 - keep[0, 0, row, j0:]
    if mutate == "mask_last_key":
        s = s.clone()
        s[..., T - 1] = float("-inf")
    mk = torch.full_like(s, 1.0) if keep is None else keep.to(work) * ik
    m = s.amax(-1, keepdim=True)
    e = torch.exp(s - m)
    l = (e * mk if mutate == "l_after_keep" else e).sum(-1, keepdim=True)
    lse = (m + torch.log(l)).squeeze(-1)
    P = e / l
    # ---- forward
    if faithful:
        mr = _run_max(s, fwd_split)
        o = rnd(((rnd(torch.exp(s - mr) * mk) * torch.exp(mr - m)) @ v) / l)
    else:
        o = (P * mk) @ v
    # ---- backward
    Pk = rnd(P * mk)
    D = (do * o).sum(-1)
    dP = do @ v.transpose(-1, -2)
    dS = P * (dP * mk - (0.0 if mutate == "no_D" else D[..., None]))
    dS16 = rnd(dS)
    out = {"T": T, "o": o, "lse": lse, "D": D,
           "dq": rnd(SCALE * (dS16 @ k)), "dk": rnd(SCALE * (dS16.transpose(-1, -2) @ q)),
           "dv": rnd(Pk.transpose(-1, -2) @ do),
           "dgate": ((dS16 if dgate16 else dS) * pb[None]).sum(-1)}
    if mutate == "swap_heads":
        perm = torch.arange(H)
        perm[:8], perm[8:16] = torch.arange(8, 16), torch.arange(8)
        out = {n: (x[:, perm] if torch.is_tensor(x) else x) for n, x in out.items()}
    if work != torch.float64:
        return out
    # ---- magnitude sums (fp64 only)
    aq, ak, av, ado, apb = q.abs(), k.abs(), v.abs(), do.abs(), pb.abs()[None]
    Pm = P * mk
    A_D = (ado * o.abs()).sum(-1)
    G = P * (mk * (ado @ av.transpose(-1, -2)) + A_D[..., None])
    aS = dS.abs()
    out.update({
        "A_o": Pm @ av, "A_dv": Pm.transpose(-1, -2) @ ado, "A_D": A_D,
        "A_dq": SCALE * (aS @ ak), "A_dk": SCALE * (aS.transpose(-1, -2) @ aq), "A_dgate": (aS * apb).sum(-1),
        "F_dq": SCALE * (G @ ak), "F_dk": SCALE * (G.transpose(-1, -2) @ aq), "F_dgate": (G * apb).sum(-1),
        "W_dq": SCALE * (P @ ak), "W_dgate": (P * apb).sum(-1), "P": P,
        "S_v": av.sum(-2, keepdim=True).expand_as(v), "S_do": ado.sum(-2, keepdim=True).expand_as(v),
        "S_k": SCALE * ak.sum(-2, keepdim=True).expand_as(v), "S_q": SCALE * aq.sum(-2, keepdim=True).expand_as(v),
        "S_rel": apb.sum(-1).expand(B, H, T), "aq": aq,
        # what one-ulp flips of o (the kernel's own o feeds its D) reach dq and dk with: dD_i <= sum_d |dO| ulp(o)
        "E_dq": (ado * ulp(o, dt)).sum(-1)[..., None] * (SCALE * (P @ ak)),
        "E_dk": SCALE * ((P * (ado * ulp(o, dt)).sum(-1)[..., None]).transpose(-1, -2) @ aq),
        "sqk": float((SCALE * (aq @ ak.transpose(-1, -2))).max()), "sb": float((gate.abs()[..., None] * apb).max()),
    })
    return out


def rho(ref):
    """Relative fp32 error of one probability exp(s - lse) (also the absolute error of lse), in the worst case:
    s = fma(S, scale log2e, gate log2e rel) with S an fp32 sum of 64 exact products: (64 + 2) u sqk + 4 u sb, where
    sqk = max scale sum_d |q||k| and sb = max |gate rel|; lse inherits the largest such error of its row, the fp32 sum
    of T terms (T u), one hardware exp2 per term and one log2 (one ulp = 2 u each) and its own storage and the
    base-2 conversions, 4 u (sqk + sb + log T); the exponent s - lse is formed in fp32 at that size once more."""
    T = ref["T"]
    return U32 * (2 * (66 * ref["sqk"] + 4 * ref["sb"]) + 8 * (ref["sqk"] + ref["sb"] + math.log(T)) + T + 8)


def tolerances_plain(ref, do, dt):
    """The plain-tier bound of every result (dict of fp64 tensors shaped like the results)."""
    T = ref["T"]
    eps, eta, r = EPS[dt], ETA[dt], rho(ref)
    acc = (T + 66) * U32
    t = {"lse": torch.full_like(ref["lse"], r)}
    t["o"] = (eps + r + acc) * ref["A_o"] + eta * ref["S_v"] + ulp(ref["o"], dt)
    t["dv"] = (eps + r + acc) * ref["A_dv"] + eta * ref["S_do"] + ulp(ref["dv"], dt)
    t["D"] = (do.abs() * t["o"]).sum(-1) + 66 * U32 * ref["A_D"]
    tD = t["D"][..., None]
    P = ref["P"]
    t["dq"] = eps * ref["A_dq"] + (r + acc) * ref["F_dq"] + tD * ref["W_dq"] + eta * ref["S_k"] + ulp(ref["dq"], dt)
    t["dk"] = (eps * ref["A_dk"] + (r + acc) * ref["F_dk"] + SCALE * ((P * tD).transpose(-1, -2) @ ref["aq"])
               + eta * ref["S_q"] + ulp(ref["dk"], dt))
    t["dgate"] = (eps * ref["A_dgate"] + (r + acc) * ref["F_dgate"] + t["D"] * ref["W_dgate"] + eta * ref["S_rel"])
    return t


def fp32_rel(ref):
    """rho plus an fp32 sum's own error: the relative size of the fp32 errors of a contraction's terms."""
    return rho(ref) + (ref["T"] + 66) * U32


def slack_faithful(ref, n):
    """The derived part of the faithful tier beside K eps A + ulp(ref): the fp32 term of the plain tier, fp32_rel F
    (where dS cancels - at T = 1 it is exactly zero and so is A; a near one-hot row's dP mk - D - the fp32 residue of D
    and dP, at the size F of the uncancelled terms, is no rounding flip; for o and dv F = A), and for dq and dk what
    one-ulp flips of o put into D: the kernel forms D from its own o, so every dS_ij of a row moves by P_ij dD_i with
    dD_i <= sum_d |dO_id| ulp(o_id) (E_dq, E_dk)."""
    A = ref["A_" + n]
    return fp32_rel(ref) * ref.get("F_" + n, A) + ref.get("E_" + n, 0.0)


def dist_faithful(got, ref, n, dt):
    """The K result `n` needs against the faithful reference `ref`: the max over every element of
    (|got - ref| - ulp(ref) - slack_faithful)+ / (eps A). Where no term was added (A == 0) anything beyond the spacing
    and the slack is infinitely far."""
    A = ref["A_" + n]
    d = ((got - ref[n]).abs() - ulp(ref[n], dt) - slack_faithful(ref, n)).clamp_min(0.0)
    x = torch.where(A > 0, d / (EPS[dt] * A).clamp_min(1e-300),
                    torch.where(d == 0, torch.zeros_like(d), torch.full_like(d, float("inf"))))
    return float(x.max())
