"""Which custom autograd ops Residual_block.forward takes, per block kind and per switch (radhip/sinc.py).

One forward of each of the encoder's four block kinds ([1, 32] first, [32, 32], [32, 64], [64, 64]) on a tiny NHWC
input (N = 2, H = 4, W = 9 and W = 3), in eval() under bf16 autocast; the names of the custom autograd nodes reachable
from y.grad_fn are held against a literal table: the default, every switch off on its own, two pairs of block-0
switches, fp32 (no autocast) and bn2 in training mode. W = 2 (no pool window at all) is rejected by rdx_res_tail_fwd's
own check in every route, so the narrow edge of the table is W = 3, the smallest width of tests/test_sconv_pool_gpu.py,
and W = 2 is held to that rejection.

The table was recorded from Residual_block.forward's if-ladder before the routing was separated from the execution.
The only difference to that record: the two ops ResBlockIdentity and ResBlockDown were merged into ResBlock
(one op with an optional downsample weight), so both names read ResBlock here."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
N, H = 2, 4
KINDS = {"b0": ([1, 32], True), "i32": ([32, 32], False), "dn": ([32, 64], False), "i64": ([64, 64], False)}
SWITCHES = ("RADHIP_B0X", "RADHIP_FUSED_B0", "RADHIP_B0_FWD", "RADHIP_SCONV_PAIR", "RADHIP_RES_FUSED",
            "RADHIP_SCONV_POOL", "RADHIP_SCONV", "RADHIP_B0X_BWD", "RADHIP_FUSED_DGRAD_BN")

RB = {"ResBlock"}
UNPAIRED = {"SConvBnSelu", "SConv", "ResTail"}
TORCH_CONVS = {"BnSelu", "ResTail"}                  # both convolutions on torch's conv2d
DEFAULT = {"b0": {"Block0Fused"}, "i32": RB, "dn": RB, "i64": RB}
BF16 = torch.bfloat16

# row -> (environment, autocast dtype or None, bn2.training, {kind: names})
ROWS = {
    "default": ({}, BF16, False, DEFAULT),
    "B0X=0": ({"RADHIP_B0X": "0"}, BF16, False, {**DEFAULT, "b0": {"Block0Front", "ResTail"}}),
    "FUSED_B0=0": ({"RADHIP_FUSED_B0": "0"}, BF16, False, DEFAULT),
    "B0_FWD=0": ({"RADHIP_B0_FWD": "0"}, BF16, False, DEFAULT),
    "SCONV_PAIR=0": ({"RADHIP_SCONV_PAIR": "0"}, BF16, False,
                     {"b0": {"Block0Convs", "BnSelu", "SConv", "ResTail"}, "i32": UNPAIRED, "dn": UNPAIRED,
                      "i64": UNPAIRED}),
    "RES_FUSED=0": ({"RADHIP_RES_FUSED": "0"}, BF16, False,
                    {"b0": {"Block0Fused"}, "i32": {"SConvBnSeluSConv", "ResTail"},
                     "dn": {"SConvBnSeluSConv", "SConv", "ResTail"}, "i64": {"SConvBnSeluSConv", "ResTail"}}),
    "SCONV_POOL=0": ({"RADHIP_SCONV_POOL": "0"}, BF16, False,
                     {**DEFAULT, "dn": {"SConvBnSeluSConv", "SConv", "ResTail"}}),
    "SCONV_POOL=fwd": ({"RADHIP_SCONV_POOL": "fwd"}, BF16, False, DEFAULT),
    "SCONV_POOL=bwd": ({"RADHIP_SCONV_POOL": "bwd"}, BF16, False, DEFAULT),
    "SCONV=0": ({"RADHIP_SCONV": "0"}, BF16, False,
                {"b0": {"Block0Convs", "BnSelu", "ResTail"}, "i32": TORCH_CONVS, "dn": TORCH_CONVS,
                 "i64": TORCH_CONVS}),
    "B0X=0,B0_FWD=0": ({"RADHIP_B0X": "0", "RADHIP_B0_FWD": "0"}, BF16, False,
                       {**DEFAULT, "b0": {"Block0Convs", "BnSeluSConv", "ResTail"}}),
    "B0X=0,FUSED_B0=0": ({"RADHIP_B0X": "0", "RADHIP_FUSED_B0": "0"}, BF16, False,
                         {**DEFAULT, "b0": {"BnSelu", "SConv", "ResTail"}}),
    "fp32": ({}, None, False, {k: TORCH_CONVS for k in KINDS}),
    "bn2 training": ({}, BF16, True, {k: set() for k in KINDS}),
}


def custom_nodes(y):
    """Names of the torch.autograd.Function nodes reachable from y.grad_fn (without the Backward suffix)."""
    names, seen, todo = set(), set(), [y.grad_fn]
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        if isinstance(fn, torch.autograd.function.BackwardCFunction):
            names.add(type(fn).__name__.removesuffix("Backward"))
        todo.extend(f for f, _ in fn.next_functions)
    return names


def block_input(ci, W):
    """fp32 [N, ci, H, W] in the channels_last form SincNetEncoder.forward hands to its encoder."""
    x = torch.randn(N, ci, H, W, generator=torch.Generator().manual_seed(ci + W)).to(DEV)
    if ci == 1:
        return x.as_strided((N, 1, H, W), (H * W, 1, W, 1))
    return x.contiguous(memory_format=torch.channels_last)


def route(kind, W, env, amp, bn2_training, monkeypatch):
    from radhip.sinc import Residual_block
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    filts, first = KINDS[kind]
    torch.manual_seed(0)
    blk = Residual_block(filts, first=first).to(DEV).eval()
    blk.bn2.train(bn2_training)
    x = block_input(filts[0], W)
    with torch.autocast("cuda", dtype=amp or torch.bfloat16, enabled=amp is not None):
        y = blk(x)
    assert y.shape == (N, filts[1], H, W // 3)
    return custom_nodes(y)


@pytest.mark.parametrize("W", [9, 3])
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("row", list(ROWS))
def test_residual_block_routing(row, kind, W, monkeypatch):
    env, amp, bn2_training, table = ROWS[row]
    got = route(kind, W, env, amp, bn2_training, monkeypatch)
    print(f"routing {row!r} {kind} W={W}: {sorted(got)}")
    assert got == table[kind]


@pytest.mark.parametrize("kind", list(KINDS))
def test_no_pool_window_reaches_the_tail_kernel(kind, monkeypatch):
    """W = 2: no route takes a kernel with the pool in its epilogue (Block0Fused, rdx_sconv_fwd_pool); every block
    comes to rdx_res_tail_fwd, whose own check (W >= 3) rejects the shape."""
    with pytest.raises(RuntimeError, match="radhip res_tail_fwd failed"):
        route(kind, 2, {}, BF16, False, monkeypatch)
