"""The residual blocks' max-pool without the full-width tensors (csrc/sconv.hip: rdx_sconv_fwd_pool and the
pooled-gradient variants of the three backward kernels) against the kernels they replace.

Forward: rdx_sconv_fwd_pool == rdx_sconv_fwd followed by rdx_res_tail_fwd, bit for bit (pooled values and window
index bytes). Backward: each kernel fed the pooled gradient (dy, arg) == the same kernel fed rdx_res_tail_bwd's
full-width scatter, bit for bit for everything a deterministic reduction produces (dc, dx, dW); the fp32-atomic
channel sums (the bias gradient, the BN sums) are held to an fp64 sum with the bound
test_kernels_gpu.test_fused_residual_block_matches_torch applies (rtol 1e-4, atol 1e-5 of the tensor's scale).
Block 2's conv_downsample gradients likewise. Ops level: Residual_block with RADHIP_SCONV_POOL = 1 / fwd / bwd against 0,
with the launches recorded by name. Widths: W % 3 in {0, 1, 2}, one partial strip, and seams of the 128-position strips (plain kernels) and of the
120-position strips (pooled epilogue). Both 16-bit storage types (libradhip.so bf16, libradhip_f16.so fp16)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
WS = (3, 5, 127, 128, 130, 253, 379)
N = 2
DTYPES = [torch.bfloat16, torch.float16]


def _nhwc(t):
    return t.contiguous(memory_format=torch.channels_last)


def _rand(gen, shape, dtype, scale=1.0):
    return _nhwc((torch.randn(shape, generator=gen) * scale).to(dtype).to(DEV))


def _bits(t):
    return t.contiguous().view(torch.int16)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _atomic_close(got, ref64, what):
    scale = ref64.abs().max().item() + 1e-6
    torch.testing.assert_close(got.double().cpu() / scale, ref64.cpu() / scale, rtol=1e-4, atol=1e-5, msg=what)


def _conv(x, w, ci, co, kh, ph):
    from radhip.ops import _sconv_run
    return _sconv_run(x, w, ci, co, kh, ph)


def _tail_fwd(a, idn, bias):
    from radhip.ops import _L, _dtype_code, _p, _stream, check
    n, c, h, w = a.shape
    y = torch.empty(n, c, h, w // 3, device=DEV, dtype=a.dtype, memory_format=torch.channels_last)
    arg = torch.empty(n, c, h, w // 3, device=DEV, dtype=torch.uint8, memory_format=torch.channels_last)
    check(_L(a).rdx_res_tail_fwd(_dtype_code(a), _p(a), _p(idn), _p(bias), _p(y), _p(arg), n * h, w, c, _stream(a)),
          "res_tail_fwd")
    return y, arg


def _tail_bwd(dy, arg, W):
    from radhip.ops import _L, _dtype_code, _p, _stream, check
    n, c, h, _ = dy.shape
    ds = torch.empty(n, c, h, W, device=DEV, dtype=dy.dtype, memory_format=torch.channels_last)
    dbias = torch.zeros(c, device=DEV, dtype=torch.float32)
    check(_L(dy).rdx_res_tail_bwd(_dtype_code(dy), _p(dy), _p(arg), _p(ds), _p(dbias), n * h, W, c, _stream(dy)),
          "res_tail_bwd")
    return ds, dbias


def _check_forward(x, w, idn, bias, c):
    from radhip.ops import _sconv_run_pool
    y0, a0 = _tail_fwd(_conv(x, w, c, c, 2, 0), idn, bias)
    y1, a1 = _sconv_run_pool(x, w, idn, bias, c)
    W = x.shape[3]
    assert _same_bits(y1, y0), f"y differs at W={W}"
    assert torch.equal(a1, a0), f"arg differs at W={W}"
    return y0, a0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [32, 64])
@pytest.mark.parametrize("H", [1, 3])
def test_pooled_forward_matches_conv_then_tail(dtype, C, H):
    gen = torch.Generator().manual_seed(100 * C + H)
    w = (torch.randn(6, C, C, generator=gen) * 0.1).to(dtype).to(DEV)
    bias = (torch.randn(C, generator=gen) * 0.1).to(DEV)
    for W in WS:
        x = _rand(gen, (N, C, H + 1, W), dtype)
        idn = _rand(gen, (N, C, H, W), dtype)
        _check_forward(x, w, idn, bias, C)


@pytest.mark.parametrize("dtype", DTYPES)
def test_pooled_forward_identity_from_downsample_conv(dtype):
    """Block 2: the identity is conv_downsample's output (32 -> 64 channels, 1 x 3), conv2 is 64 -> 64."""
    gen = torch.Generator().manual_seed(7)
    H, W = 3, 253
    x0 = _rand(gen, (N, 32, H, W), dtype)
    wd = (torch.randn(3, 64, 32, generator=gen) * 0.1).to(dtype).to(DEV)
    idn = _conv(x0, wd, 32, 64, 1, 0)
    assert idn.shape == (N, 64, H, W)
    x = _rand(gen, (N, 64, H + 1, W), dtype)
    w = (torch.randn(6, 64, 64, generator=gen) * 0.1).to(dtype).to(DEV)
    bias = (torch.randn(64, generator=gen) * 0.1).to(DEV)
    _check_forward(x, w, idn, bias, 64)


@pytest.mark.parametrize("dtype", DTYPES)
def test_pooled_forward_first_maximum_wins(dtype):
    """Small-integer inputs: every sum is exact, so pool windows hold equal values and the first of them must win."""
    gen = torch.Generator().manual_seed(11)
    C, H, W = 32, 3, 130
    x = _nhwc(torch.randint(-1, 2, (N, C, H + 1, W), generator=gen).to(dtype).to(DEV))
    w = torch.randint(-1, 2, (6, C, C), generator=gen).to(dtype).to(DEV)
    w[:, :, 4:] = 0                      # four input channels: |conv| <= 24, exact in both 16-bit types
    idn = _nhwc(torch.randint(-1, 2, (N, C, H, W), generator=gen).to(dtype).to(DEV))
    bias = torch.randint(-1, 2, (C,), generator=gen).float().to(DEV)
    y, arg = _check_forward(x, w, idn, bias, C)
    s = (_conv(x, w, C, C, 2, 0).float() + idn.float() + bias.view(1, C, 1, 1))[..., :W // 3 * 3]
    s = s.reshape(N, C, H, W // 3, 3)
    top = s.max(-1, keepdim=True).values
    assert ((s == top).sum(-1) > 1).sum().item() >= 100      # of 8256 windows: the tie rule is exercised
    first = (s == top).float().argmax(-1)                                  # index of the first maximum
    assert torch.equal(arg.long(), first)
    assert torch.equal(y.float(), top.squeeze(-1))


@pytest.mark.parametrize("dtype", DTYPES)
def test_pooled_forward_propagates_nan(dtype):
    gen = torch.Generator().manual_seed(13)
    C, H, W = 64, 1, 128
    x = _rand(gen, (N, C, H + 1, W), dtype)
    idn = _rand(gen, (N, C, H, W), dtype)
    for k, col in enumerate((0, 31, 62, 119, 121, 125)):     # each place in a window, both sides of a strip seam
        idn[k % N, (5 * k) % C, 0, col] = float("nan")
    x[1, 3, 1, 90] = float("nan")                             # through the convolution: a whole neighbourhood
    w = (torch.randn(6, C, C, generator=gen) * 0.1).to(dtype).to(DEV)
    bias = (torch.randn(C, generator=gen) * 0.1).to(DEV)
    y, arg = _check_forward(x, w, idn, bias, C)
    assert torch.isnan(y[0, 0, 0, 0]) and arg[0, 0, 0, 0] == 0
    assert torch.isnan(y[1, 5, 0, 31 // 3]) and arg[1, 5, 0, 31 // 3] == 31 % 3
    assert torch.isnan(y[1, :, 0, 30]).all()


def _bn5(gen, C):
    cb = torch.randn(C, generator=gen) * 0.1
    mean = torch.randn(C, generator=gen) * 0.1
    invstd = 1.0 / torch.sqrt(torch.rand(C, generator=gen) + 0.5)
    gamma = 1 + torch.randn(C, generator=gen) * 0.1
    beta = torch.randn(C, generator=gen) * 0.1
    return torch.stack([cb, mean, invstd * gamma, beta, invstd]).contiguous().to(DEV)


def _bnselu_sums64(do1, c, bn5):
    """The three channel sums of the frozen BN + SELU backward (d conv bias, d gamma, d beta) in fp64."""
    cb, mean, sg, beta, invstd = [t.double().view(1, -1, 1, 1) for t in bn5]
    zc = (c.double() + cb) - mean
    u = zc * sg + beta
    sd = torch.where(u > 0, torch.full_like(u, 1.0507009873554805),
                     1.0507009873554805 * 1.6732632423543772 * torch.exp(u))
    du = do1.double() * sd
    return torch.stack([(du * sg).sum((0, 2, 3)), (du * zc * invstd).sum((0, 2, 3)), du.sum((0, 2, 3))])


def _check_backward(gen, dtype, C, H, W, arg):
    from radhip.ops import _L, _p, _sconv_run, _sconv_run_res_pool, _sconv_wgrad_pool, _stream, check, lib
    Wo = W // 3
    dy = _rand(gen, (N, C, H, Wo), dtype)
    arg = _nhwc(arg.to(DEV))
    ds, dbias0 = _tail_bwd(dy, arg, W)
    wd2 = (torch.randn(6, C, C, generator=gen) * 0.1).to(dtype).to(DEV)
    wd1 = (torch.randn(6, C, C, generator=gen) * 0.1).to(dtype).to(DEV)
    c = _rand(gen, (N, C, H + 1, W), dtype)
    out1 = _rand(gen, (N, C, H + 1, W), dtype)
    bn5 = _bn5(gen, C)
    L = _L(dy)
    # conv2's input gradient through the BN + SELU backward
    dc0, dc1 = torch.empty_like(c), torch.empty_like(c)
    s0 = torch.zeros(3, C, device=DEV)
    s1 = torch.zeros(3, C, device=DEV)
    check(L.rdx_sconv_dgrad_bnselu(_p(ds), _p(wd2), _p(c), _p(dc0), _p(bn5), _p(s0), N, H, W, C, C, 2, 1,
                                   _stream(ds)), "sconv_dgrad_bnselu")
    check(L.rdx_sconv_dgrad_bnselu_pool(_p(dy), _p(arg), _p(wd2), _p(c), _p(dc1), _p(bn5), _p(s1), N, H, W, C, C, 2, 1,
                                        _stream(dy)), "sconv_dgrad_bnselu_pool")
    assert _same_bits(dc1, dc0), f"dc differs at W={W}"
    ref = _bnselu_sums64(_sconv_run(ds, wd2, C, C, 2, 1), c, bn5)
    for q, nm in enumerate(("d conv1.bias", "d gamma", "d beta")):
        _atomic_close(s1[q], ref[q], f"{nm} at W={W}")
    # conv2's weight gradient
    nblk = lib().rdx_sconv_wgrad_nblk(N, H, W)
    part = torch.empty(nblk, 6 * C * C, device=DEV)
    dw0 = torch.empty(6, C, C, device=DEV)
    check(L.rdx_sconv_wgrad(_p(out1), _p(ds), _p(dw0), _p(part), N, H + 1, W, C, C, 2, 0, _stream(ds)), "sconv_wgrad")
    dw1 = _sconv_wgrad_pool(out1, dy, arg, (C, C, 2, 3))
    assert torch.equal(dw1, dw0.view(2, 3, C, C).permute(2, 3, 0, 1)), f"dW differs at W={W}"
    # the block input's gradient: conv1's input gradient + the identity branch's
    dx0 = _sconv_run(dc0, wd1, C, C, 2, 0, res=ds)
    dbias1 = torch.zeros(C, device=DEV)
    dx1 = _sconv_run_res_pool(dc0, wd1, dy, arg, dbias1, C, C, 2, 0)
    assert _same_bits(dx1, dx0), f"dx differs at W={W}"
    _atomic_close(dbias1, dy.double().sum((0, 2, 3)), f"d bias at W={W}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [32, 64])
@pytest.mark.parametrize("H", [1, 3])
def test_pooled_gradient_variants_match_scatter_then_kernel(dtype, C, H):
    gen = torch.Generator().manual_seed(1000 * C + H)
    for W in WS:
        _check_backward(gen, dtype, C, H, W, torch.randint(0, 3, (N, C, H, W // 3), generator=gen, dtype=torch.uint8))
    for v in (0, 2):
        _check_backward(gen, dtype, C, H, 130, torch.full((N, C, H, 130 // 3), v, dtype=torch.uint8))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H", [1, 3])
def test_pooled_gradient_through_conv_downsample(dtype, H):
    """Block 2's identity branch: conv_downsample's (1 x 3, 32 -> 64) input and weight gradients from the pooled
    gradient == the same from rdx_res_tail_bwd's scatter, bit for bit."""
    from radhip.ops import _L, _p, _sconv_dgrad_pool, _sconv_run, _sconv_wgrad_pool, _stream, check, lib
    gen = torch.Generator().manual_seed(77 + H)
    sd = (64, 32, 1, 3)
    wdd = (torch.randn(3, 32, 64, generator=gen) * 0.1).to(dtype).to(DEV)      # the flipped kernel [3][ci][co]
    draws = [(W, None) for W in WS] + [(130, 0), (130, 2)]
    for W, fill in draws:
        Wo = W // 3
        dy = _rand(gen, (N, 64, H, Wo), dtype)
        arg = (torch.randint(0, 3, (N, 64, H, Wo), generator=gen, dtype=torch.uint8) if fill is None
               else torch.full((N, 64, H, Wo), fill, dtype=torch.uint8))
        arg = _nhwc(arg.to(DEV))
        x = _rand(gen, (N, 32, H, W), dtype)
        ds, _ = _tail_bwd(dy, arg, W)
        dx0 = _sconv_run(ds, wdd, 64, 32, 1, 0)
        dx1 = _sconv_dgrad_pool(dy, arg, wdd, sd, W)
        assert _same_bits(dx1, dx0), f"dx differs at W={W}"
        nblk = lib().rdx_sconv_wgrad_nblk(N, H, W)
        part = torch.empty(nblk, 3 * 64 * 32, device=DEV)
        dw0 = torch.empty(3, 64, 32, device=DEV)
        check(_L(dy).rdx_sconv_wgrad(_p(x), _p(ds), _p(dw0), _p(part), N, H, W, 32, 64, 1, 0, _stream(ds)), "sconv_wgrad")
        dw1 = _sconv_wgrad_pool(x, dy, arg, sd)
        assert torch.equal(dw1, dw0.view(1, 3, 64, 32).permute(2, 3, 0, 1)), f"dW differs at W={W}"


# launches of the pooled path and of the kernels it replaces, by the name radhip.ops.check reports them under
POOLED_FWD = {"sconv_fwd_pool"}
POOLED_BWD = {"sconv_dgrad_bnselu_pool", "sconv_wgrad_pool"}
TAILS = {"res_tail_fwd", "res_tail_bwd"}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("switch", ["1", "fwd", "bwd"])
@pytest.mark.parametrize("filts", [[32, 32], [64, 64], [32, 64]])
def test_residual_block_same_with_and_without_the_pooled_path(dtype, switch, filts, monkeypatch):
    """Residual_block under autocast (radhip.ops.ResBlock, with the downsample weight for block 2) with
    RADHIP_SCONV_POOL = 1 / fwd / bwd against 0: the same output and gradients, bit for bit except the fp32 channel
    sums; and the launches really are the pooled ones (no tail kernel on the half that is switched on)."""
    import radhip.ops as ops
    from radhip.sinc import Residual_block
    calls = []
    real_check = ops.check

    def recording_check(rc, what):
        calls.append(what)
        return real_check(rc, what)

    monkeypatch.setattr(ops, "check", recording_check)
    torch.manual_seed(filts[0] + filts[1])
    blk = Residual_block(filts).cuda()
    with torch.no_grad():
        blk.bn2.running_mean.normal_(0, 0.2)
        blk.bn2.running_var.uniform_(0.5, 2.0)
        blk.bn2.weight.normal_(1, 0.2)
        blk.bn2.bias.normal_(0, 0.2)
        blk.conv2.bias.normal_(0, 0.1)
    blk.eval()
    gen = torch.Generator().manual_seed(3)
    H, W = 3, 253
    x0 = _rand(gen, (N, filts[0], H, W), dtype)
    dy = _rand(gen, (N, filts[1], H, W // 3), dtype)

    def run(value):
        monkeypatch.setenv("RADHIP_SCONV_POOL", value)
        del calls[:]
        for p in blk.parameters():
            p.grad = None
        x = x0.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=dtype):
            y = blk(x)
        y.backward(dy)
        return (y.detach(), x.grad.detach().clone(), {n: p.grad.clone() for n, p in blk.named_parameters()
                                                      if p.grad is not None}, set(calls))

    y0, dx0, g0, c0 = run("0")
    y1, dx1, g1, c1 = run(switch)
    assert TAILS <= c0 and not (c0 & (POOLED_FWD | POOLED_BWD))
    down = filts[0] != filts[1]
    bwd_extra = {"sconv_dgrad_pool"} if down else {"sconv_fwd_res_pool"}
    if switch in ("1", "fwd"):
        assert POOLED_FWD <= c1 and "res_tail_fwd" not in c1
    else:
        assert "res_tail_fwd" in c1 and not (c1 & POOLED_FWD)
    if switch in ("1", "bwd"):
        assert (POOLED_BWD | bwd_extra) <= c1 and "res_tail_bwd" not in c1
    else:
        assert "res_tail_bwd" in c1 and not (c1 & (POOLED_BWD | bwd_extra))
    assert _same_bits(y1, y0)
    assert _same_bits(dx1, dx0)
    assert g1.keys() == g0.keys()
    for k in g0:
        if k in ("conv1.bias", "bn2.weight", "bn2.bias", "conv2.bias", "conv_downsample.bias"):
            scale = g0[k].abs().max().item() + 1e-6     # fp32 channel sums: equal to their summation order
            torch.testing.assert_close(g1[k] / scale, g0[k] / scale, rtol=1e-4, atol=1e-5, msg=k)
        else:
            assert torch.equal(g1[k], g0[k]), k


def test_unaligned_pool_gradient_falls_back(monkeypatch):
    """A pool gradient that is an offset view (not 16-byte aligned) takes the full-width path, as before."""
    import radhip.ops as ops
    calls = []
    real_check = ops.check
    monkeypatch.setattr(ops, "check", lambda rc, what: (calls.append(what), real_check(rc, what))[1])
    monkeypatch.setenv("RADHIP_SCONV_POOL", "1")
    from radhip.sinc import Residual_block
    torch.manual_seed(5)
    blk = Residual_block([32, 32]).cuda().eval()
    gen = torch.Generator().manual_seed(9)
    H, W = 1, 15
    x = _rand(gen, (N, 32, H, W), torch.bfloat16).requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = blk(x)
    flat = torch.randn(y.numel() + 4, generator=gen).to(torch.bfloat16).to(DEV)
    dy = flat[4:].as_strided(y.shape, y.stride())          # 8 bytes past an aligned address, y's NHWC strides
    assert dy.data_ptr() % 16 != 0
    y.backward(dy)
    assert "res_tail_bwd" in calls and "sconv_wgrad_pool" not in calls
    assert torch.isfinite(x.grad.float()).all()
