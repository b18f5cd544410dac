"""Host side of the x3 SincNet stream (radhip/sinc_x3.py, csrc/sconv_x3.hip) without a device: the two entry points
exist in both libraries with ctypes signatures, their argument checks return before any HIP call, the weight
re-layout keeps what the kernel reads, and a CPU tensor never takes the stream."""
import ctypes

import torch

from radhip import _lib, sinc_x3, wavlm_x3

NAMES = ("rdx_x3_b0x_fwd", "rdx_x3_sconv_fwd")


def test_both_libraries_export_the_entry_points():
    declared = _lib.header_symbols()
    for name in NAMES:
        assert name in declared, f"{name} is not declared in include/radhip.h"
        assert name in _lib.SIGNATURES
        assert hasattr(_lib.lib(), name) and hasattr(_lib.lib16(), name)


def test_argument_checks_return_before_device_work():
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    p += (-p) % 16
    # null pointers
    assert L.rdx_x3_sconv_fwd(None, p, p, None, p, 1, 3, 8, 32, 32, 2, 1, None) == -1
    assert L.rdx_x3_sconv_fwd(p, None, p, None, p, 1, 3, 8, 32, 32, 2, 1, None) == -1
    assert L.rdx_x3_sconv_fwd(p, p, p, None, None, 1, 3, 8, 32, 32, 2, 1, None) == -1
    assert L.rdx_x3_b0x_fwd(None, None, p, p, p, p, p, p, p, 1, 3, 8, None) == -1
    assert L.rdx_x3_b0x_fwd(p, None, p, p, p, p, None, p, p, 1, 3, 8, None) == -1
    # shapes the kernels are not built for
    assert L.rdx_x3_sconv_fwd(p, p, p, None, p, 1, 3, 8, 48, 32, 2, 1, None) == -2
    assert L.rdx_x3_sconv_fwd(p, p, p, None, p, 1, 3, 8, 32, 48, 2, 1, None) == -2
    assert L.rdx_x3_sconv_fwd(p, p, p, None, p, 1, 3, 8, 32, 32, 3, 1, None) == -2
    assert L.rdx_x3_sconv_fwd(p, p, p, None, p, 1, 1, 8, 32, 32, 2, 0, None) == -2     # H < kh - ph: no output row
    assert L.rdx_x3_b0x_fwd(p, None, p, p, p, p, p, p, p, 1, 3, 2, None) == -2          # W < 3
    # the fp16 library exports the names and refuses the call
    assert _lib.lib16().rdx_x3_sconv_fwd(p, p, p, None, p, 1, 3, 8, 32, 32, 2, 1, None) == -1


def test_planes_of_the_tap_major_layout_reproduce_the_weight():
    g = torch.Generator().manual_seed(3)
    for co, ci, kh in ((32, 32, 2), (64, 32, 1), (64, 64, 2)):
        w = torch.randn(co, ci, kh, 3, generator=g) / (kh * 3 * ci) ** 0.5
        t = sinc_x3.tap_major(w)
        assert t.shape == (kh * 3, co, ci) and t.is_contiguous()
        hi, lo = wavlm_x3.planes(t)
        assert hi.dtype == lo.dtype == torch.bfloat16 and hi.is_contiguous() and lo.is_contiguous()
        back = hi.double() + lo.double()
        # the kernel reads plane element [r * 3 + s][o][c] for weight [o][c][r][s]
        for r in range(kh):
            for s in range(3):
                want = w[:, :, r, s].double()
                assert float(((back[r * 3 + s] - want).abs() - 2.0 ** -17 * want.abs()).max()) <= 0.0


def test_a_cpu_tensor_is_not_eligible():
    from radhip.sinc import SincNetEncoder
    enc = SincNetEncoder().eval()
    assert sinc_x3.standard_layout(enc)
    with torch.no_grad(), wavlm_x3.scoring():
        assert not sinc_x3.eligible(enc, torch.zeros(2, 2400), False)
    assert min(sinc_x3.widths(enc, 2400)) == 3 and min(sinc_x3.widths(enc, 2300)) == 2
