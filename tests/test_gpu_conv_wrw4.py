"""Bit-exact tests of k_conv3x3_wrw_w4, the 3x3 weight gradient for 4x4
feature maps (GPU).

Same method as test_gpu_conv_exact.py, whose helpers are reused:
operands on the dyadic grid {k/4 : |k| <= 8} make every partial sum
exact in fp32 while 16 * 4 * T < 2**24 (T = N * 16 terms, asserted), so
the kernel is compared with a float64 CPU reference by torch.equal.
A chunk is W4_G = 8 whole images; one MFMA K step is an image pair.
"""

import pytest
import torch
import torch.nn.functional as F

from test_gpu_conv_exact import (_assert_exact, _assert_exact_bound, _cpu64,
                                 _dyadic, _dyadic_conv, _run_wrw, _trips,
                                 _zeros_cl)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from adaptdl_amd import ops

G = 8       # W4_G (conv_kernels.hip)


@pytest.mark.parametrize("shape,nsplit,trips,groups", [
    ((83, 512, 4, 4, 512), 4, [3, 2], 1),     # 11 chunks, tail of 3 images
    ((563, 64, 4, 4, 256), 64, [2, 1], 4),    # C != K; memset + atomics
    ((5, 64, 4, 4, 64), 1, [1], 1),           # N < G, odd
    ((1, 64, 4, 4, 64), 1, [1], 1),           # N = 1: half an image pair
    ((16, 128, 4, 4, 64), 2, [1], 1),         # N an exact multiple of G
])
def test_wrw4_exact(shape, nsplit, trips, groups):
    n, c, h, w, k = shape
    _assert_exact_bound(n * h * w)
    chunks = -(-n // G)
    mirrored = max(1, min(256 // ((k // 64) * (c // 64)), chunks))
    got = ops._load_extension().conv_wrw_nsplit(n, h, w, c, k)
    assert got == mirrored == nsplit, (got, mirrored)
    assert _trips(chunks, nsplit) == trips
    assert -(-nsplit // 16) == groups
    gen = torch.Generator().manual_seed(501)
    x, dy = _dyadic(gen, n, c, h, w), _dyadic(gen, n, k, h, w)
    dw = _run_wrw(x, dy)      # asserts conv_wrw_ok, guards, inputs
    ref = torch.nn.grad.conv2d_weight(
        _cpu64(x), (k, c, 3, 3), _cpu64(dy), stride=1, padding=1)
    _assert_exact(dw, ref.float().cuda(), "conv_wrw {}".format(shape))


@pytest.mark.parametrize("n0", [1, 2])
@pytest.mark.parametrize("h0,w0", [(i // 4, i % 4) for i in range(16)])
def test_wrw4_one_hot(h0, w0, n0):
    """dy = one 1.0 at (n0, k0, h0, w0): dw[k0, :, dh, dw] is the x pixel
    at (h0 + dh - 1, w0 + dw - 1) of image n0, zero outside the image,
    and every other k row is zero.  A failure pattern shows leakage
    between the two images of a K step (n0 is the second image of pair
    (0, 1), then the first of (2, 3)), a wrong halo line or a wrong
    alignbyte shift."""
    n, c, k, k0 = 4, 64, 64, 37
    x = _dyadic(torch.Generator().manual_seed(502), n, c, 4, 4)
    dy = _zeros_cl(n, k, 4, 4)
    dy[n0, k0, h0, w0] = 1.0
    want = torch.zeros(k, c, 3, 3, device="cuda")
    for dh in range(3):
        for dw in range(3):
            hh, ww = h0 + dh - 1, w0 + dw - 1
            if 0 <= hh < 4 and 0 <= ww < 4:
                want[k0, :, dh, dw] = x[n0, :, hh, ww].float()
    _assert_exact(_run_wrw(x, dy), want,
                  "wrw4 one-hot n0={} at ({}, {})".format(n0, h0, w0))


def test_module_w4_weight_grad_exact(monkeypatch):
    """FusedConv2d 3x3/s1 on 4x4 maps with ADAPTDL_WRW_W4=1: weight.grad
    comes from k_conv3x3_wrw_w4 (2 and 1 trips, odd tail) and must be
    exact; the library's forward and x.grad are held to
    test_fused_conv.py's tolerances.  ADAPTDL_WRW_W4=0 forces the
    library path."""
    n, c, h, w, k = 2051, 64, 4, 4, 64
    _assert_exact_bound(n * h * w)
    assert _trips(-(-n // G), 256) == [2, 1]
    conv, gen = _dyadic_conv(c, k, 1, seed=503)
    x = _dyadic(gen, n, c, h, w).requires_grad_(True)
    dy = _dyadic(gen, n, k, h, w)
    monkeypatch.setenv("ADAPTDL_WRW_W4", "0")
    assert not conv._wrw_ok(x)
    monkeypatch.setenv("ADAPTDL_WRW_W4", "1")
    assert conv._wrw_ok(x)
    y = conv(x)
    y.backward(dy)

    x64, w64, dy64 = _cpu64(x), _cpu64(conv.weight), _cpu64(dy)
    assert conv.weight.grad.dtype == torch.float32
    _assert_exact(
        conv.weight.grad,
        torch.nn.grad.conv2d_weight(x64, w64.shape, dy64, padding=1)
        .float().cuda(), "FusedConv2d 4x4 weight.grad")
    yr = F.conv2d(x64, w64, padding=1).float().cuda()
    assert torch.allclose(y.float(), yr, atol=0.2, rtol=5e-2)
    dxr = torch.nn.grad.conv2d_input(x64.shape, w64, dy64, padding=1)
    assert torch.allclose(x.grad.float(), dxr.float().cuda(),
                          atol=0.3, rtol=5e-2)
