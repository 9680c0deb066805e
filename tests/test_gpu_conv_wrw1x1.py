"""Bit-exact tests of k_conv1x1_wrw, the 1x1 weight gradient for stride
1 and 2 (GPU).

Same method as test_gpu_conv_exact.py, whose helpers are reused:
operands on the dyadic grid {k/4 : |k| <= 8} make every partial sum
exact in fp32 while 16 * 4 * T < 2**24 (T = N * Ho * Wo terms, asserted),
so the kernel is compared with a float64 CPU reference by torch.equal.
A chunk is CP = 128 flattened output pixels; K and C tile as 128s plus
one 64 remainder.
"""

import pytest
import torch
import torch.nn.functional as F

from test_gpu_conv_exact import (_assert_exact, _assert_exact_bound, _cpu64,
                                 _dyadic, _Guarded, _trips, _zeros_cl)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from adaptdl_amd import ops

CP = 128    # W1_CP (conv_kernels.hip)


def _run_wrw1x1(x, dy, stride, prefill=None):
    """dw (K, C, 1, 1) from the kernel; with ``prefill`` (K*C floats) the
    accum path into a segment one float past a 16-byte boundary."""
    ext = ops._load_extension()
    n, c, h, w = x.shape
    k, ho, wo = dy.shape[1:]
    assert ext.conv1x1_wrw_ok(h, w, c, k, stride)
    nsplit = ext.conv1x1_wrw_nsplit(n, ho, wo, c, k)
    ws = _Guarded(nsplit * k * c, torch.float32)
    off = 0 if prefill is None else 1
    out = _Guarded(k * c + off, torch.float32)
    out.inner[:off] = 7.0
    seg = out.inner[off:]
    assert seg.data_ptr() % 16 == 4 * off
    x0, dy0 = x.clone(), dy.clone()
    if prefill is None:
        ext.conv1x1_wrw(x, dy, ws.inner, seg.view(k, c, 1, 1), stride)
    else:
        seg.copy_(prefill)
        ext.conv1x1_wrw(x, dy, ws.inner, seg, stride, True)
    torch.cuda.synchronize()
    ws.check("ws")       # every slab region written, nothing beyond
    out.check("dw")
    assert (out.inner[:off] == 7.0).all(), "wrote below the segment"
    assert torch.equal(x, x0) and torch.equal(dy, dy0), "inputs changed"
    return seg.view(k, c, 1, 1)


# (N, C, H, W, K, stride), chunks, nsplit, trips, reduce groups, accum
@pytest.mark.parametrize("shape,chunks,nsplit,trips,groups,accum", [
    ((3, 64, 5, 7, 64, 1), 1, 1, [1], 1, False),      # M=105 < CP, odd
    ((2, 128, 8, 8, 64, 1), 1, 1, [1], 1, False),     # 64k x 128c tile
    ((37, 64, 7, 7, 192, 1), 15, 15, [1], 1, False),  # K = 128 + 64, tail
    ((37, 64, 7, 7, 192, 1), 15, 15, [1], 1, True),   # unaligned accum
    ((130, 256, 14, 14, 64, 1), 200, 128, [2, 1], 8, False),  # atomics
    ((40, 512, 11, 11, 512, 1), 38, 16, [3, 2], 1, False),    # 128x128
    ((5, 64, 6, 10, 128, 2), 1, 1, [1], 1, False),    # Ho x Wo = 3x5
    ((33, 128, 8, 8, 256, 2), 5, 5, [1], 1, False),   # multi-chunk s2
])
def test_wrw1x1_exact(shape, chunks, nsplit, trips, groups, accum):
    n, c, h, w, k, s = shape
    ho, wo = h // s, w // s
    m = n * ho * wo
    _assert_exact_bound(m + 1)
    assert -(-m // CP) == chunks
    tiles = -(-k // 128) * -(-c // 128)
    mirrored = max(1, min(256 // tiles, chunks))
    got = ops._load_extension().conv1x1_wrw_nsplit(n, ho, wo, c, k)
    assert got == mirrored == nsplit, (got, mirrored)
    assert _trips(chunks, nsplit) == trips
    assert -(-nsplit // 16) == groups
    gen = torch.Generator().manual_seed(601)
    x, dy = _dyadic(gen, n, c, h, w), _dyadic(gen, n, k, ho, wo)
    ref = torch.nn.grad.conv2d_weight(
        _cpu64(x), (k, c, 1, 1), _cpu64(dy), stride=s)
    pre = None
    if accum:
        pre = (torch.randint(-8, 9, (k * c,), generator=gen).float() / 4) \
            .cuda()
        ref = ref + pre.double().cpu().view(k, c, 1, 1)
    dw = _run_wrw1x1(x, dy, s, pre)
    _assert_exact(dw, ref.float().cuda(), "conv1x1_wrw {}".format(shape))


@pytest.mark.parametrize("s,n0,h0,w0", [
    (1, 0, 0, 0),       # first pixel
    (1, 0, 5, 9),       # last pixel of an image
    (1, 2, 0, 7),       # p = 127: last pixel of chunk 0
    (1, 2, 0, 8),       # p = 128: first pixel of the tail chunk
    (1, 2, 5, 9),       # last pixel overall
    (2, 0, 0, 0),
    (2, 0, 2, 4),       # last output pixel of an image
    (2, 1, 1, 3),       # odd pixel of a staged pair, second image
    (2, 2, 2, 4),       # last output pixel overall
])
def test_wrw1x1_one_hot(s, n0, h0, w0):
    """dy = one 1.0 at (n0, k0, h0, w0): dw[k0, :] is the x pixel at
    (s*h0, s*w0) of image n0 and every other k row is zero."""
    n, c, h, w, k, k0 = 3, 64, 6, 10, 64, 37
    x = _dyadic(torch.Generator().manual_seed(602), n, c, h, w)
    dy = _zeros_cl(n, k, h // s, w // s)
    dy[n0, k0, h0, w0] = 1.0
    want = torch.zeros(k, c, 1, 1, device="cuda")
    want[k0, :, 0, 0] = x[n0, :, s * h0, s * w0].float()
    _assert_exact(_run_wrw1x1(x, dy, s), want,
                  "wrw1x1 one-hot s={} at ({}, {}, {})".format(s, n0, h0, w0))


@pytest.mark.parametrize("s", [1, 2])
def test_module_1x1_weight_grad_exact(s, monkeypatch):
    """FusedConv2d 1x1 with ADAPTDL_WRW_1X1=1: weight.grad comes from
    k_conv1x1_wrw (128k x 64c tile, 3 or 2 chunks) and must be exact; the
    library's forward and x.grad are held to test_gpu_conv_wrw4.py's
    tolerances.  ADAPTDL_WRW_1X1=0 forces the library path."""
    from adaptdl_amd.torch.layers import FusedConv2d
    n, c, h, w, k = 5, 64, 6, 10 * s, 128
    ho, wo = h // s, w // s
    _assert_exact_bound(n * ho * wo)
    conv = FusedConv2d(c, k, 1, stride=s, bias=False).to("cuda")
    gen = torch.Generator().manual_seed(603)
    with torch.no_grad():
        conv.weight.copy_(
            torch.randint(-8, 9, conv.weight.shape, generator=gen) / 4)
    x = _dyadic(gen, n, c, h, w).requires_grad_(True)
    dy = _dyadic(gen, n, k, ho, wo)
    monkeypatch.setenv("ADAPTDL_WRW_1X1", "0")
    assert not conv._wrw1x1_ok(x)
    monkeypatch.setenv("ADAPTDL_WRW_1X1", "1")
    assert conv._wrw1x1_ok(x)
    y = conv(x)
    y.backward(dy)

    x64, w64, dy64 = _cpu64(x), _cpu64(conv.weight), _cpu64(dy)
    assert conv.weight.grad.dtype == torch.float32
    _assert_exact(
        conv.weight.grad,
        torch.nn.grad.conv2d_weight(x64, w64.shape, dy64, stride=s)
        .float().cuda(), "FusedConv2d 1x1 s{} weight.grad".format(s))
    yr = F.conv2d(x64, w64, stride=s).float().cuda()
    assert torch.allclose(y.float(), yr, atol=0.2, rtol=5e-2)
    dxr = torch.nn.grad.conv2d_input(x64.shape, w64, dy64, stride=s)
    assert torch.allclose(x.grad.float(), dxr.float().cuda(),
                          atol=0.3, rtol=5e-2)
