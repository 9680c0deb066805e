"""Bit-exact tests of the MFMA conv kernels on dyadic inputs (GPU).

All operands are drawn from the dyadic grid {k/4 : |k| <= 8}, which is
exact in bf16.  Every product is then a multiple of 1/16 of magnitude
<= 4, and every partial sum of T products, in ANY order, is a multiple
of 1/16 below 4*T -- exactly representable in fp32 while
16 * 4 * T < 2**24.  Under that condition (asserted per test) the
result does not depend on accumulation order, split count or atomics,
and the kernels in adaptdl_amd/ops/hip/conv_kernels.hip are compared
with a float64 CPU reference by torch.equal:

  - fp32 outputs (conv_wrw) must equal the reference exactly,
  - bf16 outputs (conv_mm, conv_s2_bwd) must equal the reference
    rounded ONCE to bf16 (RNE); the grid yields many exact ties, so
    truncation or round-half-up fails.

The shapes are the smallest that make each kernel's software pipeline
run more than one chunk per block (trip counts asserted from a mirror
of the launcher formulas), plus tail chunks, padded widths, C != K and
the minimum sizes.  Every output is carved out of a larger sentinel
buffer: the guards must stay untouched, no sentinel may survive inside
the output, and the inputs must come back unchanged.
"""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from adaptdl_amd import ops
    assert ops.has_extension(), \
        "HIP extension must be built+importable on a GPU box"

GUARD = 256                 # guard elements on each side (multiple of 64)
BF16_SENTINEL = 0x5A5B      # bf16 bits of ~1.5e13: not a grid result


def _dyadic(gen, n, c, h, w):
    """(n, c, h, w) channels_last bf16 GPU tensor on the dyadic grid."""
    v = torch.randint(-8, 9, (n, h, w, c), generator=gen).float() / 4
    return v.to(torch.bfloat16).cuda().permute(0, 3, 1, 2)


def _zeros_cl(n, c, h, w):
    return torch.zeros(n, h, w, c, dtype=torch.bfloat16,
                       device="cuda").permute(0, 3, 1, 2)


def _cpu64(t):
    return t.detach().double().cpu()


def _assert_exact_bound(terms):
    """16 * 4 * T < 2**24: every partial sum is exact in fp32."""
    assert 16 * 4 * terms < 2 ** 24, terms


def _trips(chunks, stride):
    """Distinct per-block loop trip counts when block s of `stride`
    takes chunks s, s + stride, ... (largest first)."""
    return sorted({len(range(s, chunks, stride)) for s in range(stride)},
                  reverse=True)


class _Guarded:
    """An output carved out of a sentinel-filled buffer."""

    def __init__(self, numel, dtype):
        self.flat = torch.empty(numel + 2 * GUARD, dtype=dtype,
                                device="cuda")
        if dtype == torch.float32:
            self.flat.fill_(float("nan"))
            self.bits = self.flat.view(torch.int32)
        else:
            self.bits = self.flat.view(torch.int16)
            self.bits.fill_(BF16_SENTINEL)
        self.before = self.bits.clone()
        self.inner = self.flat[GUARD:GUARD + numel]

    def check(self, what):
        assert torch.equal(self.bits[:GUARD], self.before[:GUARD]), \
            what + ": wrote below its output"
        assert torch.equal(self.bits[-GUARD:], self.before[-GUARD:]), \
            what + ": wrote past its output"
        left = (self.bits[GUARD:-GUARD] == self.before[0]).sum().item()
        assert left == 0, \
            "{}: {} elements were never written".format(what, left)


def _assert_exact(got, want, what):
    """torch.equal, with a report that shows the PATTERN of a failure
    (one chunk's pixels, one tap, one tile) so it can be diagnosed from
    the log."""
    assert got.shape == want.shape and got.dtype == want.dtype
    if torch.equal(got, want):
        return
    idx = (got != want).nonzero()        # NaN != anything
    spans = ["dim{}: {} distinct in [{}, {}]".format(
        d, idx[:, d].unique().numel(), idx[:, d].min().item(),
        idx[:, d].max().item()) for d in range(idx.shape[1])]
    first = ["{} got {!r} want {!r}".format(
        tuple(i.tolist()), got[tuple(i.tolist())].item(),
        want[tuple(i.tolist())].item()) for i in idx[:8]]
    pytest.fail("{}: {} of {} elements differ ({}); first: {}".format(
        what, idx.shape[0], got.numel(), ", ".join(spans),
        "; ".join(first)))


# ---- conv_wrw -----------------------------------------------------------

def _wrw_params(w, small=False):
    """Mirror of conv3x3_wrw_params (conv_kernels.hip): (P, Wp)."""
    return {8: (8, 8), 16: (8, 16), 32: (4, 32), 56: (1, 64),
            28: (4, 32), 14: (2 if small else 8, 16),
            7: (4 if small else 8, 8)}[w]


def _wrw_nsplit(n, c, h, w, k, small=False):
    """Mirror of conv3x3_wrw_nsplit: (chunks, nsplit)."""
    p, _ = _wrw_params(w, small)
    chunks = n * -(-h // p)
    return chunks, max(1, min(256 // ((k // 64) * (c // 64)), chunks))


def _run_wrw(x, dy):
    ext = ops._load_extension()
    n, c, h, w = x.shape
    k = dy.shape[1]
    assert ext.conv_wrw_ok(n, h, w, c, k)
    nsplit = ext.conv_wrw_nsplit(n, h, w, c, k)
    ws = _Guarded(nsplit * k * 9 * c, torch.float32)
    out = _Guarded(k * 9 * c, torch.float32)
    dw = out.inner.view(k, 3, 3, c).permute(0, 3, 1, 2)
    x0, dy0 = x.clone(), dy.clone()
    ext.conv_wrw(x, dy, ws.inner, dw)
    torch.cuda.synchronize()
    ws.check("ws")       # every slab region written, nothing beyond
    out.check("dw")      # overwritten, or zeroed before the atomic reduce
    assert torch.equal(x, x0) and torch.equal(dy, dy0), "inputs changed"
    return dw


def _wrw_exact(shape, seed):
    n, c, h, w, k = shape
    _assert_exact_bound(n * h * w)
    gen = torch.Generator().manual_seed(seed)
    x, dy = _dyadic(gen, n, c, h, w), _dyadic(gen, n, k, h, w)
    dw = _run_wrw(x, dy)
    ref = torch.nn.grad.conv2d_weight(
        _cpu64(x), (k, c, 3, 3), _cpu64(dy), stride=1, padding=1)
    _assert_exact(dw, ref.float().cuda(), "conv_wrw {}".format(shape))


@pytest.mark.parametrize("shape,nsplit,trips,groups", [
    ((11, 512, 8, 8, 512), 4, [3, 2], 1),     # 64 tiles, trips 3,3,3,2
    ((40, 256, 8, 8, 256), 16, [3, 2], 1),
    ((70, 64, 8, 16, 256), 64, [2, 1], 4),    # C != K; memset + atomics
    ((150, 128, 7, 7, 128), 64, [3, 2], 4),   # padded width + tail lines
    ((5, 64, 56, 56, 64), 256, [2, 1], 16),   # Wp=64, P=1
    ((3, 64, 6, 32, 64), 6, [1], 1),          # H % P != 0, non-square
    ((2, 64, 2, 8, 64), 2, [1], 1),           # minimum H: mostly tail
    ((1, 64, 16, 16, 64), 2, [1], 1),         # N = 1
])
def test_wrw_exact(shape, nsplit, trips, groups):
    n, c, h, w, k = shape
    chunks, mirrored = _wrw_nsplit(n, c, h, w, k)
    got = ops._load_extension().conv_wrw_nsplit(n, h, w, c, k)
    assert got == mirrored == nsplit, (got, mirrored)
    assert _trips(chunks, nsplit) == trips
    # launch_conv3x3_wrw reduces in groups of 16 slabs; more than one
    # group takes the memset + atomicAdd path
    assert -(-nsplit // 16) == groups
    _wrw_exact(shape, seed=101)


@pytest.mark.parametrize("shape,nsplit", [
    ((2, 64, 14, 14, 64), 14),     # P=2: 7 exact-cover chunks per image
    ((2, 64, 7, 7, 64), 4),        # P=4: 2 chunks per image, 1 tail line
])
def test_wrw_exact_smallchunk(shape, nsplit, monkeypatch):
    monkeypatch.setenv("ADAPTDL_WRW_SMALLCHUNK", "1")
    n, c, h, w, k = shape
    chunks, mirrored = _wrw_nsplit(n, c, h, w, k, small=True)
    got = ops._load_extension().conv_wrw_nsplit(n, h, w, c, k)
    assert got == mirrored == nsplit == chunks, (got, mirrored, chunks)
    _wrw_exact(shape, seed=102)


@pytest.mark.parametrize("h,w", [(7, 7), (14, 14), (28, 28), (56, 56),
                                 (6, 32), (16, 16)])
def test_wrw_one_hot(h, w):
    """dy = one 1.0 at (n0, k0, h0, w0): dw[k0, :, dh, dw] is the x pixel
    at (h0 + dh - 1, w0 + dw - 1), zero outside the image, and every
    other k row is zero.  The corners include the last real column of
    the padded widths and the last line of the tail chunks."""
    n, c, k, n0, k0 = 2, 64, 64, 1, 37
    p, wp = _wrw_params(w)
    if (h, w) in ((7, 7), (14, 14), (6, 32)):
        assert h % p, "wants a tail chunk"
    if w in (7, 14, 28, 56):
        assert wp > w, "wants a padded width"
    x = _dyadic(torch.Generator().manual_seed(103), n, c, h, w)
    for h0, w0 in [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1),
                   (h // 2, w // 2)]:
        dy = _zeros_cl(n, k, h, w)
        dy[n0, k0, h0, w0] = 1.0
        want = torch.zeros(k, c, 3, 3, device="cuda")
        for dh in range(3):
            for dw in range(3):
                hh, ww = h0 + dh - 1, w0 + dw - 1
                if 0 <= hh < h and 0 <= ww < w:
                    want[k0, :, dh, dw] = x[n0, :, hh, ww].float()
        _assert_exact(_run_wrw(x, dy), want,
                      "wrw one-hot {}x{} at ({}, {})".format(h, w, h0, w0))


# ---- conv_s2_bwd (Wo = 16 and the Wo = 8 variant) -----------------------

def _s2_spread(n, c, ho, wo):
    """Mirror of launch_conv3x3_s2_bwd: (chunks, spread)."""
    ct = 16 if wo == 8 else 32          # S2W8_CT / S2_CT
    chunks = n * (ho // 2)              # S2_P2 = 2 phase rows per chunk
    return chunks, max(1, min(256 // (c // ct), chunks))


def _run_s2_bwd(dy, w, c):
    """w: (K, C, 3, 3) bf16; returns dx (N, C, 2Ho, 2Wo)."""
    ext = ops._load_extension()
    n, k, ho, wo = dy.shape
    assert ext.conv_s2_bwd_ok(n, ho, wo, k, c)
    wt = w.permute(1, 2, 3, 0).contiguous()
    out = _Guarded(n * 2 * ho * 2 * wo * c, torch.bfloat16)
    dx = out.inner.view(n, 2 * ho, 2 * wo, c).permute(0, 3, 1, 2)
    dy0, wt0 = dy.clone(), wt.clone()
    ext.conv_s2_bwd(dy, wt, dx)
    torch.cuda.synchronize()
    out.check("dx")
    assert torch.equal(dy, dy0) and torch.equal(wt, wt0), "inputs changed"
    return dx


@pytest.mark.parametrize("shape,spread,trips", [
    ((40, 256, 4, 16, 128), 32, [3, 2]),      # 8 c-tiles, 80 chunks
    ((3, 96, 6, 16, 128), 9, [1]),            # 3 c-tiles, 3 chunks/image
    ((2, 32, 2, 16, 64), 2, [1]),             # minimum Ho, K=64
    ((20, 128, 8, 8, 128), 32, [3, 2]),       # Wo=8 k-split variant
    ((2, 48, 2, 8, 256), 2, [1]),             # Wo=8, K=256
])
def test_s2_bwd_exact(shape, spread, trips):
    n, c, ho, wo, k = shape
    _assert_exact_bound(4 * k)
    chunks, mirrored = _s2_spread(n, c, ho, wo)
    assert mirrored == spread and _trips(chunks, spread) == trips
    gen = torch.Generator().manual_seed(201)
    dy = _dyadic(gen, n, k, ho, wo)
    w = _dyadic(gen, k, c, 3, 3).contiguous()
    dx = _run_s2_bwd(dy, w, c)
    ref = torch.nn.grad.conv2d_input(
        (n, c, 2 * ho, 2 * wo), _cpu64(w), _cpu64(dy), stride=2, padding=1)
    _assert_exact(dx, ref.to(torch.bfloat16).cuda(),
                  "conv_s2_bwd {}".format(shape))


@pytest.mark.parametrize("ho,wo,k", [(4, 16, 64), (4, 8, 128)])
def test_s2_bwd_one_hot(ho, wo, k):
    """dy = one 1.0 at (n0, k0, ho0, wo0): dx is the weight taps of k0
    scattered to (2 ho0 + dh - 1, 2 wo0 + dw - 1), zero elsewhere."""
    n, c, n0, k0 = 2, 32, 1, 21
    w = _dyadic(torch.Generator().manual_seed(202), k, c, 3, 3).contiguous()
    for ho0, wo0 in [(0, 0), (ho - 1, wo - 1)]:
        dy = _zeros_cl(n, k, ho, wo)
        dy[n0, k0, ho0, wo0] = 1.0
        want = _zeros_cl(n, c, 2 * ho, 2 * wo)
        for dh in range(3):
            for dw in range(3):
                hi, wi = 2 * ho0 + dh - 1, 2 * wo0 + dw - 1
                if 0 <= hi < 2 * ho and 0 <= wi < 2 * wo:
                    want[n0, :, hi, wi] = w[k0, :, dh, dw]
        _assert_exact(_run_s2_bwd(dy, w, c), want,
                      "s2_bwd one-hot Wo={} at ({}, {})".format(
                          wo, ho0, wo0))


# ---- conv_mm ------------------------------------------------------------

def _mm_plan(n, c, h, w, k):
    """Mirror of launch_conv3x3_mm: (chunks, spread, dbuf)."""
    p = 4 if w == 32 else 8
    kt = 64 if c <= 64 else 32
    chunks = n * (h // p)
    spread = max(1, min(256 // (k // kt), chunks))
    lds2 = (kt * 9 * (c + 8) + 2 * (p + 2) * (w + 2) * (c + 16)) * 2
    return chunks, spread, int(lds2 <= 160 * 1024)


def _run_conv_mm(x, w):
    ext = ops._load_extension()
    n, c, h, wd = x.shape
    k = w.shape[0]
    assert ext.conv_mm_ok(n, h, wd, c, k)
    out = _Guarded(n * h * wd * k, torch.bfloat16)
    y = out.inner.view(n, h, wd, k).permute(0, 3, 1, 2)
    x0, w0 = x.clone(), w.clone()
    ext.conv_mm(x, w, y)
    torch.cuda.synchronize()
    out.check("y")
    assert torch.equal(x, x0) and torch.equal(w, w0), "inputs changed"
    return y


@pytest.mark.parametrize("shape,spread,trips,dbuf", [
    ((150, 64, 8, 16, 256), 64, [3, 2], 1),   # two LDS x windows
    # two windows would need > 160 KB: one window, register prefetch
    ((150, 128, 8, 16, 128), 64, [3, 2], 0),
    ((2, 96, 4, 32, 64), 2, [1], 1),          # C % 64 != 0, KT=32, W=32
])
def test_conv_mm_exact(shape, spread, trips, dbuf):
    n, c, h, w, k = shape
    _assert_exact_bound(9 * c)
    chunks, mirrored, mirrored_dbuf = _mm_plan(n, c, h, w, k)
    assert mirrored == spread and _trips(chunks, spread) == trips
    assert mirrored_dbuf == dbuf
    gen = torch.Generator().manual_seed(301)
    x, wt = _dyadic(gen, n, c, h, w), _dyadic(gen, k, c, 3, 3)
    y = _run_conv_mm(x, wt)
    ref = F.conv2d(_cpu64(x), _cpu64(wt), padding=1)
    _assert_exact(y, ref.to(torch.bfloat16).cuda(),
                  "conv_mm {}".format(shape))


def test_conv_mm_one_hot():
    """x = one 1.0 at (n0, c0, h0, w0): y[n0, :, h0 - dh + 1,
    w0 - dw + 1] is the weight tap w[:, c0, dh, dw], zero elsewhere."""
    n, c, h, w, k, n0, c0 = 2, 64, 8, 16, 64, 1, 13
    wt = _dyadic(torch.Generator().manual_seed(302), k, c, 3, 3)
    for h0, w0 in [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)]:
        x = _zeros_cl(n, c, h, w)
        x[n0, c0, h0, w0] = 1.0
        want = _zeros_cl(n, k, h, w)
        for dh in range(3):
            for dw in range(3):
                hh, ww = h0 - dh + 1, w0 - dw + 1
                if 0 <= hh < h and 0 <= ww < w:
                    want[n0, :, hh, ww] = wt[:, c0, dh, dw]
        _assert_exact(_run_conv_mm(x, wt), want,
                      "conv_mm one-hot at ({}, {})".format(h0, w0))


def test_conv_mm_rejects_window_past_prefetch_registers():
    """C=128 at W=32 needs 6 b128 pieces per thread for the x window;
    mm_issue holds 5, so the predicate must refuse it."""
    ext = ops._load_extension()
    assert (4 + 2) * 32 * (128 // 8) > 5 * 512
    assert not ext.conv_mm_ok(2, 4, 32, 128, 64)
    assert (4 + 2) * 32 * (96 // 8) <= 5 * 512
    assert ext.conv_mm_ok(2, 4, 32, 96, 64)


# ---- FusedConv2d --------------------------------------------------------

def _dyadic_conv(cin, cout, stride, seed):
    from adaptdl_amd.torch.layers import FusedConv2d
    conv = FusedConv2d(cin, cout, 3, stride=stride, padding=1,
                       bias=False).to("cuda")
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        conv.weight.copy_(
            torch.randint(-8, 9, conv.weight.shape, generator=gen) / 4)
    return conv, gen


def test_module_stride1_weight_grad_exact():
    """FusedConv2d 3x3/s1: weight.grad comes from k_conv3x3_wrw running
    2 and 1 trips per block and must be exact; the library's forward
    and x.grad are held to test_fused_conv.py's tolerances."""
    n, c, h, w, k = 300, 64, 8, 8, 64
    _assert_exact_bound(n * h * w)
    chunks, nsplit = _wrw_nsplit(n, c, h, w, k)
    assert nsplit == 256 and _trips(chunks, nsplit) == [2, 1]
    conv, gen = _dyadic_conv(c, k, 1, seed=401)
    x = _dyadic(gen, n, c, h, w).requires_grad_(True)
    dy = _dyadic(gen, n, k, h, w)
    assert conv._wrw_ok(x)
    y = conv(x)
    y.backward(dy)

    x64, w64, dy64 = _cpu64(x), _cpu64(conv.weight), _cpu64(dy)
    assert conv.weight.grad.dtype == torch.float32
    _assert_exact(
        conv.weight.grad,
        torch.nn.grad.conv2d_weight(x64, w64.shape, dy64, padding=1)
        .float().cuda(), "FusedConv2d s1 weight.grad")
    yr = F.conv2d(x64, w64, padding=1).float().cuda()
    assert torch.allclose(y.float(), yr, atol=0.2, rtol=5e-2)
    dxr = torch.nn.grad.conv2d_input(x64.shape, w64, dy64, padding=1)
    assert torch.allclose(x.grad.float(), dxr.float().cuda(),
                          atol=0.3, rtol=5e-2)


def test_module_stride2_input_grad_exact():
    """FusedConv2d 3x3/s2: x.grad comes from k_conv3x3_s2_bwd and must
    be exact; the library's forward and weight.grad are held to
    test_fused_conv.py's tolerances."""
    n, c, h, w, k = 2, 64, 32, 32, 128
    _assert_exact_bound(4 * k)
    conv, gen = _dyadic_conv(c, k, 2, seed=402)
    x = _dyadic(gen, n, c, h, w).requires_grad_(True)
    dy = _dyadic(gen, n, k, h // 2, w // 2)
    assert conv._s2_ok(x)
    y = conv(x)
    assert y.shape == (n, k, h // 2, w // 2)
    y.backward(dy)

    x64, w64, dy64 = _cpu64(x), _cpu64(conv.weight), _cpu64(dy)
    dxr = torch.nn.grad.conv2d_input(x64.shape, w64, dy64, stride=2,
                                     padding=1)
    _assert_exact(x.grad, dxr.to(torch.bfloat16).cuda(),
                  "FusedConv2d s2 x.grad")
    yr = F.conv2d(x64, w64, stride=2, padding=1).float().cuda()
    assert torch.allclose(y.float(), yr, atol=0.2, rtol=5e-2)
    dwr = torch.nn.grad.conv2d_weight(x64, w64.shape, dy64, stride=2,
                                      padding=1)
    assert torch.allclose(conv.weight.grad.float(), dwr.float().cuda(),
                          atol=0.3, rtol=5e-2)
