"""Fused BN tail kernels and the saved ReLU bitmask.

Goes through FusedBatchNormAct2d and compares with torch.nn.BatchNorm2d
in fp32 on the same bf16 values, at the tolerances of test_fused_bn.py.
Shapes reach every path of bn_kernels.hip: one row, idle threads
(slots=3), two partly filled reduce blocks, rpb=4, a second grid-stride
trip of the capped reduce (1024 blocks, all four row-sum trips of the
tail kernels) and apply (2048 blocks) grids, and rpb=1 with 256 slots.
"""

import pytest
import torch
import torch.nn.functional as F

from adaptdl_amd import ops
from adaptdl_amd.torch import layers as L
from adaptdl_amd.torch.layers import FusedBatchNormAct2d

pytestmark = pytest.mark.gpu

SHAPES = [(1, 8, 1, 1), (2, 24, 3, 5), (5, 64, 3, 3), (16, 512, 4, 4),
          (36, 512, 16, 16), (3, 2048, 2, 3)]


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _bf16(shape, gen, scale=1.0, shift=0.0):
    t = torch.randn(*shape, device="cuda", generator=gen) * scale + shift
    return _cl(t.to(torch.bfloat16))


def _ref_forward(ref, x32):
    """torch.nn.BatchNorm2d in fp32.  With one value per channel the
    module's Python-side size check refuses training mode, so that case
    calls the same ATen op the module calls, without the check."""
    if x32.numel() // x32.shape[1] > 1:
        return ref(x32)
    return torch.batch_norm(x32, ref.weight, ref.bias, ref.running_mean,
                            ref.running_var, True, ref.momentum, ref.eps,
                            False)


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_forward_backward_matches_batchnorm(shape, relu, residual):
    gen = torch.Generator(device="cuda").manual_seed(11)
    n, c, h, w = shape
    m = n * h * w
    bn = FusedBatchNormAct2d(c, relu=relu).cuda()
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.normal_()
    ref = torch.nn.BatchNorm2d(c).cuda()
    ref.load_state_dict(bn.state_dict())

    x = _bf16(shape, gen, 2.0, 0.5).requires_grad_(True)
    z = _bf16(shape, gen).requires_grad_(True) if residual else None
    x32 = x.detach().float().requires_grad_(True)
    z32 = z.detach().float().requires_grad_(True) if residual else None

    y = bn(x, residual=z)
    assert y.dtype == torch.bfloat16
    yr = _ref_forward(ref, x32)
    if residual:
        yr = yr + z32
    if relu:
        yr = F.relu(yr)
    assert torch.allclose(y.float(), yr, atol=5e-2, rtol=5e-2)

    # the reference gets the same bf16 gradient values, in fp32
    dy16 = _bf16(shape, gen)
    y.backward(dy16)
    yr.backward(dy16.float())
    assert torch.allclose(x.grad.float(), x32.grad, atol=7e-2, rtol=7e-2)
    if residual:
        assert torch.allclose(z.grad.float(), z32.grad,
                              atol=7e-2, rtol=7e-2)
        # dL/dz is the masked dy itself: exact, whatever the path.
        expect = torch.where(y > 0, dy16, torch.zeros_like(dy16)) \
            if relu else dy16
        assert torch.equal(z.grad, expect)
    assert torch.allclose(bn.weight.grad, ref.weight.grad,
                          atol=2e-1, rtol=2e-2)
    assert torch.allclose(bn.bias.grad, ref.bias.grad, atol=2e-1, rtol=2e-2)
    assert torch.allclose(bn.running_mean, ref.running_mean,
                          atol=2e-2, rtol=1e-2)
    if m > 1:
        assert torch.allclose(bn.running_var, ref.running_var,
                              atol=2e-2, rtol=1e-2)
    else:
        # The unbiased variance of one sample is 0/0 in the reference;
        # the kernel documents the biased value (0) for m == 1.
        assert torch.allclose(bn.running_var,
                              torch.full_like(bn.running_var, 0.9),
                              atol=1e-6, rtol=0)
    assert int(bn.num_batches_tracked) == 1


def _small_input(gen, c=64):
    return _bf16((4, c, 5, 5), gen, 2.0, 0.5)


def test_batch_counter_and_running_stats():
    gen = torch.Generator(device="cuda").manual_seed(12)
    bn = FusedBatchNormAct2d(64, relu=True).cuda()
    ref = torch.nn.BatchNorm2d(64).cuda()
    for step in range(1, 4):
        x = _small_input(gen)
        bn(x)
        ref(x.float())
        assert int(bn.num_batches_tracked) == step
    assert int(ref.num_batches_tracked) == 3
    assert bn.num_batches_tracked.dtype == torch.int64
    assert torch.allclose(bn.running_mean, ref.running_mean,
                          atol=2e-2, rtol=1e-2)
    assert torch.allclose(bn.running_var, ref.running_var,
                          atol=2e-2, rtol=1e-2)
    # under no_grad the training forward still counts
    with torch.no_grad():
        bn(_small_input(gen))
    assert int(bn.num_batches_tracked) == 4
    bn.eval()
    bn(_small_input(gen))
    assert int(bn.num_batches_tracked) == 4


def test_batch_counter_absent_without_running_stats():
    gen = torch.Generator(device="cuda").manual_seed(13)
    bn = FusedBatchNormAct2d(64, relu=True,
                             track_running_stats=False).cuda()
    assert bn.num_batches_tracked is None
    x = _small_input(gen)
    y = bn(x)
    yr = F.relu(F.batch_norm(x.float(), None, None, bn.weight, bn.bias,
                             True, 0.1, bn.eps))
    assert torch.allclose(y.float(), yr, atol=5e-2, rtol=5e-2)
    assert bn.num_batches_tracked is None and bn.running_mean is None


class _SpyExt:
    """Forwards to the extension and keeps the arguments of bn_fwd."""

    def __init__(self, ext):
        self._ext = ext
        self.fwd_args = []

    def __getattr__(self, name):
        return getattr(self._ext, name)

    def bn_fwd(self, *args):
        self.fwd_args.append(args)
        return self._ext.bn_fwd(*args)


def _masks(args):
    return [a for a in args
            if torch.is_tensor(a) and a.dtype == torch.uint8]


def test_no_mask_without_backward(monkeypatch):
    gen = torch.Generator(device="cuda").manual_seed(14)
    spy = _SpyExt(ops._load_extension())
    monkeypatch.setattr(L.ops, "_load_extension", lambda: spy)
    bn = FusedBatchNormAct2d(64, relu=True).cuda()
    x = _small_input(gen).requires_grad_(True)
    z = _small_input(gen).requires_grad_(True)

    # backward to follow: mask of M*C/8 bytes, residual not kept
    y_grad = bn(x, residual=z)
    (mask,) = _masks(spy.fwd_args[-1])
    assert mask.numel() == x.numel() // 8
    saved = y_grad.grad_fn.saved_tensors
    assert any(t.dtype == torch.uint8 and t.numel() == x.numel() // 8
               for t in saved)
    assert not any(t.data_ptr() == z.data_ptr() for t in saved
                   if t.numel() > 0)
    # bit k of byte [row * C/8 + slot] <=> y[row, slot*8+k] > 0
    rows = y_grad.detach().permute(0, 2, 3, 1).reshape(-1, 8, 8) > 0
    bits = (rows.to(torch.int32) <<
            torch.arange(8, device="cuda", dtype=torch.int32)).sum(-1)
    assert torch.equal(mask.view(-1, 8).to(torch.int32), bits)

    # same batch statistics, no grad: same y, no mask
    with torch.no_grad():
        y_nograd = bn(x, residual=z)
    (mask,) = _masks(spy.fwd_args[-1])
    assert mask.numel() == 0
    assert y_nograd.grad_fn is None
    assert torch.equal(y_nograd, y_grad.detach())

    # inputs that need no gradient: no mask either
    bn.requires_grad_(False)
    bn(x.detach(), residual=z.detach())
    (mask,) = _masks(spy.fwd_args[-1])
    assert mask.numel() == 0

    # eval: no mask, y matches the reference
    bn.eval()
    y_eval = bn(x.detach(), residual=z.detach())
    (mask,) = _masks(spy.fwd_args[-1])
    assert mask.numel() == 0
    ref = torch.nn.BatchNorm2d(64).cuda()
    ref.load_state_dict(bn.state_dict())
    ref.eval()
    yr = F.relu(ref(x.detach().float()) + z.detach().float())
    assert torch.allclose(y_eval.float(), yr, atol=5e-2, rtol=5e-2)


def test_non_residual_relu_keeps_recompute(monkeypatch):
    gen = torch.Generator(device="cuda").manual_seed(15)
    spy = _SpyExt(ops._load_extension())
    monkeypatch.setattr(L.ops, "_load_extension", lambda: spy)
    bn = FusedBatchNormAct2d(64, relu=True).cuda()
    x = _small_input(gen).requires_grad_(True)
    y = bn(x)
    (mask,) = _masks(spy.fwd_args[-1])
    assert mask.numel() == 0
    dy = _small_input(gen)
    y.backward(dy)
    # dbeta = sum of dy where the ReLU passed, in fp32
    kept = torch.where(y.detach() > 0, dy, torch.zeros_like(dy)).float()
    assert torch.allclose(bn.bias.grad, kept.sum((0, 2, 3)),
                          atol=2e-1, rtol=2e-2)
