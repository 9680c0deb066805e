"""Numerics of the master-weight HIP kernels vs fp64 torch references.

k_fused_sgd_mw_*, k_fused_adamw_mw_* and k_precond_sqsum[_dev]_mw_* take a
bf16/fp16 gradient next to fp32 master weights / optimizer state.  Each is
compared with the same math in fp64 torch on the upcast inputs, over
slices that reach the scalar head, the 16-byte vector body, the scalar
tail, a second grid-stride trip, and the whole-launch scalar fallback.
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from adaptdl_amd import ops
    assert ops.has_extension(), \
        "HIP extension must be built+importable on a GPU box"

DTYPES = [torch.bfloat16, torch.float16]

# (n, element offset of the low-precision operands, of the fp32 ones).
# Equal offsets keep every operand co-aligned.  The grid is capped at
# 2048 blocks of 256 lanes with <= 8 elements per lane, so only the last
# co-aligned shape makes the stride loop take a second trip.  In the final
# row the fp32 operands are 16-byte aligned where the low-precision ones
# are not: the whole launch takes the scalar loop.
SHAPES = [(1, 0, 0), (17, 1, 1), (255, 3, 3), (4097, 2, 2),
          (2048 * 256 * 8 + 4099, 3, 3), (4097, 1, 0)]
PAD = 16  # guard elements on either side of every slice


class _Buf(object):
    """A slice [PAD + off, PAD + off + n) of a larger buffer, with a
    snapshot to check that nothing outside the slice was written."""

    def __init__(self, full, off, n):
        self.full = full
        self.lo, self.hi = PAD + off, PAD + off + n
        self.view = full[self.lo:self.hi]
        self.before = full.clone()

    def outside_unchanged(self):
        return torch.equal(self.full[:self.lo], self.before[:self.lo]) \
            and torch.equal(self.full[self.hi:], self.before[self.hi:])


def _lp(n, off, dtype, fill=None):
    size = n + off + 2 * PAD
    if fill is None:
        full = torch.randn(size, device="cuda").to(dtype)
    else:
        full = torch.full((size,), fill, device="cuda", dtype=dtype)
    return _Buf(full, off, n)


def _f32(n, off, scale=1.0, positive=False):
    full = torch.randn(n + off + 2 * PAD, device="cuda")
    full = (full.abs() if positive else full) * scale
    return _Buf(full, off, n)


def _check_alignment(bufs_lp, bufs_f32, off_lp, off_f32):
    ptrs = [b.view.data_ptr() for b in bufs_lp]
    head = (-ptrs[0] % 16) // 2
    co_aligned = all((b.view.data_ptr() + 2 * head) % 16 == 0
                     for b in bufs_lp) and \
        all((b.view.data_ptr() + 4 * head) % 16 == 0 for b in bufs_f32)
    assert co_aligned == (off_lp == off_f32)


@pytest.mark.parametrize("n,off_lp,off_f32", SHAPES)
@pytest.mark.parametrize("momentum,nesterov,wd", [
    (0.0, False, 0.0), (0.9, False, 5e-4), (0.9, True, 5e-4)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_sgd_master_step(dtype, momentum, nesterov, wd, n, off_lp,
                               off_f32):
    torch.manual_seed(n + 70)
    p = _lp(n, off_lp, dtype, fill=7.0)
    g = _lp(n, off_lp, dtype)
    w = _f32(n, off_f32)
    m = _f32(n, off_f32)
    _check_alignment([p, g], [w, m], off_lp, off_f32)
    lr, damp = 0.1, 0.0
    d = g.view.double()
    w_ref, m_ref = w.view.double(), m.view.double()
    if wd:
        d = d + wd * w_ref
    if momentum:
        m_ref = momentum * m_ref + (1 - damp) * d
        d = d + momentum * m_ref if nesterov else m_ref
    w_ref = w_ref - lr * d

    ops.fused_sgd_master_step(p.view, g.view, w.view,
                              m.view if momentum else None, lr, momentum,
                              wd, damp, nesterov)
    assert torch.allclose(w.view.double(), w_ref, rtol=1e-5, atol=1e-6)
    if momentum:
        assert torch.allclose(m.view.double(), m_ref, rtol=1e-5, atol=1e-6)
    else:
        assert torch.equal(m.full, m.before)
    assert torch.equal(p.view, w.view.to(dtype))  # RNE of the new master
    assert torch.equal(g.full, g.before)          # gradient is read-only
    for buf in (p, w, m):
        assert buf.outside_unchanged()


@pytest.mark.parametrize("n,off_lp,off_f32", SHAPES)
@pytest.mark.parametrize("adam_mode,wd", [(True, 0.0), (True, 1e-2),
                                          (False, 1e-2)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_adamw_master_step(dtype, adam_mode, wd, n, off_lp, off_f32):
    torch.manual_seed(n + 71)
    p = _lp(n, off_lp, dtype, fill=7.0)
    g = _lp(n, off_lp, dtype)
    w = _f32(n, off_f32)
    m = _f32(n, off_f32, scale=0.01, positive=True)
    v = _f32(n, off_f32, scale=0.01, positive=True)
    _check_alignment([p, g], [w, m, v], off_lp, off_f32)
    lr, b1, b2, eps, step = 1e-3, 0.9, 0.999, 1e-8, 10
    g_ref, w_ref = g.view.double(), w.view.double()
    m_ref, v_ref = m.view.double(), v.view.double()
    if adam_mode and wd:
        g_ref = g_ref + wd * w_ref
    elif not adam_mode and wd:
        w_ref = w_ref * (1 - lr * wd)
    m_ref = b1 * m_ref + (1 - b1) * g_ref
    v_ref = b2 * v_ref + (1 - b2) * g_ref * g_ref
    denom = (v_ref / (1 - b2 ** step)).sqrt() + eps
    w_ref = w_ref - lr / (1 - b1 ** step) * m_ref / denom

    ops.fused_adamw_master_step(p.view, g.view, w.view, m.view, v.view, lr,
                                b1, b2, eps, wd, step, adam_mode)
    assert torch.allclose(w.view.double(), w_ref, rtol=1e-4, atol=1e-6)
    assert torch.allclose(m.view.double(), m_ref, rtol=1e-4, atol=1e-6)
    assert torch.allclose(v.view.double(), v_ref, rtol=1e-4, atol=1e-6)
    assert torch.equal(p.view, w.view.to(dtype))
    assert torch.equal(g.full, g.before)
    for buf in (p, w, m, v):
        assert buf.outside_unchanged()


@pytest.mark.parametrize("n,off_lp,off_f32", SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_precond_sqsum_mixed(dtype, n, off_lp, off_f32):
    """bf16/fp16 g with fp32 v: host-scalar and device-scalar forms, both
    use_precond settings, accumulating into a non-zero ``out``."""
    torch.manual_seed(n + 72)
    g = _lp(n, off_lp, dtype)
    v = _Buf(torch.rand(n + off_f32 + 2 * PAD, device="cuda"), off_f32, n)
    beta2, eps, step = 0.999, 1e-8, 42
    corr = 1 - beta2 ** step
    pinv = (v.view.double() / corr).sqrt() + eps
    ref = (g.view.double() / pinv).pow(2).sum()
    start = 3.5

    out = torch.full((), start, dtype=torch.float64, device="cuda")
    ops.precond_sqsum(g.view, v.view, beta2, eps, step, out)
    assert torch.allclose(out - start, ref, rtol=1e-5)

    pc = torch.zeros(4, dtype=torch.float32, device="cuda")
    ops.set_precond_scalars(pc, beta2, eps, step)
    out = torch.full((), start, dtype=torch.float64, device="cuda")
    ops.precond_sqsum_dev(g.view, v.view, pc, out)
    assert torch.allclose(out - start, ref, rtol=1e-5)

    # Identity mode (step below the warmup gate) == plain sqsum of g.
    ops.set_precond_scalars(pc, beta2, eps, 2)
    out = torch.full((), start, dtype=torch.float64, device="cuda")
    ops.precond_sqsum_dev(g.view, v.view, pc, out)
    assert torch.allclose(out - start, g.view.double().pow(2).sum(),
                          rtol=1e-10)
    assert torch.equal(g.full, g.before) and torch.equal(v.full, v.before)


@pytest.mark.parametrize("dtype", DTYPES)
def test_precond_sqsum_low_precision_second_moment(dtype):
    """Stock torch.optim.Adam on a bf16/fp16 model keeps exp_avg_sq in the
    parameter dtype; the per-segment statistics widen it for the kernel."""
    n = 1023
    torch.manual_seed(n + 73)
    g = torch.randn(n + 1, device="cuda").to(dtype)[1:]
    v = torch.rand(n, device="cuda").to(dtype)
    beta2, eps, step = 0.999, 1e-8, 42
    out = torch.zeros((), dtype=torch.float64, device="cuda")
    ops.precond_sqsum(g, v, beta2, eps, step, out)
    pinv = (v.double() / (1 - beta2 ** step)).sqrt() + eps
    ref = (g.double() / pinv).pow(2).sum()
    assert torch.allclose(out, ref, rtol=1e-5)


def test_master_entry_points_check_arguments():
    ext = ops._load_extension()
    p = torch.zeros(8, device="cuda", dtype=torch.bfloat16)
    g = torch.zeros(8, device="cuda", dtype=torch.bfloat16)
    w = torch.zeros(8, device="cuda")
    none = torch.empty(0, device="cuda")
    with pytest.raises(RuntimeError, match="dtype mismatch"):
        ext.fused_sgd_mw(p, g.half(), w, none, 0.1, 0.0, 0.0, 0.0, False)
    with pytest.raises(RuntimeError, match="bfloat16 or float16"):
        ext.fused_sgd_mw(w, w, w, none, 0.1, 0.0, 0.0, 0.0, False)
    with pytest.raises(RuntimeError, match="master must be float32"):
        ext.fused_sgd_mw(p, g, p, none, 0.1, 0.0, 0.0, 0.0, False)
    with pytest.raises(RuntimeError, match="size mismatch"):
        ext.fused_sgd_mw(p, g, w[:4], none, 0.1, 0.0, 0.0, 0.0, False)
    with pytest.raises(RuntimeError, match="size mismatch"):
        ext.fused_adamw_mw(p, g, w, w, w[:4], 1e-3, 0.9, 0.999, 1e-8, 0.0,
                           1, False)
    with pytest.raises(RuntimeError, match="contiguous"):
        ext.fused_adamw_mw(p, g, torch.zeros(16, device="cuda")[::2], w, w,
                           1e-3, 0.9, 0.999, 1e-8, 0.0, 1, False)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ext.fused_adamw_mw(p, g, w.cpu(), w, w, 1e-3, 0.9, 0.999, 1e-8,
                           0.0, 1, False)


def test_bf16_model_fused_adamw_master_e2e(tmp_ckpt_env):
    """bf16 MLP through AdaptiveDataParallel with
    FusedAdamW(master_weights=True): 8 eager steps on the GPU."""
    import adaptdl_amd.collective as collective
    import adaptdl_amd.torch as adl

    if not collective.initialized():
        collective.initialize(master_addr="127.0.0.1")
    device = torch.device("cuda")
    torch.manual_seed(0)
    model = torch.nn.Sequential(
        torch.nn.Linear(8, 16), torch.nn.ReLU(),
        torch.nn.Linear(16, 4)).to(device).bfloat16()
    params = list(model.parameters())
    optim = adl.FusedAdamW(params, lr=1e-3, weight_decay=0.01,
                           master_weights=True)
    adp = adl.AdaptiveDataParallel(model, optim, name="mw-gpu-e2e")
    start = [optim.state[p]["master_param"].clone() for p in params]
    xs = torch.randn(64, 8, device=device).bfloat16()
    ys = torch.randint(0, 4, (64,), device=device)
    loader = adl.AdaptiveDataLoader(
        torch.utils.data.TensorDataset(torch.arange(64)), batch_size=16)
    steps = 0
    for _pass in range(2):  # loader iterates outside any epoch loop
        for (idx,) in loader:
            idx = idx.to(device)
            optim.zero_grad()
            loss = torch.nn.functional.cross_entropy(
                adp(xs[idx]).float(), ys[idx])
            loss.backward()
            optim.step()
            steps += 1
    assert steps == 8
    assert torch.isfinite(loss.detach()).item()
    for bucket in adp.gns.engine.buckets:
        assert bucket.flat.dtype == torch.bfloat16
        assert bucket.master_flat.dtype == torch.float32
        assert bucket.adam_state["precond"] is not None
        assert bucket.adam_state["exp_avg_sq"].dtype == torch.float32
        assert bucket.adam_state["step"] == 8
    assert np.isfinite(adp.gns.sqr_avg())
    assert np.isfinite(adp.gns.var_avg())
    for p, w0 in zip(params, start):
        master = optim.state[p]["master_param"]
        assert torch.isfinite(master).all()
        assert not torch.equal(master, w0)
        assert torch.equal(p.detach(), master.bfloat16())
