"""Gradient sinks on the GPU: kernels that add a parameter gradient into
its fp32 bucket segment (k_bn_bwd_tail / k_wrw_reduce in accumulate mode,
k_accum_cast), and ResNet-18 through AdaptiveDataParallel with them.

Every kernel test carves its destinations out of one larger fp32 buffer
with guard floats on both sides, at float offsets that make the segment
16-byte aligned (0) or not (1, 3); the guards must come back untouched.
BN and the cast-accumulate are one fp32 add per element and must equal
the separate add bit for bit; the wrw tests use the dyadic inputs of
test_gpu_conv_exact.py, on which every order of addition is exact.
"""

import itertools

import pytest
import torch

from test_gpu_conv_exact import (GUARD, _Guarded, _assert_exact,
                                 _assert_exact_bound, _cpu64, _dyadic)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from adaptdl_amd import ops

GUARD_VALUE = 12345.0


class _Segments:
    """fp32 segments at given float offsets inside one guarded buffer:
    | GUARD | off floats | segment | GUARD | off | segment | ... | GUARD |
    """

    def __init__(self, sizes_offsets, gen):
        total = GUARD
        self.spans = []
        for numel, off in sizes_offsets:
            # keep every segment's base 16-byte aligned before `off`
            start = total + off
            self.spans.append((start, numel))
            total = start + numel + GUARD
            total += -total % 4
        self.flat = torch.full((total,), GUARD_VALUE, device="cuda")
        self.inside = torch.zeros(total, dtype=torch.bool, device="cuda")
        for start, numel in self.spans:
            # seeded dyadic prefill: multiples of 1/4, |v| <= 2
            self.flat[start:start + numel] = \
                (torch.randint(-8, 9, (numel,), generator=gen) / 4).cuda()
            self.inside[start:start + numel] = True
        self.prefill = [s.clone() for s in self.segments()]

    def segments(self):
        return [self.flat[a:a + n] for a, n in self.spans]

    def check_guards(self, what):
        assert bool((self.flat[~self.inside] == GUARD_VALUE).all()), \
            what + ": wrote outside its segment"


def _ext():
    ext = ops._load_extension()
    assert ext is not None
    return ext


# ---- BN ---------------------------------------------------------------

def _bn_bwd(ext, t, dgamma, dbeta, accum):
    dx = torch.empty_like(t["x"])
    dz = torch.empty_like(t["x"]) if t["z"].numel() else \
        torch.empty(0, dtype=torch.bfloat16, device="cuda")
    c = t["x"].shape[1]
    pqr = torch.full((3 * c,), float("nan"), device="cuda")
    ws = torch.empty(t["ws_numel"], device="cuda")
    ext.bn_bwd(t["x"], t["z"], t["dy"], dx, dz, t["gamma"], t["mean"],
               t["rstd"], t["scale"], t["shift"], True, t["relu"], ws,
               dgamma, dbeta, pqr, torch.empty(0, dtype=torch.uint8,
                                               device="cuda"), accum)
    return dx, dz, pqr


@pytest.mark.parametrize("off", [0, 3])
@pytest.mark.parametrize("shape,relu,residual", [
    ((2, 8, 4, 4), False, False),
    ((3, 64, 8, 8), True, True),
    ((2, 512, 4, 4), True, False),
])
def test_bn_bwd_accumulates_into_segments(shape, relu, residual, off):
    ext = _ext()
    n, c, h, w = shape
    m = n * h * w
    gen = torch.Generator().manual_seed(601)

    def bf16():
        return torch.randn(n, h, w, c, generator=gen).to(torch.bfloat16) \
            .cuda().permute(0, 3, 1, 2)

    f32 = dict(dtype=torch.float32, device="cuda")
    none16 = torch.empty(0, dtype=torch.bfloat16, device="cuda")
    t = {"x": bf16(), "dy": bf16(), "z": bf16() if residual else none16,
         "gamma": (torch.rand(c, generator=gen) + 0.5).cuda(),
         "relu": relu,
         "ws_numel": 2 * c * ext.bn_num_rblocks(m, c)}
    beta = torch.randn(c, generator=gen).cuda()
    for name in ("mean", "rstd", "scale", "shift"):
        t[name] = torch.empty(c, **f32)
    ext.bn_fwd(t["x"], t["z"], torch.empty_like(t["x"]), t["gamma"], beta,
               torch.zeros(c, **f32), torch.ones(c, **f32), 0.1, 1e-5,
               True, relu, torch.empty(t["ws_numel"], **f32), t["mean"],
               t["rstd"], t["scale"], t["shift"],
               torch.empty(0, dtype=torch.uint8, device="cuda"),
               torch.empty(0, dtype=torch.int64, device="cuda"))

    dgamma0, dbeta0 = torch.empty(c, **f32), torch.empty(c, **f32)
    dx0, dz0, pqr0 = _bn_bwd(ext, t, dgamma0, dbeta0, False)

    segs = _Segments([(c, off), (c, off)], gen)
    dgamma, dbeta = segs.segments()
    want_g, want_b = segs.prefill
    for _ in range(3):
        dx, dz, pqr = _bn_bwd(ext, t, dgamma, dbeta, True)
        want_g = torch.add(want_g, dgamma0)
        want_b = torch.add(want_b, dbeta0)
        assert torch.equal(dgamma, want_g) and torch.equal(dbeta, want_b)
        assert torch.equal(dx, dx0) and torch.equal(dz, dz0)
        assert torch.equal(pqr, pqr0)
    segs.check_guards("bn_bwd accum")


# ---- wrw --------------------------------------------------------------

@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("shape,nsplit,groups", [
    ((2, 64, 8, 8, 64), 2, 1),
    ((32, 64, 8, 8, 64), 32, 2),      # atomics into the segment, no memset
    ((16, 128, 4, 4, 64), 2, 1),      # w4 kernel
    ((136, 64, 4, 4, 64), 17, 2),     # w4 kernel, 17 chunks
])
def test_wrw_accumulates_into_segment(shape, nsplit, groups, off):
    ext = _ext()
    n, c, h, w, k = shape
    # two accumulated results plus a prefill no larger than one product
    _assert_exact_bound(2 * n * h * w + 1)
    assert ext.conv_wrw_ok(n, h, w, c, k)
    assert ext.conv_wrw_nsplit(n, h, w, c, k) == nsplit
    assert -(-nsplit // 16) == groups
    gen = torch.Generator().manual_seed(602)
    x, dy = _dyadic(gen, n, c, h, w), _dyadic(gen, n, k, h, w)
    ref = torch.nn.grad.conv2d_weight(
        _cpu64(x), (k, c, 3, 3), _cpu64(dy), stride=1, padding=1)
    ref = ref.permute(0, 2, 3, 1).reshape(-1).float().cuda()   # (K,3,3,C)

    segs = _Segments([(k * 9 * c, off)], gen)
    seg, = segs.segments()
    assert (seg.data_ptr() % 16 == 0) == (off == 0)
    x0, dy0 = x.clone(), dy.clone()
    for _ in range(2):
        ws = _Guarded(nsplit * k * 9 * c, torch.float32)
        ext.conv_wrw(x, dy, ws.inner, seg, True)
        torch.cuda.synchronize()
        ws.check("ws")
    _assert_exact(seg, segs.prefill[0] + 2 * ref,
                  "conv_wrw accum {} off {}".format(shape, off))
    segs.check_guards("conv_wrw accum")
    assert torch.equal(x, x0) and torch.equal(dy, dy0), "inputs changed"


# ---- cast-accumulate --------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("src_off", [0, 1])
@pytest.mark.parametrize("dst_off", [0, 1, 3])
def test_accum_cast(dst_off, src_off, dtype):
    ext = _ext()
    gen = torch.Generator().manual_seed(603)
    sizes = [1, 7, 8, 1027, 2 ** 20 + 5]
    segs = _Segments([(n, dst_off) for n in sizes], gen)
    for n, dst in zip(sizes, segs.segments()):
        src = torch.randn(n + src_off, generator=gen).to(dtype) \
            .cuda()[src_off:]
        want = dst + src.float()
        src0 = src.clone()
        ext.accum_cast(dst, src)
        assert torch.equal(dst, want), (n, dst_off, src_off, dtype)
        assert torch.equal(src, src0)
    segs.check_guards("accum_cast")


# ---- in context: ResNet-18 under AdaptiveDataParallel -----------------

_HOOKED = ["linear.bias", "linear.weight"]
_RUN_ID = itertools.count()     # AdaptiveDataParallel names are unique
_REAL = {}


def _noisy(name):
    """layer1/layer2 stride-1 3x3 weights: several reduce groups add
    into the segment with atomics, in an order that varies run to run."""
    return name.startswith(("layer1.", "layer2.")) and \
        name.endswith(("conv1.weight", "conv2.weight")) and \
        not name.startswith("layer2.0.conv1")


def _resnet_cycle(monkeypatch, sink, graphed=False, n_micro=4, lr=0.05):
    """ResNet-18, N=8, bf16 autocast, channels_last: one sync microbatch,
    then cycles of two accumulation microbatches and a sync one.
    Returns per-microbatch segment contents and hook firings."""
    import adaptdl_amd.collective as collective
    import adaptdl_amd.torch as adl
    from adaptdl_amd.models import ResNet18
    from adaptdl_amd.torch import _engine
    from adaptdl_amd.torch.data import AdaptiveDataLoaderHelper
    from adaptdl_amd.torch.graph_step import GraphedStepper

    monkeypatch.setenv("ADAPTDL_GRAD_SINK", sink)
    if not collective.initialized():
        collective.initialize(master_addr="127.0.0.1")

    def fake_sync(self):
        self._state.current_local_bsz = 8
        self._state.accumulation_steps = 2
        return 8

    monkeypatch.setattr(AdaptiveDataLoaderHelper, "_sync_local_bsz",
                        fake_sync)
    AdaptiveDataLoaderHelper._training = None
    AdaptiveDataLoaderHelper._current = None
    AdaptiveDataLoaderHelper._position.clear()

    hooked, in_hook = [], []
    cls = _engine.GradSyncEngine
    # the engine's own methods, not an earlier run's wrappers
    real_hook, real_ready = _REAL.setdefault(
        "methods", (cls._grad_ready_hook, cls._param_ready))

    def hook(self, param):
        in_hook.append(1)
        try:
            return real_hook(self, param)
        finally:
            in_hook.pop()

    def ready(self, param):
        if in_hook:
            hooked.append(names[param])
        return real_ready(self, param)

    monkeypatch.setattr(cls, "_grad_ready_hook", hook)
    monkeypatch.setattr(cls, "_param_ready", ready)

    torch.manual_seed(7)
    model = ResNet18().cuda().to(memory_format=torch.channels_last)
    names = {p: n for n, p in model.named_parameters()}
    optim = adl.FusedSGD(model.parameters(), lr=lr, momentum=0.9)
    adp = adl.AdaptiveDataParallel(
        model, optim, name="sink-{}".format(next(_RUN_ID)))
    engine = adp.gns.engine
    gen = torch.Generator().manual_seed(8)
    x = torch.randn(8, 3, 32, 32, generator=gen).cuda() \
        .contiguous(memory_format=torch.channels_last)
    y = torch.randint(0, 10, (8,), generator=gen).cuda()
    loader = adl.AdaptiveDataLoader(
        torch.utils.data.TensorDataset(torch.arange(8 * n_micro)),
        batch_size=8)

    def fwd_bwd(xb, yb):
        optim.zero_grad()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = torch.nn.functional.cross_entropy(adp(xb), yb)
        loss.backward()
        return loss

    stepper = GraphedStepper(adp, optim, fwd_bwd) if graphed else None
    record = []
    for _ in loader:
        del hooked[:]
        if stepper is not None:
            stepper.microbatch(x, y)
        else:
            fwd_bwd(x, y)
        record.append({
            "seg": {names[p]: b.flat[o:o + n].clone()
                    for b in engine.buckets for p, o, n in b.segments},
            "hooked": sorted(hooked)})
        optim.step()
    torch.cuda.synchronize()
    out = {"record": record,
           "weights": {n: p.detach().float().clone()
                       for n, p in model.named_parameters()},
           "stats": dict(stepper.stats) if stepper is not None else None}
    engine.detach()
    return out


def test_resnet18_sink_matches_hook_path(monkeypatch, tmp_ckpt_env):
    """Sink on against sink off, segment by segment.

    The library convs run with torch.backends.cudnn.deterministic: in
    its default mode the library's forward and backward-data results at
    N=8 differ between two identical calls (the loss itself does), so
    no two runs of ANY path would agree bit for bit.  With it, two
    sink-off runs differ only in the layer1 wrw weights, whose reduce
    groups are added with atomics.
    """
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    # lr = 0 keeps the weights fixed: the run-to-run rounding of the
    # atomically reduced gradients would otherwise reach every later
    # microbatch through the optimizer step.
    on = _resnet_cycle(monkeypatch, "1", lr=0.0)
    off = _resnet_cycle(monkeypatch, "0", lr=0.0)
    off2 = _resnet_cycle(monkeypatch, "0", lr=0.0)
    assert len(on["record"]) == 4
    names = sorted(on["record"][0]["seg"])
    assert len(names) == 62 and sum(map(_noisy, names)) == 7
    worst = noise = 0.0
    # measured before anything is asserted: the same figures for the
    # parameters held to torch.equal below
    exact_worst = max((a["seg"][n] - b["seg"][n]).abs().max().item()
                      for a, b in zip(on["record"], off["record"])
                      for n in names if not _noisy(n))
    exact_noise = max((b["seg"][n] - b2["seg"][n]).abs().max().item()
                      for b, b2 in zip(off["record"], off2["record"])
                      for n in names if not _noisy(n))
    print("other segments: sink-vs-hook max abs diff {:.3e}, "
          "hook-vs-hook {:.3e}".format(exact_worst, exact_noise))
    for a, b, b2 in zip(on["record"], off["record"], off2["record"]):
        # the post-accumulate hook notifies for the two linear
        # parameters only; with the switch off, for all 62
        assert a["hooked"] == _HOOKED
        assert b["hooked"] == names
        for name in names:
            if _noisy(name):
                worst = max(worst, (a["seg"][name] - b["seg"][name])
                            .abs().max().item())
                noise = max(noise, (b["seg"][name] - b2["seg"][name])
                            .abs().max().item())
            else:
                # BN, one-group wrw convs, library-wrw convs, linear
                assert torch.equal(a["seg"][name], b["seg"][name]), name
    print("layer1/layer2 wrw segments: sink-vs-hook max abs diff {:.3e}, "
          "hook-vs-hook {:.3e}".format(worst, noise))
    assert worst <= 2 * noise, (worst, noise)


def test_resnet18_sink_under_graph_stepper(monkeypatch, tmp_ckpt_env):
    import os
    if os.getenv("ADAPTDL_HIPGRAPH") != "1":
        pytest.skip("experimental: set ADAPTDL_HIPGRAPH=1")
    eager = _resnet_cycle(monkeypatch, "1", n_micro=25)
    eager2 = _resnet_cycle(monkeypatch, "1", n_micro=25)
    graphed = _resnet_cycle(monkeypatch, "1", graphed=True, n_micro=25)
    stats = graphed["stats"]
    assert stats["captures"] == 3 and stats["replays"] >= 3, stats
    # as test_hipgraph_stepper_matches_eager: within the order of the
    # eager runs' own divergence
    noise = max((eager["weights"][n] - eager2["weights"][n]).abs().max()
                .item() for n in eager["weights"])
    budget = max(10.0 * noise, 5e-3)
    for n, wg in graphed["weights"].items():
        assert torch.isfinite(wg).all(), n
        diff = (eager["weights"][n] - wg).abs().max().item()
        assert diff <= budget, (n, diff, noise)
