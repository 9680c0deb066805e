"""Gradient sinks on CPU: the engine's bookkeeping with the switch forced
on and the layers' plain-torch accumulation (``segment.add_``).

A sunk parameter's gradient is added to its bucket segment by the layer
that computes it; autograd gets None for it, so its post-accumulate hook
never fires and ``grad_written`` stands in for it.  Everything the engine
derives from the buckets (statistics, optimizer steps) must equal the
hook path exactly: each scenario runs in a child process once per switch
setting, eight microbatches that include a full cycle of three accumulation
microbatches and its sync microbatch, and the recorded tensors are compared
by torch.equal.
"""

import collections

import pytest
import torch
import torch.nn.functional as F

from conftest import elastic_multiprocessing

ACCUM = 3


class _Net(torch.nn.Module):
    def __init__(self, scenario):
        super().__init__()
        from adaptdl_amd.torch.layers import (FusedBatchNormAct2d,
                                              FusedConv2d)
        self.scenario = scenario
        self.conv = FusedConv2d(3, 8, 3, padding=1, bias=False)
        self.bn = FusedBatchNormAct2d(8, relu=True)
        self.conv2 = FusedConv2d(8, 8, 3, padding=1, bias=False)
        self.linear = torch.nn.Linear(8, 4)
        if scenario == "unused":
            self.spare = FusedConv2d(8, 8, 1, bias=False)
        self.armed = []   # was a sink engine armed during each forward

    def forward(self, x):
        from adaptdl_amd.torch import _engine
        self.armed.append(_engine._armed is not None)
        out = self.bn(self.conv(x))
        out = self.conv2(out)
        if self.scenario == "twice":
            out = self.conv2(F.relu(out))
        return self.linear(F.adaptive_avg_pool2d(out, 1).flatten(1))


def _run(scenario, sink, out_path):
    import os
    import adaptdl_amd.collective as collective
    import adaptdl_amd.torch as adl
    from adaptdl_amd.torch import _engine
    from adaptdl_amd.torch.data import AdaptiveDataLoaderHelper

    os.environ["ADAPTDL_GRAD_SINK"] = sink
    os.environ["ADAPTDL_BUCKET_CAP_MB"] = "0.0002"   # several buckets
    collective.initialize()

    def fake_sync(self):
        self._state.current_local_bsz = 8
        self._state.accumulation_steps = ACCUM
        return 8

    AdaptiveDataLoaderHelper._sync_local_bsz = fake_sync

    # Count what the engine sees, per backward pass.
    cls = _engine.GradSyncEngine
    seen = {"hook": [], "ready": [], "end": 0, "local_stat": 0}
    real_hook, real_ready = cls._grad_ready_hook, cls._param_ready
    real_end = cls._end_of_backward

    in_hook = []

    def hook(self, param):
        in_hook.append(1)
        try:
            return real_hook(self, param)
        finally:
            in_hook.pop()

    def ready(self, param):
        seen["ready"].append(names[param])
        if in_hook:   # counted by the post-accumulate hook
            seen["hook"].append(names[param])
        return real_ready(self, param)

    def end(self):
        seen["end"] += 1
        return real_end(self)

    cls._grad_ready_hook, cls._param_ready = hook, ready
    cls._end_of_backward = end

    torch.manual_seed(0)
    xs = torch.randn(64, 3, 6, 6)
    ys = torch.randint(0, 4, (64,))
    torch.manual_seed(1)
    model = _Net(scenario)
    names = {p: n for n, p in model.named_parameters()}
    tensor_hook_calls = []
    if scenario == "hooked":
        model.conv.weight.register_hook(
            lambda g: tensor_hook_calls.append(1))
    optim = torch.optim.SGD(model.parameters(), lr=0.05, momentum=0.9)
    adp = adl.AdaptiveDataParallel(model, optim)
    engine = adp.gns.engine
    real_local = adp.gns._local_stat

    def local_stat(bucket, mb):
        seen["local_stat"] += 1
        return real_local(bucket, mb)

    adp.gns._local_stat = local_stat
    loader = adl.AdaptiveDataLoader(
        torch.utils.data.TensorDataset(xs, ys), batch_size=8)

    record = []
    for _epoch in adl.remaining_epochs_until(1):
        for x, y in loader:
            optim.zero_grad()
            seen.update(hook=[], ready=[], end=0, local_stat=0)
            F.cross_entropy(adp(x), y).backward()
            record.append({
                "flat": [b.flat.clone() for b in engine.buckets],
                "stats": engine.stats.clone(),
                "hook": sorted(seen["hook"]),
                "ready": sorted(seen["ready"]),
                "end": seen["end"],
                "local_stat": seen["local_stat"],
                "sync": adp.require_backward_grad_sync,
            })
            optim.step()

    # Never armed: no_grad and eval forwards through ADP, and the bare
    # module.  None of them may hand out a sink.
    x = xs[:8]
    with torch.no_grad():
        adp(x)
    adp.eval()
    adp(x)
    adp.train()
    model(x)
    outside = _engine.grad_sink(model.conv.weight)

    torch.save({
        "record": record,
        "params": {n: p.detach().clone()
                   for n, p in model.named_parameters()},
        "n_buckets": len(engine.buckets),
        "armed": model.armed,
        "outside_is_none": outside is None,
        "tensor_hook_calls": len(tensor_hook_calls),
    }, out_path)
    collective.teardown()
    return 0


@elastic_multiprocessing
def _child(scenario, sink, out_path):
    return _run(scenario, sink, out_path)


def _both(tmp_path, scenario):
    out = {}
    for sink in ("1", "0"):
        path = str(tmp_path / "sink{}.pt".format(sink))
        _child(scenario, sink, path)
        out[sink] = torch.load(path, weights_only=False)
    return out["1"], out["0"]


def _same(a, b, exact):
    if exact:
        return torch.equal(a, b)
    # Re-associated fp32 sums: a gradient added in two parts rounds twice
    # per microbatch where autograd's pre-summed one rounds once; over
    # the at most 4 microbatches of a cycle that is within 8 ulp of the
    # largest magnitude involved (the optimizer steps carry it along).
    tol = 8 * 2.0 ** -23 * max(a.abs().max().item(), b.abs().max().item())
    return bool(((a - b).abs() <= tol).all())


def _assert_same_results(on, off, exact=True):
    assert len(on["record"]) == len(off["record"]) == 8
    syncs = [a["sync"] for a in on["record"]]
    # a cycle of ACCUM accumulation microbatches and its sync microbatch
    assert any(syncs[i:i + ACCUM + 1] == [False] * ACCUM + [True]
               for i in range(len(syncs))), syncs
    for i, (a, b) in enumerate(zip(on["record"], off["record"])):
        assert a["sync"] == b["sync"]
        for fa, fb in zip(a["flat"], b["flat"]):
            assert _same(fa, fb, exact), "bucket differs at microbatch %d" % i
        if exact:
            assert torch.equal(a["stats"], b["stats"]), i
        else:
            assert torch.allclose(a["stats"], b["stats"], rtol=1e-5), i
        assert a["end"] == b["end"] == 1          # once per backward
        assert a["ready"] == b["ready"]           # same parameters, once
        assert a["local_stat"] == b["local_stat"]
    assert on["params"].keys() == off["params"].keys()
    for name in on["params"]:
        assert _same(on["params"][name], off["params"][name], exact), name


_ALL = ["bn.bias", "bn.weight", "conv.weight", "conv2.weight",
        "linear.bias", "linear.weight"]
_LINEAR = ["linear.bias", "linear.weight"]


def test_sink_equals_hook_path(tmp_path):
    on, off = _both(tmp_path, "base")
    _assert_same_results(on, off)
    assert on["n_buckets"] > 1
    for a, b in zip(on["record"], off["record"]):
        # the post-accumulate hook fires only for parameters not sunk
        assert a["hook"] == _LINEAR
        assert a["ready"] == _ALL
        # ADAPTDL_GRAD_SINK=0 restores the hook for every parameter
        assert b["hook"] == b["ready"] == _ALL
        # every bucket's local statistic runs, on the sync microbatch only
        assert (a["local_stat"] >= on["n_buckets"]) == a["sync"]
        assert a["sync"] or a["local_stat"] == 0


def test_arming(tmp_path):
    on, off = _both(tmp_path, "base")
    train = [True] * 8
    # then: no_grad through ADP, eval through ADP, the bare module
    assert on["armed"] == train + [False, False, False]
    assert off["armed"] == on["armed"]    # armed, but the switch is off
    assert on["outside_is_none"] and off["outside_is_none"]


def test_module_applied_twice_notifies_once(tmp_path):
    on, off = _both(tmp_path, "twice")
    # conv2's two gradients reach the bucket one by one instead of
    # pre-summed by autograd: equal up to that re-association
    _assert_same_results(on, off, exact=False)
    for a in on["record"]:
        assert a["ready"].count("conv2.weight") == 1
        assert a["hook"] == _LINEAR


def test_unused_parameter_bucket_still_flushes(tmp_path):
    on, off = _both(tmp_path, "unused")
    _assert_same_results(on, off)
    for a in on["record"]:
        assert "spare.weight" not in a["ready"]
        assert (a["local_stat"] >= on["n_buckets"]) == a["sync"]
    assert not on["params"]["spare.weight"].isnan().any()


def test_parameter_with_tensor_hook_is_not_sunk(tmp_path):
    on, off = _both(tmp_path, "hooked")
    _assert_same_results(on, off)
    for a in on["record"]:
        assert a["hook"] == ["conv.weight"] + _LINEAR
    assert on["tensor_hook_calls"] == off["tensor_hook_calls"] \
        == 8


def test_grad_sinks_all_or_nothing(monkeypatch):
    """A kernel that writes two parameters gets both segments or none."""
    from adaptdl_amd.torch import _engine
    monkeypatch.setenv("ADAPTDL_GRAD_SINK", "1")

    class _Owner:
        pass

    w = torch.nn.Parameter(torch.randn(4))
    b = torch.nn.Parameter(torch.randn(4))
    other = torch.nn.Parameter(torch.randn(4))
    engine = _engine.GradSyncEngine([[w, b]], owner=_Owner())
    try:
        assert _engine.grad_sinks((w, b)) is None          # not armed
        with _engine.armed(engine):
            assert _engine.grad_sinks((w, other)) is None  # no engine
            assert not engine._sink_pending
            segs = _engine.grad_sinks((w, b))
            assert [s.data_ptr() for s in segs] == \
                [w.grad.data_ptr(), b.grad.data_ptr()]
            assert all(s.dim() == 1 and s.is_contiguous() for s in segs)
            assert collections.Counter(engine._sink_pending.values()) \
                == {1: 2}
        assert _engine.grad_sink(w) is None                # disarmed
    finally:
        engine.detach()
    with _engine.armed(engine):
        assert _engine.grad_sink(w) is None                # detached


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_low_precision_bucket_has_no_sink(dtype, monkeypatch):
    from adaptdl_amd.torch import _engine
    monkeypatch.setenv("ADAPTDL_GRAD_SINK", "1")

    class _Owner:
        pass

    w = torch.nn.Parameter(torch.randn(4).to(dtype))
    engine = _engine.GradSyncEngine([[w]], owner=_Owner())
    try:
        with _engine.armed(engine):
            assert _engine.grad_sink(w) is None
    finally:
        engine.detach()
