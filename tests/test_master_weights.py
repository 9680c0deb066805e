"""Fused optimizers with fp32 master weights on bf16/fp16 parameters.

``FusedSGD/FusedAdam/FusedAdamW(master_weights=True)`` keep an fp32 master
copy of every low-precision bucket, integrate the update there and write
the parameters as the rounded master (CPU fallback path here; the HIP
kernels are covered by tests/test_gpu_master_weights.py).
"""

import logging

import numpy as np
import pytest
import torch

import adaptdl_amd.checkpoint
import adaptdl_amd.collective
import adaptdl_amd.env
from conftest import elastic_multiprocessing

LP_DTYPES = [torch.bfloat16, torch.float16]


def _mlp(seed, dtype):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(8, 16), torch.nn.ReLU(),
                               torch.nn.Linear(16, 4)).to(dtype)


def _reset_loop_state(adp):
    """Let one replica process run a second training loop."""
    from adaptdl_amd.torch import data as _data
    from adaptdl_amd.torch import epoch as _epoch
    adp.gns.engine.detach()
    _data.AdaptiveDataLoaderHelper._current = None
    _data.AdaptiveDataLoaderHelper._training = None
    _data.AdaptiveDataLoaderHelper._position.clear()
    if _epoch._EPOCH_STATE is not None:
        _epoch._EPOCH_STATE.finished_epochs = 0
        _epoch._EPOCH_STATE.current_epoch = None


def _masters(optim, params):
    return [optim.state[p]["master_param"] for p in params]


# ---- sub-ulp accumulation -------------------------------------------------

class _OneWeight(torch.nn.Module):
    """One bf16 weight of value 1.0 whose gradient is exactly 1.0."""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(1, dtype=torch.bfloat16))

    def forward(self, x):
        return self.w.sum() + 0.0 * x.sum()


@elastic_multiprocessing
def _run_sub_ulp():
    import adaptdl_amd.torch as adl
    from adaptdl_amd.torch.optim import FusedSGD
    adaptdl_amd.collective.initialize("127.0.0.1")
    finals = {}
    for variant in ("stock", "master"):
        model = _OneWeight()
        if variant == "stock":
            optim = torch.optim.SGD(model.parameters(), lr=1e-3)
        else:
            optim = FusedSGD(model.parameters(), lr=1e-3,
                             master_weights=True)
        adp = adl.AdaptiveDataParallel(model, optim, name="ulp-" + variant)
        loader = adl.AdaptiveDataLoader(
            torch.utils.data.TensorDataset(torch.zeros(20, 1)),
            batch_size=1)
        steps = 0
        for _ in adl.remaining_epochs_until(1):
            for (x,) in loader:
                optim.zero_grad()
                adp(x.bfloat16()).backward()
                assert float(model.w.grad) == 1.0
                optim.step()
                steps += 1
        assert steps == 20
        finals[variant] = model.w.detach().clone()
        if variant == "master":
            master = optim.state[model.w]["master_param"]
            assert master.dtype == torch.float32
            assert abs(float(master) - 0.98) < 1e-6, float(master)
        _reset_loop_state(adp)
    # A bf16 ulp at 1.0 is 2**-7: every 1e-3 step rounds away in bf16.
    assert float(finals["stock"]) == 1.0
    expect = torch.tensor(0.98).bfloat16()
    assert float(expect) == 0.98046875
    assert torch.equal(finals["master"], expect.reshape(1))
    adaptdl_amd.collective.teardown()
    return 0


def test_sub_ulp_updates_accumulate_in_master():
    _run_sub_ulp()


# ---- trajectory against stock torch on an fp32 shadow ---------------------

@elastic_multiprocessing
def _run_trajectory(fused_name, plain_cls, kwargs, dtype):
    import adaptdl_amd.torch as adl
    from adaptdl_amd.torch import optim as fused_optim
    adaptdl_amd.collective.initialize("127.0.0.1")
    model = _mlp(21, dtype)
    params = list(model.parameters())
    optim = getattr(fused_optim, fused_name)(
        params, master_weights=True, **kwargs)
    adp = adl.AdaptiveDataParallel(model, optim, name="mw-traj")
    shadow = [p.detach().float().clone().requires_grad_(True)
              for p in params]
    shadow_optim = plain_cls(shadow, **kwargs)
    torch.manual_seed(22)
    xs = torch.randn(64, 8).to(dtype)
    ys = torch.randint(0, 4, (64,))
    loader = adl.AdaptiveDataLoader(
        torch.utils.data.TensorDataset(xs, ys), batch_size=16)
    steps = 0
    for _ in adl.remaining_epochs_until(2):
        for x, y in loader:
            optim.zero_grad()
            torch.nn.functional.cross_entropy(adp(x).float(), y).backward()
            for p, s in zip(params, shadow):
                s.grad = p.grad.float().clone()
            optim.step()
            shadow_optim.step()
            steps += 1
            for p, s, master in zip(params, shadow, _masters(optim, params)):
                assert master.dtype == torch.float32
                assert torch.allclose(master, s.detach(), atol=1e-5), \
                    (steps, (master - s.detach()).abs().max())
                assert torch.equal(p.detach(), master.to(dtype))
    assert steps == 8
    assert np.isfinite(adp.gns.sqr_avg())
    assert np.isfinite(adp.gns.var_avg())
    for bucket in adp.gns.engine.buckets:
        assert bucket.master_flat is not None
        assert bucket.master_flat.dtype == torch.float32
        assert bucket.param_flat.dtype == dtype
        if fused_name != "FusedSGD":
            # The one-launch preconditioned statistics path is reachable.
            assert bucket.adam_state["exp_avg_sq"].dtype == torch.float32
            assert "precond" in bucket.adam_state
    adaptdl_amd.collective.teardown()
    return 0


@pytest.mark.parametrize("dtype", LP_DTYPES)
def test_master_sgd_trajectory(dtype):
    _run_trajectory("FusedSGD", torch.optim.SGD,
                    dict(lr=0.05, momentum=0.9, weight_decay=1e-4), dtype)


@pytest.mark.parametrize("dtype", LP_DTYPES)
def test_master_adamw_trajectory(dtype):
    _run_trajectory("FusedAdamW", torch.optim.AdamW,
                    dict(lr=1e-3, weight_decay=0.01), dtype)


@pytest.mark.parametrize("dtype", LP_DTYPES)
def test_master_adam_trajectory(dtype):
    _run_trajectory("FusedAdam", torch.optim.Adam, dict(lr=1e-3), dtype)


@elastic_multiprocessing
def _run_stock_adam_lp_model():
    """Stock torch.optim.Adam on a bf16 model: the per-segment
    preconditioned statistics see a bf16 gradient."""
    import adaptdl_amd.torch as adl
    adaptdl_amd.collective.initialize("127.0.0.1")
    model = _mlp(23, torch.bfloat16)
    optim = torch.optim.Adam(model.parameters(), lr=1e-3)
    adp = adl.AdaptiveDataParallel(model, optim, name="mw-stock-adam")
    xs = torch.randn(64, 8).bfloat16()
    ys = torch.randint(0, 4, (64,))
    loader = adl.AdaptiveDataLoader(
        torch.utils.data.TensorDataset(xs, ys), batch_size=16)
    for _ in adl.remaining_epochs_until(2):
        for x, y in loader:
            optim.zero_grad()
            torch.nn.functional.cross_entropy(adp(x).float(), y).backward()
            optim.step()
    assert np.isfinite(adp.gns.sqr_avg())
    assert np.isfinite(adp.gns.var_avg())
    adaptdl_amd.collective.teardown()
    return 0


def test_stock_adam_on_bf16_model_statistics():
    _run_stock_adam_lp_model()


# ---- one fp32 and one bf16 bucket -----------------------------------------

class _Mixed(torch.nn.Module):
    """bf16 Linears around an fp32 LayerNorm."""

    def __init__(self):
        super().__init__()
        self.fc1 = torch.nn.Linear(8, 16).bfloat16()
        self.norm = torch.nn.LayerNorm(16)
        self.fc2 = torch.nn.Linear(16, 4).bfloat16()

    def linears(self):
        return list(self.fc1.parameters()) + list(self.fc2.parameters())

    def forward(self, x):
        h = self.norm(self.fc1(x.bfloat16()).float())
        return self.fc2(torch.relu(h).bfloat16()).float()


def _train_mixed(adl, model, optim, name):
    adp = adl.AdaptiveDataParallel(model, optim, name=name)
    torch.manual_seed(32)
    xs = torch.randn(64, 8)
    ys = torch.randint(0, 4, (64,))
    loader = adl.AdaptiveDataLoader(
        torch.utils.data.TensorDataset(xs, ys), batch_size=16)
    for _ in adl.remaining_epochs_until(2):
        for x, y in loader:
            optim.zero_grad()
            torch.nn.functional.cross_entropy(adp(x), y).backward()
            optim.step()
    return adp


@elastic_multiprocessing
def _run_mixed_dtypes():
    """The fp32 bucket of a mixed model is handled as without masters.

    First a plain run (one param group, real learning rate) checks the
    bucket kinds.  Then the LayerNorm's trajectory beside a bf16 bucket
    is compared with the same model in which the LayerNorm is the only
    bucket.  Its gradients depend on the Linears, so both runs hold them
    fixed: a zero learning rate on their (stepped, master-weight) bucket
    in the first, requires_grad=False in the second.
    """
    import adaptdl_amd.torch as adl
    from adaptdl_amd.torch.optim import FusedSGD
    adaptdl_amd.collective.initialize("127.0.0.1")
    kwargs = dict(lr=0.05, momentum=0.9, master_weights=True)

    torch.manual_seed(31)
    model = _Mixed()
    before = [p.detach().clone() for p in model.parameters()]
    optim = FusedSGD(model.parameters(), **kwargs)
    adp = _train_mixed(adl, model, optim, "mw-mixed")
    kinds = {b.flat.dtype: b for b in adp.gns.engine.buckets}
    assert len(adp.gns.engine.buckets) == 2
    assert kinds[torch.float32].master_flat is None
    assert kinds[torch.bfloat16].master_flat.dtype == torch.float32
    for p in model.norm.parameters():
        assert "master_param" not in optim.state[p]
        assert optim.state[p]["momentum_buffer"].dtype == torch.float32
    for p in model.linears():
        st = optim.state[p]
        assert st["momentum_buffer"].dtype == torch.float32
        assert torch.equal(p.detach(), st["master_param"].bfloat16())
    for p, b in zip(model.parameters(), before):
        assert not torch.equal(p.detach(), b)
    _reset_loop_state(adp)

    results = {}
    for variant in ("beside-bf16", "alone"):
        torch.manual_seed(31)
        model = _Mixed()
        norm = list(model.norm.parameters())
        if variant == "alone":
            for p in model.linears():
                p.requires_grad_(False)
            optim = FusedSGD(norm, **kwargs)
        else:
            optim = FusedSGD([{"params": norm},
                              {"params": model.linears(), "lr": 0.0}],
                             **kwargs)
        adp = _train_mixed(adl, model, optim, "mw-mixed-" + variant)
        n_buckets = len(adp.gns.engine.buckets)
        assert n_buckets == (1 if variant == "alone" else 2)
        for b in adp.gns.engine.buckets:
            assert (b.master_flat is None) == (b.flat.dtype ==
                                               torch.float32)
        results[variant] = [p.detach().clone() for p in norm] + \
            [optim.state[p]["momentum_buffer"].clone() for p in norm]
        _reset_loop_state(adp)
    for a, b in zip(results["beside-bf16"], results["alone"]):
        assert torch.equal(a, b)
    adaptdl_amd.collective.teardown()
    return 0


def test_mixed_dtype_buckets():
    _run_mixed_dtypes()


# ---- checkpoint restart ---------------------------------------------------

_STATE_KEYS = ("master_param", "exp_avg", "exp_avg_sq")


@elastic_multiprocessing
def _run_master_checkpoint_roundtrip(saved_path):
    import adaptdl_amd.torch as adl
    from adaptdl_amd.torch.optim import FusedAdamW
    adaptdl_amd.collective.initialize("127.0.0.1")
    model = _mlp(41, torch.bfloat16)
    params = list(model.parameters())
    optim = FusedAdamW(params, lr=1e-3, weight_decay=0.01,
                       master_weights=True)
    adp = adl.AdaptiveDataParallel(model, optim, name="mw-ckpt")
    if adaptdl_amd.env.num_restarts() == 1:
        # Restored by the constructor: bit-exact fp32, in flat storage.
        saved = torch.load(saved_path)
        flats = {}
        for bucket in adp.gns.engine.buckets:
            flats["master_param"] = bucket.master_flat
            flats["exp_avg"] = bucket.adam_state["exp_avg"]
            flats["exp_avg_sq"] = bucket.adam_state["exp_avg_sq"]
        assert len(adp.gns.engine.buckets) == 1
        for i, p in enumerate(params):
            st = optim.state[p]
            for key in _STATE_KEYS:
                assert st[key].dtype == torch.float32, key
                assert torch.equal(st[key], saved[key][i]), key
                assert st[key].untyped_storage().data_ptr() == \
                    flats[key].untyped_storage().data_ptr(), key
            assert torch.equal(p.detach(), st["master_param"].bfloat16())
            assert int(st["step"]) == saved["step"]
        assert adp.gns.engine.buckets[0].adam_state["step"] == \
            saved["step"]
    torch.manual_seed(42)
    xs = torch.randn(32, 8).bfloat16()
    ys = torch.randint(0, 4, (32,))
    loader = adl.AdaptiveDataLoader(
        torch.utils.data.TensorDataset(xs, ys), batch_size=8)
    for epoch in adl.remaining_epochs_until(4):
        for x, y in loader:
            optim.zero_grad()
            torch.nn.functional.cross_entropy(adp(x).float(), y).backward()
            optim.step()
        if adaptdl_amd.env.num_restarts() == 0 and epoch == 1:
            masters = _masters(optim, params)
            # The saved master must need more than bf16 to be restored.
            assert any((m != m.bfloat16().float()).any() for m in masters)
            saved = {key: [optim.state[p][key].clone() for p in params]
                     for key in _STATE_KEYS}
            saved["step"] = int(optim.state[params[0]]["step"])
            torch.save(saved, saved_path)
            adaptdl_amd.collective.teardown()
            adaptdl_amd.checkpoint.save_all_states()
            return 2
    for p in params:
        assert torch.equal(p.detach(),
                           optim.state[p]["master_param"].bfloat16())
    assert np.isfinite(adp.gns.var_avg())
    adaptdl_amd.collective.teardown()
    return 0


def test_master_checkpoint_restart(tmp_path):
    _run_master_checkpoint_roundtrip(str(tmp_path / "expected.pt"))


# ---- replicas start from rank 0's weights ---------------------------------

def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@elastic_multiprocessing
def _run_replica_start():
    import adaptdl_amd.torch as adl
    from adaptdl_amd.torch.optim import FusedSGD
    if adaptdl_amd.env.num_restarts() == 0:
        return 2  # restart with two replicas
    adaptdl_amd.collective.initialize()
    torch.distributed.init_process_group(
        "gloo", init_method="tcp://127.0.0.1:{}".format(
            adaptdl_amd.collective.broadcast(_free_port())),
        world_size=adaptdl_amd.env.num_replicas(),
        rank=adaptdl_amd.env.replica_rank())
    rank = adaptdl_amd.env.replica_rank()
    model = _mlp(50 + rank, torch.bfloat16)
    params = list(model.parameters())
    initial = [p.detach().float().clone() for p in params]
    rank0 = [t.clone() for t in initial]
    for t in rank0:
        torch.distributed.broadcast(t, src=0)
    if rank != 0:
        assert not torch.equal(initial[0], rank0[0])
    optim = FusedSGD(params, lr=0.05, master_weights=True)
    adl.AdaptiveDataParallel(model, optim, name="mw-replicas")
    for p, master, want in zip(params, _masters(optim, params), rank0):
        assert master.dtype == torch.float32
        assert torch.equal(master, want)
        assert torch.equal(p.detach().float(), want)
    adaptdl_amd.collective.teardown()
    torch.distributed.destroy_process_group()
    return 0


def test_replica_masters_start_from_rank0():
    _run_replica_start()


# ---- the flag is opt-in ---------------------------------------------------

@pytest.mark.parametrize("dtype", LP_DTYPES)
def test_refusal_names_the_flag(tmp_ckpt_env, dtype):
    import adaptdl_amd.torch as adl
    if not adaptdl_amd.collective.initialized():
        adaptdl_amd.collective.initialize(master_addr="127.0.0.1")
    try:
        model = torch.nn.Linear(4, 2).to(dtype)
        optim = adl.FusedAdamW(model.parameters(), lr=0.1)
        with pytest.raises(ValueError) as err:
            adl.AdaptiveDataParallel(model, optim, name="mw-refused")
        assert "float32" in str(err.value)
        assert "master_weights" in str(err.value)
    finally:
        adaptdl_amd.collective.teardown()


def test_unattached_warns_once_and_steps_like_torch(caplog):
    from adaptdl_amd.torch.optim import FusedSGD
    torch.manual_seed(60)
    model = torch.nn.Linear(4, 2).bfloat16()
    twin = torch.nn.Linear(4, 2).bfloat16()
    twin.load_state_dict(model.state_dict())
    optim = FusedSGD(model.parameters(), lr=0.1, master_weights=True)
    plain = torch.optim.SGD(twin.parameters(), lr=0.1)
    x = torch.randn(3, 4).bfloat16()
    with caplog.at_level(logging.WARNING, logger="adaptdl_amd.torch.optim"):
        for _ in range(2):
            for m, o in ((model, optim), (twin, plain)):
                o.zero_grad()
                m(x).float().sum().backward()
                o.step()
    warned = [r for r in caplog.records if "master_weights" in r.message]
    assert len(warned) == 1
    for p, q in zip(model.parameters(), twin.parameters()):
        assert torch.equal(p, q)
        assert "master_param" not in optim.state[p]


def test_cpu_ops_master_steps():
    """The torch fallbacks: fp32 math on the master, parameter = rounded
    master, gradient untouched."""
    from adaptdl_amd import ops
    torch.manual_seed(61)
    for dtype in LP_DTYPES:
        master = torch.randn(33)
        grad = torch.randn(33).to(dtype)
        grad0 = grad.clone()
        param = torch.zeros(33, dtype=dtype)
        ref = master.clone()
        m = torch.zeros(33)
        ops.fused_sgd_master_step(param, grad, master, m, 0.1, 0.9, 1e-4,
                                  0.0, False)
        ref_m = torch.zeros(33)
        ops.fused_sgd_step(ref, grad.float(), ref_m, 0.1, 0.9, 1e-4, 0.0,
                           False)
        assert torch.equal(master, ref) and torch.equal(m, ref_m)
        assert torch.equal(param, master.to(dtype))
        ea, eas = torch.zeros(33), torch.zeros(33)
        ops.fused_adamw_master_step(param, grad, master, ea, eas, 1e-3,
                                    0.9, 0.999, 1e-8, 0.01, 1, False)
        rea, reas = torch.zeros(33), torch.zeros(33)
        ops.fused_adamw_step(ref, grad.float(), rea, reas, 1e-3, 0.9,
                             0.999, 1e-8, 0.01, 1, False)
        assert torch.equal(master, ref)
        assert torch.equal(ea, rea) and torch.equal(eas, reas)
        assert torch.equal(param, master.to(dtype))
        assert torch.equal(grad, grad0)
        # Mixed-dtype preconditioned statistics (bf16/fp16 g, fp32 v).
        out = torch.zeros((), dtype=torch.float64)
        ops.precond_sqsum(grad, eas, 0.999, 1e-8, 7, out)
        pinv = (eas.double() / (1 - 0.999 ** 7)).sqrt() + 1e-8
        want = (grad.double() / pinv).pow(2).sum()
        assert torch.allclose(out, want, rtol=1e-12)
