"""Time the fused Adam(W) update passes at one 32 Mi-element bucket.

  k_fused_adamw_mw_bf16   bf16 p/g, fp32 master + moments (master weights)
  k_fused_adamw           fp32 p/g/moments (unchanged)
  torch.optim.AdamW(foreach=True) on a bf16 tensor of the same size

HIP events around ITERS back-to-back steps after WARMUP steps; the three
are timed alternately over ROUNDS rounds and the median round is kept.
Bytes are the streams each pass touches once per element:
  mw:    read g(2) w(4) m(4) v(4), write p(2) w(4) m(4) v(4) = 28 B
  fp32:  read p(4) g(4) m(4) v(4), write p(4) m(4) v(4)       = 28 B
  torch: foreach runs several passes over bf16 p/g/m/v; the figure given
         is the single-pass minimum (read 8 B, write 6 B = 14 B), so its
         GB/s is an effective rate, not achieved bandwidth.
Writes profiles/optim_master_weights.json (or the path given as argv[1]).
"""

import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from adaptdl_amd import ops  # noqa: E402

N = 32 * 1024 * 1024
WARMUP, ITERS, ROUNDS = 3, 20, 5
HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01)


def timed(fn):
    t0 = torch.cuda.Event(enable_timing=True)
    t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(ITERS):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / ITERS  # microseconds per step


def main():
    assert torch.cuda.is_available(), "optim_time.py needs the GPU"
    assert ops.has_extension()
    dev = torch.device("cuda")
    torch.manual_seed(0)
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(
        ROOT, "profiles", "optim_master_weights.json")

    g32 = torch.randn(N, device=dev)
    p32 = torch.randn(N, device=dev)
    m32, v32 = torch.zeros(N, device=dev), torch.zeros(N, device=dev)
    g16 = g32.bfloat16()
    w = p32.clone()
    p16 = torch.empty(N, device=dev, dtype=torch.bfloat16)
    m, v = torch.zeros(N, device=dev), torch.zeros(N, device=dev)
    pt = torch.nn.Parameter(p32.bfloat16())
    pt.grad = g16.clone()
    topt = torch.optim.AdamW([pt], lr=HYPER["lr"], betas=(0.9, 0.999),
                             eps=HYPER["eps"],
                             weight_decay=HYPER["weight_decay"],
                             foreach=True)

    def step_mw():
        ops.fused_adamw_master_step(
            p16, g16, w, m, v, HYPER["lr"], HYPER["beta1"], HYPER["beta2"],
            HYPER["eps"], HYPER["weight_decay"], 10, False)

    def step_f32():
        ops.fused_adamw_step(
            p32, g32, m32, v32, HYPER["lr"], HYPER["beta1"],
            HYPER["beta2"], HYPER["eps"], HYPER["weight_decay"], 10, False)

    passes = [("k_fused_adamw_mw_bf16", step_mw, 28),
              ("k_fused_adamw", step_f32, 28),
              ("torch_adamw_foreach_bf16", topt.step, 14)]
    for _, fn, _ in passes:
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
    samples = {name: [] for name, _, _ in passes}
    for _ in range(ROUNDS):
        for name, fn, _ in passes:
            samples[name].append(timed(fn))

    result = {"elements": N, "warmup": WARMUP, "iters_per_round": ITERS,
              "rounds": ROUNDS, "device": torch.cuda.get_device_name(0),
              "passes": {}}
    for name, _, bpe in passes:
        us = statistics.median(samples[name])
        result["passes"][name] = {
            "us": round(us, 1),
            "us_min": round(min(samples[name]), 1),
            "us_max": round(max(samples[name]), 1),
            "bytes_per_element": bpe,
            "gb_per_s": round(N * bpe / us / 1e3, 1),
        }
        print("{:28s} {:9.1f} us  {:7.1f} GB/s  ({} B/elem)".format(
            name, us, result["passes"][name]["gb_per_s"], bpe))
    result["passes"]["torch_adamw_foreach_bf16"]["note"] = \
        "effective rate over the single-pass minimum bytes"
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
