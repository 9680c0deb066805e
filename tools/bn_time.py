"""Per-shape timer for the fused NHWC BatchNorm(+ReLU) kernels.

Times forward and backward of layers._FusedBNFunction (training mode,
relu on) at the flagship ResNet-18/CIFAR BN shapes, each with and
without a residual:

  C=64 32x32, C=128 16x16, C=256 8x8, C=512 4x4 at N=1024 (one
  microbatch) and at N=128 (the init batch).

ITERS back-to-back calls are captured into one hipGraph (the flagship
replays a graph, so launches are back to back with no host gaps) and the
replay is timed with HIP events; ROUNDS rounds after WARMUP replays, the
median round is reported.  Forward = reduce + tail + apply, backward the
same three; launches per call are counted from a torch.profiler trace of
one eager call (null if the profiler sees no kernels).

Bytes are the streams each direction touches once per element (bf16 = 2 B
per element, M*C elements):
  forward   reduce reads x; apply reads x [+ z], writes y [+ mask]
  backward  reduce reads x, dy [+ z or mask]; apply reads the same and
            writes dx [+ dz]
The saved ReLU bitmask is M*C/8 bytes; whether a call uses one is read
off the tensors the forward saved, so the same script times trees with
and without it.  The per-channel vectors and the partials workspace are
left out (< 1 % of the bytes at N=1024).

Prints one JSON document; also writes it to the path given as argv[1].
"""

import inspect
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from adaptdl_amd import ops  # noqa: E402
from adaptdl_amd.torch.layers import _FusedBNFunction  # noqa: E402

SHAPES = [(n, c, hw, hw) for n in (1024, 128)
          for c, hw in ((64, 32), (128, 16), (256, 8), (512, 4))]
WARMUP, ITERS, ROUNDS = 3, 20, 5


class _Ctx:
    """Stand-in for the autograd context: every input needs a gradient."""
    needs_input_grad = (True, True, True, True) + (False,) * 8

    def save_for_backward(self, *tensors):
        self.saved_tensors = tensors


def _graph_us(fn):
    """Median/min/max microseconds per call of fn over ROUNDS replays."""
    fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(ITERS):
            fn()
    for _ in range(WARMUP):
        graph.replay()
    torch.cuda.synchronize()
    samples = []
    for _ in range(ROUNDS):
        t0 = torch.cuda.Event(enable_timing=True)
        t1 = torch.cuda.Event(enable_timing=True)
        t0.record()
        graph.replay()
        t1.record()
        torch.cuda.synchronize()
        samples.append(t0.elapsed_time(t1) * 1e3 / ITERS)
    return statistics.median(samples), min(samples), max(samples)


def _launches(fn):
    try:
        from torch.profiler import profile, ProfilerActivity
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events()
                if str(e.device_type).endswith("CUDA")
                and "memcpy" not in e.name.lower()
                and "memset" not in e.name.lower())
        return n or None
    except Exception:  # profiler backend not available
        return None


def time_shape(shape, residual):
    n, c, h, w = shape
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)

    def rand():
        return torch.randn(n, c, h, w, device=dev, generator=gen) \
            .to(torch.bfloat16).contiguous(memory_format=torch.channels_last)

    x, dy = rand(), rand()
    z = rand() if residual else None
    weight = torch.rand(c, device=dev, generator=gen) + 0.5
    bias = torch.randn(c, device=dev, generator=gen)
    rm = torch.zeros(c, device=dev)
    rv = torch.ones(c, device=dev)
    ctx = _Ctx()
    # trees with the saved ReLU mask take (num_batches_tracked, save_mask)
    params = inspect.signature(_FusedBNFunction.forward).parameters
    extra = (None, True) if "save_mask" in params else ()

    def fwd():
        return _FusedBNFunction.forward(ctx, x, z, weight, bias, rm, rv,
                                        True, 0.1, 1e-5, True, *extra)

    def bwd():
        return _FusedBNFunction.backward(ctx, dy)

    fwd()
    has_mask = any(t.dtype == torch.uint8 and t.numel() > 0
                   for t in ctx.saved_tensors)
    elems = n * h * w * c
    mask_b = elems // 8 if has_mask else 0
    zin = 2 * elems if residual else 0
    zbwd = mask_b if has_mask else zin
    fwd_bytes = 2 * elems + (2 * elems + zin) + 2 * elems + mask_b
    bwd_bytes = 2 * (4 * elems + zbwd) + 2 * elems + \
        (2 * elems if residual else 0)

    out = {"shape": list(shape), "residual": residual, "relu": True,
           "saved_mask": has_mask}
    for name, fn, nbytes in (("forward", fwd, fwd_bytes),
                             ("backward", bwd, bwd_bytes)):
        us, lo, hi = _graph_us(fn)
        out[name] = {"us": round(us, 2), "us_min": round(lo, 2),
                     "us_max": round(hi, 2), "launches": _launches(fn),
                     "bytes": nbytes,
                     "gb_per_s": round(nbytes / us / 1e3, 1)}
    return out


def main():
    assert torch.cuda.is_available(), "bn_time.py needs the GPU"
    assert ops.has_extension()
    result = {"device": torch.cuda.get_device_name(0), "warmup": WARMUP,
              "iters_per_round": ITERS, "rounds": ROUNDS, "timing":
              "hipGraph replay of ITERS back-to-back calls, HIP events",
              "cases": []}
    for shape in SHAPES:
        for residual in (False, True):
            case = time_shape(shape, residual)
            result["cases"].append(case)
            print("N{:5d} C{:4d} {:2d}x{:<2d} res={:d}  fwd {:8.2f} us "
                  "{:7.1f} GB/s   bwd {:8.2f} us {:7.1f} GB/s".format(
                      shape[0], shape[1], shape[2], shape[3], residual,
                      case["forward"]["us"], case["forward"]["gb_per_s"],
                      case["backward"]["us"], case["backward"]["gb_per_s"]),
                  file=sys.stderr)
    text = json.dumps(result, indent=1, sort_keys=True)
    print(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])),
                    exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
