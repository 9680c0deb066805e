import torch, sys
sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
from adaptdl_amd import ops
ext = ops._load_extension()
dev = torch.device("cuda")
shapes = [(1024, 64, 32, 32, 64), (1024, 128, 16, 16, 128), (1024, 256, 8, 8, 256),
          # ImageNet-resolution (ResNet-50 at 224) padded-width shapes
          (256, 64, 56, 56, 64), (256, 128, 28, 28, 128),
          (256, 256, 14, 14, 256), (256, 512, 7, 7, 512),
          # CIFAR layer4 (ResNet-18/34): k_conv3x3_wrw_w4
          (1024, 512, 4, 4, 512), (1024, 256, 4, 4, 256)]
# k_conv1x1_wrw (n, c, h, w, k, stride): the flagship's stride-2 shortcuts
# and ResNet-50 at 224
shapes_1x1 = [(1024, 64, 32, 32, 128, 2), (1024, 128, 16, 16, 256, 2),
              (1024, 256, 8, 8, 512, 2),
              (256, 64, 56, 56, 256, 1), (256, 256, 56, 56, 64, 1),
              (256, 512, 28, 28, 128, 1), (256, 1024, 14, 14, 256, 1),
              (256, 2048, 7, 7, 512, 1)]


def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = torch.cuda.Event(enable_timing=True); t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(10):
        fn()
    t1.record(); torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 100


def rel_err(got, ref):
    return ((got.double().cpu() - ref).abs().max() / ref.abs().max()).item()


if "1x1" in sys.argv[1:]:       # wrw_time.py 1x1: only the 1x1 shapes
    shapes = []
    torch.manual_seed(0)
    for i, (n, c, h, w, k, s) in enumerate(shapes_1x1):
        ho, wo = h // s, w // s
        x = torch.randn(n, c, h, w, device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        dy = torch.randn(n, k, ho, wo, device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        nsplit = ext.conv1x1_wrw_nsplit(n, ho, wo, c, k)
        ws = torch.empty(nsplit * k * c, dtype=torch.float32, device=dev)
        dw = torch.empty(k, c, 1, 1, dtype=torch.float32, device=dev)
        wt = torch.zeros(k, c, 1, 1, device=dev, dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
        lib = lambda: torch.ops.aten.convolution_backward(dy, x, wt, None, [s, s], [0, 0], [1, 1], False, [0, 0], 1, [False, True, False])[1]
        us = timed(lambda: ext.conv1x1_wrw(x, dy, ws, dw, s))
        us_m = timed(lib)
        gflop = 2 * n * k * c * ho * wo / 1e9
        print(f"shape1x1 N{n} C{c} {h}x{w} K{k} s{s}: ours {us:7.1f}us ({gflop/us*1e3:6.0f} GF/s)  miopen {us_m:7.1f}us ({gflop/us_m*1e3:6.0f} GF/s)  nsplit={nsplit}")
        if i == 6:              # error against float64, ours and the library's
            ref = torch.nn.grad.conv2d_weight(x.double().cpu(), (k, c, 1, 1), dy.double().cpu(), stride=s)
            print(f"  max|err|/max|dW| vs float64: ours {rel_err(dw, ref):.2e}  miopen {rel_err(lib(), ref):.2e}")
elif len(sys.argv) > 1:         # wrw_time.py W [W ...]: only these widths
    shapes = [s for s in shapes if str(s[3]) in sys.argv[1:]]
for n, c, h, w, k in shapes:
    x = torch.randn(n, c, h, w, device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    dy = torch.randn(n, k, h, w, device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    nsplit = ext.conv_wrw_nsplit(n, h, w, c, k)
    ws = torch.empty(nsplit * k * 9 * c, dtype=torch.float32, device=dev)
    dw = torch.empty(k, c, 3, 3, dtype=torch.float32, device=dev).contiguous(memory_format=torch.channels_last)
    for _ in range(3):
        ext.conv_wrw(x, dy, ws, dw)
    torch.cuda.synchronize()
    t0 = torch.cuda.Event(enable_timing=True); t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(10):
        ext.conv_wrw(x, dy, ws, dw)
    t1.record(); torch.cuda.synchronize()
    us = t0.elapsed_time(t1) * 100
    # MIOpen comparison
    x32 = x.float().requires_grad_(True)
    wt = torch.zeros(k, c, 3, 3, device=dev, dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    import torch.nn.functional as F
    for _ in range(3):
        gw = torch.ops.aten.convolution_backward(dy, x, wt, None, [1,1], [1,1], [1,1], False, [0,0], 1, [False, True, False])[1]
    torch.cuda.synchronize()
    t0.record()
    for _ in range(10):
        gw = torch.ops.aten.convolution_backward(dy, x, wt, None, [1,1], [1,1], [1,1], False, [0,0], 1, [False, True, False])[1]
    t1.record(); torch.cuda.synchronize()
    us_m = t0.elapsed_time(t1) * 100
    gflop = 2 * n * k * c * 9 * h * w / 1e9
    print(f"shape N{n} C{c} {h}x{w} K{k}: ours {us:7.1f}us ({gflop/us*1e3:6.0f} GF/s)  miopen {us_m:7.1f}us ({gflop/us_m*1e3:6.0f} GF/s)  nsplit={nsplit}")
