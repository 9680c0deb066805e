"""CPU simulations of the HIP conv kernels' index math.

Each test mirrors the exact staging layout, tap decode, and store
mapping of a kernel in adaptdl_amd/ops/hip/conv_kernels.hip and checks
it against torch's reference op in fp32.  They run without a GPU, so a
refactor that breaks the polyphase index math fails here before it
costs GPU time (the bf16 numerics themselves are covered by the
@gpu tests in test_fused_conv.py).

The second half models the kernels' software-pipelined chunk LOOPS
(prefetch registers, two LDS buffers, bounce stores through the staging
buffer) and runs the layouts through them on dyadic data, where the
comparison with the float64 reference is exact; the same exact
comparison runs on the GPU in test_gpu_conv_exact.py.
"""

import pytest
import torch


def test_s2_bwd_polyphase_decomposition():
    """k_conv3x3_s2_bwd: phase tap sets, dy window, store interleave."""
    torch.manual_seed(0)
    N, Ho, Wo, K, C, P2 = 2, 16, 16, 32, 32, 2
    Hi, Wi = 2 * Ho, 2 * Wo
    dy = torch.randn(N, Ho, Wo, K)
    w = torch.randn(K, C, 3, 3)
    ref = torch.nn.grad.conv2d_input(
        (N, C, Hi, Wi), w, dy.permute(0, 3, 1, 2), stride=2,
        padding=1).permute(0, 2, 3, 1)
    wt = w.permute(1, 2, 3, 0).reshape(C, 9, K)
    dx = torch.zeros(N, Hi, Wi, C)
    for n in range(N):
        for r0 in range(0, Ho, P2):
            win = torch.zeros(P2 + 1, Wo + 8, K)
            for j in range(P2 + 1):
                if r0 + j < Ho:
                    win[j, :Wo] = dy[n, r0 + j]
            stage = torch.zeros(4, P2, Wo, C)
            for ph in range(4):
                a, b = ph >> 1, ph & 1
                for h2 in range(P2):
                    for dh in ((0, 2) if a else (1,)):
                        for dw in ((0, 2) if b else (1,)):
                            j = h2 + (1 if dh == 0 else 0)
                            off = 1 if dw == 0 else 0
                            seg = win[j, off:off + Wo]
                            stage[ph, h2] += seg @ wt[:, dh * 3 + dw].t()
            for hl in range(2 * P2):
                for wi in range(Wi):
                    phc = ((hl & 1) << 1) | (wi & 1)
                    dx[n, 2 * r0 + hl, wi] = stage[phc, hl >> 1, wi >> 1]
    assert (dx - ref).abs().max().item() < 1e-3


def test_s2_fwd_eo_staging():
    """k_conv3x3_s2_fwd: E|z|O column-split staging + per-lane taps."""
    torch.manual_seed(2)
    N, H, W, C, K, P2 = 2, 16, 32, 16, 8, 4
    Ho, Wo = H // 2, W // 2
    x = torch.randn(N, H, W, C)
    w = torch.randn(K, C, 3, 3)
    ref = torch.nn.functional.conv2d(
        x.permute(0, 3, 1, 2), w, stride=2, padding=1).permute(0, 2, 3, 1)
    wt = w.permute(0, 2, 3, 1).reshape(K, 9, C)
    LS2 = 2 * Wo + 2
    y = torch.zeros(N, Ho, Wo, K)
    for n in range(N):
        for r0 in range(0, Ho, P2):
            xs = torch.zeros(2 * P2 + 1, LS2, C)
            for j in range(2 * P2 + 1):
                h = 2 * r0 - 1 + j
                if 0 <= h < H:
                    for wcol in range(W):
                        slot = (Wo + 1 + wcol // 2) if wcol % 2 \
                            else wcol // 2
                        xs[j, slot] = x[n, h, wcol]
            for ho_loc in range(P2):
                for wo in range(Wo):
                    acc = torch.zeros(K)
                    for dh in range(3):
                        for dw in range(3):
                            L = 2 * ho_loc + dh
                            slot = wo if dw == 1 else \
                                Wo + 1 + wo - (1 if dw == 0 else 0)
                            acc += wt[:, dh * 3 + dw] @ xs[L, slot]
                    y[n, r0 + ho_loc, wo] = acc
    assert (y - ref).abs().max().item() < 2e-3


def test_s2_wrw_polyphase_window():
    """k_conv3x3_s2_wrw: E|pad|O rows, window taps, dW accumulation."""
    torch.manual_seed(3)
    N, Ho, Wo, C, K, P = 2, 8, 8, 16, 8, 4
    Hi, Wi = 2 * Ho, 2 * Wo
    x = torch.randn(N, Hi, Wi, C)
    dy = torch.randn(N, Ho, Wo, K)
    xg = x.permute(0, 3, 1, 2).requires_grad_(True)
    w0 = torch.zeros(K, C, 3, 3, requires_grad=True)
    torch.nn.functional.conv2d(xg, w0, stride=2, padding=1) \
        .backward(dy.permute(0, 3, 1, 2))
    ref = w0.grad
    LS2 = 2 * Wo + 8
    dW = torch.zeros(K, 3, 3, C)
    for n in range(N):
        for lo0 in range(0, Ho, P):
            xt = torch.zeros(2 * P + 1, LS2, C)
            for j in range(2 * P + 1):
                h = 2 * lo0 - 1 + j
                if 0 <= h < Hi:
                    for wcol in range(Wi):
                        col = (Wo + 4 + (wcol - 1) // 2) if wcol % 2 \
                            else wcol // 2
                        xt[j, col] = x[n, h, wcol]
            for li in range(P):
                for wo in range(Wo):
                    for dh in range(3):
                        row = xt[2 * li + dh]
                        for dw in range(3):
                            if dw == 1:
                                v = row[wo]
                            else:
                                # O window: j = wo-1 (dw=0) or wo (dw=2);
                                # j = -1 hits the zeroed col Wo+3
                                j = wo - 1 if dw == 0 else wo
                                v = row[Wo + 4 + j]
                            dW[:, dh, dw] += torch.outer(
                                dy[n, lo0 + li, wo], v)
    err = (dW.permute(0, 3, 1, 2) - ref).abs().max().item()
    assert err < 1e-3, err


def test_w8b_wave_mapping():
    """k_conv3x3_s2_bwd_w8b: frag-quad coverage, one atomicAdd per
    k-quarter, invertible store mapping."""
    P2, Wo, CT = 4, 8, 16
    writes = {}
    for wid in range(8):
        wg2, kq = wid >> 2, wid & 3
        for fi in range(4):
            pha, phb = (0, 3) if wg2 == 0 else (1, 2)
            ph = phb if fi >> 1 else pha
            f = fi & 1
            for lane in range(64):
                for r in range(4):
                    m = (lane >> 4) * 4 + r
                    key = (ph, 2 * f + (m >> 3), m & 7, lane & 15)
                    writes.setdefault(key, []).append(kq)
    assert len(writes) == 4 * P2 * Wo * CT
    assert all(sorted(v) == [0, 1, 2, 3] for v in writes.values())
    for hl in range(2 * P2):
        for wi in range(2 * Wo):
            ph = ((hl & 1) << 1) | (wi & 1)
            s = (ph * P2 + (hl >> 1)) * Wo + (wi >> 1)
            ph2, rem = divmod(s, P2 * Wo)
            assert (ph2, rem // Wo, rem % Wo) == (ph, hl >> 1, wi >> 1)


def _wrw_params(W):
    """Mirror of conv3x3_wrw_params (conv_kernels.hip)."""
    table = {8: (8, 8), 16: (8, 16), 32: (4, 32),
             56: (1, 64), 28: (4, 32), 14: (8, 16), 7: (8, 8)}
    P, Wp = table[W]
    return P, Wp


def _wrw_loop(total, nsplit, split, issue, write, consume, defect=None):
    """Loop schedule of k_conv3x3_wrw for one block (branch structure
    copied from the kernel).  issue(q) returns what the global loads of
    chunk q leave in the prefetch registers, write(buf, regs) commits
    them to LDS buffer `buf`, consume(q, buf) is the MFMA phase of
    chunk q reading buffer `buf`.  `defect` injects a schedule bug."""
    regs = None
    # Prologue: stage chunk 0 into buffer 0, issue chunk 1's loads.
    if split < total:
        regs = issue(split)
        write(0, regs)
    if split + nsplit < total:
        regs = issue(split + nsplit)
    cur = 0
    q = split
    while q < total:
        consume(q, cur)
        if q + nsplit < total:
            write(cur ^ 1, regs)
            if q + 2 * nsplit < total and defect != "skip_issue2":
                regs = issue(q + 2 * nsplit)
        q += nsplit
        if defect != "no_flip":
            cur ^= 1


def _mm_loop(total, spread, sp, dbuf, issue, write, consume, defect=None):
    """Loop schedule shared by k_conv3x3_mm and k_conv3x3_s2_bwd(_w8):
    two LDS buffers when dbuf, else one buffer with the next chunk held
    in registers through the contraction.  consume(q, buf) stands for
    the contraction AND the bounce store through buffer `buf`."""
    regs = None
    if sp < total:
        regs = issue(sp)
        write(0, regs)
    if sp + spread < total:
        regs = issue(sp + spread)
    cur = 0
    q = sp
    while q < total:
        buf = 1 if (dbuf and cur) else 0
        if not dbuf and q != sp:
            write(0, regs)
            if q + spread < total:
                regs = issue(q + spread)
        consume(q, buf)
        if dbuf:
            if q + spread < total:
                write(buf ^ 1, regs)
                if q + 2 * spread < total and defect != "skip_issue2":
                    regs = issue(q + 2 * spread)
            if defect != "no_flip":
                cur ^= 1
        q += spread


def _trace(loop, *args, **kwargs):
    """Run a schedule on chunk ids alone: [(chunk consumed, buffer read,
    chunk that buffer holds at that moment)]."""
    held = {}
    events = []
    loop(*args, issue=lambda q: q,
         write=lambda buf, regs: held.__setitem__(buf, regs),
         consume=lambda q, buf: events.append((q, buf, held.get(buf))),
         **kwargs)
    return events


def test_pipeline_schedules_consume_each_chunk_once():
    """Every chunk q == split (mod nsplit) is consumed exactly once, in
    order, from the buffer that holds it; no other chunk is consumed."""
    for total in range(8):
        for nsplit in range(1, 5):
            for split in range(nsplit):
                want = list(range(split, total, nsplit))
                ev = _trace(_wrw_loop, total, nsplit, split)
                assert [e[0] for e in ev] == want, (total, nsplit, split)
                assert all(e[2] == e[0] for e in ev), ev
                # the wrw kernel alternates buffers from buffer 0
                assert [e[1] for e in ev] == [i & 1 for i in
                                              range(len(ev))]
                for dbuf in (1, 0):
                    ev = _trace(_mm_loop, total, nsplit, split, dbuf)
                    assert [e[0] for e in ev] == want, \
                        (total, nsplit, split, dbuf)
                    assert all(e[2] == e[0] for e in ev), ev
                    assert [e[1] for e in ev] == \
                        [(i & 1) if dbuf else 0 for i in range(len(ev))]


def test_pipeline_schedule_defects_are_visible():
    """The two schedule defects change what a 3-trip block consumes."""
    for loop, extra in ((_wrw_loop, ()), (_mm_loop, (1,))):
        for defect in ("skip_issue2", "no_flip"):
            ev = _trace(loop, 5, 2, 0, *extra, defect=defect)
            assert [e[0] for e in ev] == [0, 2, 4]
            assert any(e[2] != e[0] for e in ev), (loop, defect, ev)


def _dyadic(gen, *shape):
    """Uniform on {k/4 : |k| <= 8}: exact in bf16, and every sum of T
    products is an exact multiple of 1/16 in fp32 while 64 T < 2**24 --
    so results do not depend on the order of accumulation."""
    return torch.randint(-8, 9, shape, generator=gen).double() / 4


def _simulate_wrw(x, dy, P, Wp, nsplit=1, defect=None):
    """CPU mirror of k_conv3x3_wrw: the padded-width chunking run
    through the kernel's software pipeline (_wrw_loop), one block per
    split, slabs summed at the end.  dy pixels with w >= W or h >= H
    stage zero; the tap read for dy pixel (li, w) and offset (dh, dw) is
    x_pad[li + dh][3 + w + dw] in the LS-padded line layout (4 left
    zeros).  The global loads fetch pixel PAIRS (w, w + 1): with
    defect="no_w_guard" the odd pixel is loaded without its w + 1 < W
    check and picks up whatever follows the line in memory."""
    N, H, W, C = x.shape
    K = dy.shape[3]
    LS = Wp + 8
    lines = -(-H // P)
    total = N * lines
    xf, dyf = x.reshape(-1, C), dy.reshape(-1, K)

    def after_line(flat, n, h):
        i = (n * H + h) * W + W
        return flat[i] if i < flat.shape[0] else 0.0

    def issue(q):
        n, h0 = q // lines, (q % lines) * P
        x_pad = torch.zeros(P + 2, LS, C, dtype=x.dtype)
        for j in range(P + 2):
            h = h0 - 1 + j
            if 0 <= h < H:
                x_pad[j, 4:4 + W] = x[n, h]
                if defect == "no_w_guard" and W % 2:
                    x_pad[j, 4 + W] = after_line(xf, n, h)
        dy_pad = torch.zeros(P, Wp, K, dtype=x.dtype)
        for li in range(P):
            h = h0 + li
            if h < H:
                dy_pad[li, :W] = dy[n, h]
                if defect == "no_w_guard" and W % 2:
                    dy_pad[li, W] = after_line(dyf, n, h)
        return x_pad, dy_pad

    lds = {}
    slabs = torch.zeros(nsplit, K, 9, C, dtype=x.dtype)

    def write(buf, regs):
        lds[buf] = regs

    for split in range(nsplit):
        def consume(q, buf):
            x_pad, dy_pad = lds[buf]
            for dh in range(3):
                for dwo in range(3):
                    # x cols for w = 0..Wp-1 at this tap
                    cols = torch.arange(Wp) + 3 + dwo
                    xt = x_pad[dh:dh + P, cols]     # (P, Wp, C)
                    slabs[split, :, dh * 3 + dwo] += torch.einsum(
                        "pwk,pwc->kc", dy_pad, xt)
        lds.clear()
        _wrw_loop(total, nsplit, split, issue, write, consume,
                  defect=defect)
    return slabs.sum(0)


def test_wrw_padded_width_chunking():
    """k_conv3x3_wrw generalized chunking vs torch conv2d_weight for the
    ImageNet-resolution widths (ResNet-50 at 224) and a legacy width."""
    torch.manual_seed(1)
    for (H, W, C, K, N) in [(7, 7, 64, 64, 2), (14, 14, 64, 64, 2),
                            (28, 28, 64, 64, 1), (56, 56, 64, 64, 1),
                            (16, 16, 64, 64, 2)]:
        P, Wp = _wrw_params(W)
        x = torch.randn(N, H, W, C)
        dy = torch.randn(N, H, W, K)
        got = _simulate_wrw(x, dy, P, Wp)
        ref = torch.nn.grad.conv2d_weight(
            x.permute(0, 3, 1, 2), (K, C, 3, 3),
            dy.permute(0, 3, 1, 2), stride=1, padding=1)
        ref = ref.permute(0, 2, 3, 1).reshape(K, 9, C)
        assert torch.allclose(got, ref, rtol=1e-4, atol=1e-3), (H, W)


def _ref_wrw(x, dy):
    """float64 conv2d_weight of NHWC x, dy as (K, 9, C)."""
    K, C = dy.shape[3], x.shape[3]
    ref = torch.nn.grad.conv2d_weight(
        x.permute(0, 3, 1, 2), (K, C, 3, 3), dy.permute(0, 3, 1, 2),
        stride=1, padding=1)
    return ref.permute(0, 2, 3, 1).reshape(K, 9, C)


def _wrw_case(W, N=5, C=8, K=8, seed=11):
    gen = torch.Generator().manual_seed(seed)
    H = W
    x, dy = _dyadic(gen, N, H, W, C), _dyadic(gen, N, H, W, K)
    assert 16 * 4 * N * H * W < 2 ** 24      # exact in fp32 too
    return x, dy, _ref_wrw(x, dy)


def test_wrw_pipeline_exact_on_dyadic_data():
    """_simulate_wrw through the 3/2-trip schedule (5 chunks over 2
    splits) equals the fp64 conv2d_weight EXACTLY on dyadic data, at a
    legacy width, a padded odd width with a tail chunk, and P < H."""
    for W in (8, 7, 32):
        P, Wp = _wrw_params(W)
        x, dy, ref = _wrw_case(W, N=5 if W < 32 else 1)
        total = x.shape[0] * -(-W // P)
        nsplit = 2 if W < 32 else 3
        trips = {len(range(s, total, nsplit)) for s in range(nsplit)}
        assert trips == {3, 2}, (W, trips)
        assert torch.equal(_simulate_wrw(x, dy, P, Wp, nsplit), ref), W


def test_wrw_exact_comparison_catches_injected_defects():
    """Each defect injected into the MODEL makes the exact comparison
    fail, so the same comparison on the GPU has teeth."""
    P, Wp = _wrw_params(7)
    x, dy, ref = _wrw_case(7)
    assert torch.equal(_simulate_wrw(x, dy, P, Wp, 2), ref)
    for defect in ("skip_issue2", "no_flip", "no_w_guard"):
        with pytest.raises(AssertionError):
            assert torch.equal(
                _simulate_wrw(x, dy, P, Wp, 2, defect=defect), ref), defect


def _simulate_s2_bwd(dy, w, spread, dbuf, defect=None):
    """CPU mirror of k_conv3x3_s2_bwd (Wo = 16, P2 = 2, CT = 32) run
    through _mm_loop with the LDS dy window as FLAT memory, so the dx
    bounce store clobbers it exactly where the kernel's does and
    s2_write's refresh of the zero pad columns matters.
    defect="no_rezero" zeroes the pad columns once instead."""
    N, Ho, Wo, K = dy.shape
    C = w.shape[1]
    P2, CT, KS, LW = 2, 32, K + 16, Wo + 8
    assert Wo == 16 and Ho % P2 == 0 and C % CT == 0
    # the bounce stage [4 * P2 * Wo][CT] must fit the window
    assert 4 * P2 * Wo * CT <= (P2 + 1) * LW * KS
    Hi, Wi = 2 * Ho, 2 * Wo
    rows = Ho // P2
    total = N * rows
    dx = torch.full((N, Hi, Wi, C), float("nan"), dtype=dy.dtype)

    def issue(q):
        n, r0 = q // rows, (q % rows) * P2
        win = torch.zeros(P2 + 1, Wo, K, dtype=dy.dtype)
        for j in range(P2 + 1):
            if r0 + j < Ho:
                win[j] = dy[n, r0 + j]
        return win

    for ct in range(C // CT):
        wt = w[:, ct * CT:(ct + 1) * CT].permute(1, 2, 3, 0) \
            .reshape(CT, 9, K)
        for sp in range(spread):
            lds = torch.zeros(2, (P2 + 1) * LW * KS, dtype=dy.dtype)

            def write(buf, regs):
                view = lds[buf].view(P2 + 1, LW, KS)
                view[:, :Wo, :K] = regs
                if defect != "no_rezero":
                    view[:, Wo:, :K] = 0

            def consume(q, buf):
                n, r0 = q // rows, (q % rows) * P2
                view = lds[buf].view(P2 + 1, LW, KS)
                stage = torch.zeros(4, P2, Wo, CT, dtype=dy.dtype)
                for ph in range(4):
                    a, b = ph >> 1, ph & 1
                    for h2 in range(P2):
                        for dh in ((0, 2) if a else (1,)):
                            for dwo in ((0, 2) if b else (1,)):
                                j = h2 + (1 if dh == 0 else 0)
                                off = 1 if dwo == 0 else 0
                                seg = view[j, off:off + Wo, :K]
                                stage[ph, h2] += \
                                    seg @ wt[:, dh * 3 + dwo].t()
                # bounce: ystage[s * CT + c] over the start of dy_s
                lds[buf][:stage.numel()] = stage.reshape(-1)
                ystage = lds[buf][:stage.numel()].view(4, P2, Wo, CT)
                for hl in range(2 * P2):
                    for wi in range(Wi):
                        phc = ((hl & 1) << 1) | (wi & 1)
                        dx[n, 2 * r0 + hl, wi, ct * CT:(ct + 1) * CT] = \
                            ystage[phc, hl >> 1, wi >> 1]

            _mm_loop(total, spread, sp, dbuf, issue, write, consume,
                     defect=defect if defect != "no_rezero" else None)
    return dx


def _simulate_conv_mm(x, w, spread, dbuf, defect=None):
    """CPU mirror of k_conv3x3_mm (W = 16, P = 8, KT = 64) through
    _mm_loop, x window and y bounce stage in the same flat memory."""
    N, H, W, C = x.shape
    K = w.shape[0]
    P, KT, CS, LP = 8, 64, C + 16, W + 2
    assert W == 16 and H % P == 0 and K % KT == 0 and C <= 64
    QR = (P + 2) * LP
    assert P * W * KT <= QR * CS
    lines = H // P
    total = N * lines
    y = torch.full((N, H, W, K), float("nan"), dtype=x.dtype)

    def issue(q):
        n, h0 = q // lines, (q % lines) * P
        win = torch.zeros(P + 2, W, C, dtype=x.dtype)
        for j in range(P + 2):
            h = h0 - 1 + j
            if 0 <= h < H:
                win[j] = x[n, h]
        return win

    for kt in range(K // KT):
        wk = w[kt * KT:(kt + 1) * KT]            # (KT, C, 3, 3)
        for sp in range(spread):
            lds = torch.zeros(2, QR * CS, dtype=x.dtype)

            def write(buf, regs):
                view = lds[buf].view(P + 2, LP, CS)
                view[:, 1:W + 1, :C] = regs
                if defect != "no_rezero":
                    view[:, 0, :C] = 0
                    view[:, W + 1, :C] = 0

            def consume(q, buf):
                n, h0 = q // lines, (q % lines) * P
                view = lds[buf].view(P + 2, LP, CS)
                acc = torch.zeros(P, W, KT, dtype=x.dtype)
                for dh in range(3):
                    for dwo in range(3):
                        acc += view[dh:dh + P, dwo:dwo + W, :C] \
                            @ wk[:, :, dh, dwo].t()
                lds[buf][:acc.numel()] = acc.reshape(-1)   # bounce
                y[n, h0:h0 + P, :, kt * KT:(kt + 1) * KT] = \
                    lds[buf][:acc.numel()].view(P, W, KT)

            _mm_loop(total, spread, sp, dbuf, issue, write, consume,
                     defect=defect if defect != "no_rezero" else None)
    return y


def _s2_case():
    gen = torch.Generator().manual_seed(12)
    N, Ho, Wo, K, C = 5, 2, 16, 64, 32        # 5 chunks
    dy, w = _dyadic(gen, N, Ho, Wo, K), _dyadic(gen, K, C, 3, 3)
    assert 16 * 4 * 4 * K < 2 ** 24
    ref = torch.nn.grad.conv2d_input(
        (N, C, 2 * Ho, 2 * Wo), w, dy.permute(0, 3, 1, 2), stride=2,
        padding=1).permute(0, 2, 3, 1)
    return dy, w, ref


def _mm_case():
    gen = torch.Generator().manual_seed(13)
    N, H, W, C, K = 5, 8, 16, 32, 64          # 5 chunks
    x, w = _dyadic(gen, N, H, W, C), _dyadic(gen, K, C, 3, 3)
    assert 16 * 4 * 9 * C < 2 ** 24
    ref = torch.nn.functional.conv2d(
        x.permute(0, 3, 1, 2), w, padding=1).permute(0, 2, 3, 1)
    return x, w, ref


def test_s2_bwd_and_conv_mm_pipelines_exact_on_dyadic_data():
    """Both bounce-store kernels, double- and single-buffered, at 3/2
    trips (5 chunks spread over 2 blocks), equal fp64 exactly."""
    dy, w, ref = _s2_case()
    x, wm, refm = _mm_case()
    for dbuf in (1, 0):
        assert torch.equal(_simulate_s2_bwd(dy, w, 2, dbuf), ref), dbuf
        assert torch.equal(_simulate_conv_mm(x, wm, 2, dbuf), refm), dbuf


def test_bounce_kernels_exact_comparison_catches_injected_defects():
    """Pad columns zeroed once and never refreshed after the bounce
    store clobbered them (what k_conv3x3_mm did before mm_write
    refreshed them), and the two schedule defects, all fail the exact
    comparison.  Stale pads show from the 2nd trip single-buffered and
    from the 3rd double-buffered."""
    dy, w, ref = _s2_case()
    x, wm, refm = _mm_case()
    for defect, dbufs in (("no_rezero", (1, 0)), ("skip_issue2", (1,)),
                          ("no_flip", (1,))):
        for dbuf in dbufs:
            with pytest.raises(AssertionError):
                assert torch.equal(
                    _simulate_s2_bwd(dy, w, 2, dbuf, defect=defect), ref)
            with pytest.raises(AssertionError):
                assert torch.equal(
                    _simulate_conv_mm(x, wm, 2, dbuf, defect=defect),
                    refm)
