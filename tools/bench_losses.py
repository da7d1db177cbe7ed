"""Time one step of the two training losses (csrc/lpips_grad.hip, csrc/edge_loss.hip) at the training shape, 16 x 3 x 512x512 fp32
(relu maps 127 / 63 / 31), gradient w.r.t. the first operand only (the second is the ground truth: M = 16 gradient images).

Per launch, on preallocated operands, event-timed (median of `--repeats` windows of `--iters` calls: device time of one call with
its launch gaps; nothing is allocated or synchronised inside a window):
    keep            dc_lpips_alex_keep: the forward of both sides with the maps kept (13 launches)
    tail_grad l     the distance-tail gradient of layer l
    conv_dgrad l    the data gradient of conv(l + 1) on the fp32 MFMA, with TFLOP/s = 2 M H W Cout Cin k^2 / time, next to
    conv_fwd l      lpips.hip's forward convolution of the same layer and image count (dc_lpips_conv), the same FLOP count
    pool_grad, conv1_dgrad (2 M H W 3 . 64 . 121 / 16 FLOP per pixel on average: 121 taps over 16 phases)
    backward        dc_lpips_alex_backward, the whole chain (12 launches)
    step            NormFixLPIPS forward + backward through autograd (allocations and the Python dispatch included)
    torch_step      the same loss written with torch.nn.functional in fp32 on the same device, forward + backward by autograd
    sobel_*         SobelEdgeLoss forward ('mean') and its gradient w.r.t. pred; bytes = each operand read once, the gradient
                    written once, against `--hbm-tbs` (6.3 TB/s, the achievable streaming rate of the MI355X)
The stage operands are the device's own maps and random gradients: the kernels' time does not depend on the values.

    python tools/bench_losses.py [--iters 20] [--repeats 5]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

N, H, W = 16, 512, 512
CH, CIN, KS = (64, 192, 384, 256, 256), (3, 64, 192, 384, 256), (11, 5, 3, 3, 3)


def device_ms(fn, iters, repeats):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    windows = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        windows.append(e0.elapsed_time(e1) / iters)
    return statistics.median(windows), min(windows), max(windows)


def torch_lpips(sd, dev):
    """the NormFix loss with torch.nn.functional in fp32 (the rules of tests/lpips_ref.py), differentiable"""
    import lpips_ref as R
    convs = [(sd[f"net.slice{l + 1}.{p}.weight"].to(dev), sd[f"net.slice{l + 1}.{p}.bias"].to(dev)) for l, p in enumerate(R.POSITION)]
    lins = [sd[f"lin{l}.model.1.weight"].to(dev).view(1, -1, 1, 1) for l in range(5)]
    shift, scale = torch.tensor(R.SHIFT, device=dev).view(1, 3, 1, 1), torch.tensor(R.SCALE, device=dev).view(1, 3, 1, 1)

    def feats(x):
        x = (x - shift) / scale
        out = []
        for l, (w, b) in enumerate(convs):
            if l in (1, 2):
                x = F.max_pool2d(x, 3, 2)
            x = torch.relu(F.conv2d(x, w, b, stride=R.STRIDE[l], padding=R.PAD[l]))
            out.append(x)
        return out

    def loss(x, y):
        val = 0
        for a, b, w in zip(feats(x), feats(y), lins):
            ua = a / torch.sqrt((a * a + 1e-8).sum(1, keepdim=True))
            ub = b / torch.sqrt((b * b + 1e-8).sum(1, keepdim=True))
            val = val + (w * (ua - ub) ** 2).sum(1, keepdim=True).mean((2, 3), keepdim=True)
        return val
    return loss


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--hbm-tbs", type=float, default=6.3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_losses needs the GPU"
    import lpips_ref as R
    from diffcodec_amd import lib, losses
    from diffcodec_amd.metrics import lpips_map_sizes
    dev = torch.device("cuda")
    L = lib.load()
    st = torch.cuda.current_stream().cuda_stream
    sd = R.synth_weights(seed=20)
    model = losses.NormFixLPIPS.from_state_dict(sd).to(dev)
    wts, dwts = model._weights(dev), model._dgrad_weights(dev)
    gen = torch.Generator(device="cuda").manual_seed(0)
    x = torch.rand(N, 3, H, W, device=dev, generator=gen) * 2 - 1
    y = torch.rand(N, 3, H, W, device=dev, generator=gen) * 2 - 1
    sizes = lpips_map_sizes(H, W)
    rows = []

    def leg(name, fn, flops=0.0, nbytes=0.0, iters=None):
        ms, lo, hi = device_ms(fn, iters or a.iters, a.repeats)
        r = dict(leg=name, ms_per_call=round(ms, 4), ms_min=round(lo, 4), ms_max=round(hi, 4))
        if flops:
            r["tflops"] = round(flops / (ms * 1e-3) / 1e12, 2)
        if nbytes:
            r["tb_per_s"] = round(nbytes / (ms * 1e-3) / 1e12, 3)
            r["share_of_hbm"] = round(r["tb_per_s"] / a.hbm_tbs, 3)
        rows.append(r)
        print(json.dumps(r), flush=True)

    keep = torch.empty(L.dc_lpips_keep_ws_bytes(N, H, W), dtype=torch.uint8, device=dev)
    out = torch.empty(6 * N, dtype=torch.float64, device=dev)
    strides = (ctypes.c_longlong * 8)(*x.stride(), *y.stride())
    leg("keep", lambda: lib.call("dc_lpips_alex_keep", x.data_ptr(), y.data_ptr(), strides, N, H, W, 0, wts.data_ptr(), keep.data_ptr(),
                                 out.data_ptr(), st))
    maps = model.features(torch.cat([x, y]))                         # [2N] per layer, x first: dc_lpips_tail_grad's operand
    g = torch.rand(5, N, device=dev, generator=gen)
    d = [torch.randn(N, c, h, w, device=dev, generator=gen) * 1e-4 for c, (h, w) in zip(CH, sizes)]
    outs = [torch.empty_like(t) for t in d]
    pools = [torch.empty(N, 64, *sizes[1], device=dev), torch.empty(N, 192, *sizes[2], device=dev)]
    for l in range(5):
        h, w = sizes[l]
        leg(f"tail_grad {l}", lambda: lib.call("dc_lpips_tail_grad", l, maps[l].data_ptr(), N, h * w, 1, wts.data_ptr(), g[l].data_ptr(),
                                               outs[l].data_ptr(), st), nbytes=4.0 * N * CH[l] * h * w * 5)
    for l in (4, 3, 2, 1):
        h, w = sizes[l]
        flops = 2.0 * N * h * w * CH[l] * CIN[l] * KS[l] ** 2
        fused = l >= 3
        dst = outs[l - 1] if fused else pools[l - 1]
        leg(f"conv_dgrad {l}", lambda: lib.call("dc_lpips_conv_dgrad", l, d[l].data_ptr(), N, h, w, dwts.data_ptr(),
                                                outs[l - 1].data_ptr() if fused else None, maps[l - 1].data_ptr() if fused else None,
                                                dst.data_ptr(), st), flops=flops)
        src = maps[l - 1][:N] if fused else pools[l - 1]
        leg(f"conv_fwd {l}", lambda: lib.call("dc_lpips_conv", l, src.data_ptr(), 0, None, N, h, w, 0, wts.data_ptr(), outs[l].data_ptr(), st),
            flops=flops)
    for l in (1, 0):
        h, w = sizes[l]
        leg(f"pool_grad {l}", lambda: lib.call("dc_lpips_pool_grad", pools[l].data_ptr(), maps[l].data_ptr(), d[l].data_ptr(), N * CH[l], h, w,
                                               outs[l].data_ptr(), st), nbytes=4.0 * N * CH[l] * (3 * h * w + sizes[l + 1][0] * sizes[l + 1][1]))
    dx = torch.empty_like(x)
    leg("conv1_dgrad", lambda: lib.call("dc_lpips_conv1_dgrad", d[0].data_ptr(), N, N, H, W, 0, wts.data_ptr(), dx.data_ptr(), None, st),
        flops=2.0 * N * H * W * 3 * 64 * 121 / 16)
    ws = torch.empty(L.dc_lpips_train_ws_bytes(N, H, W, 1), dtype=torch.uint8, device=dev)
    leg("backward", lambda: lib.call("dc_lpips_alex_backward", keep.data_ptr(), g.data_ptr(), N, H, W, 0, 1, wts.data_ptr(), dwts.data_ptr(),
                                     ws.data_ptr(), dx.data_ptr(), None, st))

    xs = x.clone().requires_grad_(True)

    def step(fn):
        return lambda: torch.autograd.grad(fn(xs, y).mean(), xs)
    leg("step", step(model), iters=max(3, a.iters // 4))
    leg("torch_step", step(torch_lpips(sd, dev)), iters=max(3, a.iters // 4))

    edge = losses.SobelEdgeLoss()
    img = 4.0 * N * 3 * H * W
    acc, sws = torch.empty(1, dtype=torch.float64, device=dev), torch.empty(L.dc_sobel_edge_ws_bytes(N, 3, H, W), dtype=torch.uint8, device=dev)
    one = torch.ones(1, device=dev)
    leg("sobel_forward", lambda: lib.call("dc_sobel_edge_loss", x.data_ptr(), y.data_ptr(), strides, N, 3, H, W, 1, sws.data_ptr(), None,
                                          acc.data_ptr(), st), nbytes=2 * img)
    leg("sobel_grad", lambda: lib.call("dc_sobel_edge_grad", x.data_ptr(), y.data_ptr(), strides, N, 3, H, W, 0, one.data_ptr(), 0,
                                       1.0 / (N * 3 * H * W), dx.data_ptr(), st), nbytes=3 * img)
    leg("sobel_step", step(edge), iters=max(3, a.iters // 4))
    import loss_ref
    leg("torch_sobel_step", step(lambda p, t: loss_ref.sobel_edge_loss(p, t)), iters=max(3, a.iters // 4))


if __name__ == "__main__":
    main()
