"""Time the backward of the fp32 extractor convolution (csrc/conv_f32_grad.hip) on the production layers of a 512 x 512 frame with
Cin, Cout >= 32 (tests/conv_grad_ref.PRODUCTION_LAYERS) at batch 16, next to the same layer's forward launch in the same run and
to PyTorch's fp32 convolution on the same device.

Per launch, on preallocated operands, event-timed: median (and range) of `--repeats` windows of `--iters` calls = device time of
one call with its launch gap; nothing is allocated or synchronised inside a window.  TFLOP/s = 2 N Ho Wo Cout Cin 9 / time for
the forward, the data gradient and the weight gradient alike (the algorithm's count: at stride 2 the data gradient does the same
multiply-adds as the forward); the SiLU gradient is reported in TB/s of its three streams.
    fwd         dc_conv3x3_nchw_f32 without SiLU (the route's form is printed: every layer here takes the MFMA form)
    silu_grad   dc_silu_grad_f32 on the layer's output
    dgrad       dc_conv3x3_f32_dgrad
    wgrad       dc_conv3x3_f32_wgrad with the bias gradient (partials, bias partials and the finish launch)
    t_fwd       F.conv2d                                  (PyTorch-ROCm fp32; whatever its backend picks after warm-up)
    t_dgrad     torch.nn.grad.conv2d_input
    t_wgrad     torch.nn.grad.conv2d_weight + the bias sum
The table goes to `--out` (default profiles/conv_grad_bench.txt).

    python tools/bench_conv_grad.py [--iters 10] [--repeats 5] [--batch 16] [--no-torch]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv_grad_bench.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_conv_grad needs the GPU"
    import conv_grad_ref as R
    from diffcodec_amd import lib, ops, train
    dev = torch.device("cuda")
    L = lib.load()
    st = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(0)
    n = a.batch
    legs = ["fwd", "silu_grad", "dgrad", "wgrad"] + ([] if a.no_torch else ["t_fwd", "t_dgrad", "t_wgrad"])
    lines = [f"# tools/bench_conv_grad.py --batch {n} --iters {a.iters} --repeats {a.repeats}: ms per call, median [min, max] of the windows; "
             "TFLOP/s of the median (silu_grad: TB/s)",
             f"# device: {torch.cuda.get_device_name(0)}, torch {torch.__version__}",
             "layer".ljust(28) + "".join(l.rjust(34) for l in legs)]
    print("\n".join(lines), flush=True)
    for cin, h, w, cout, s in R.PRODUCTION_LAYERS:
        ho, wo = R.out_size(h, w, s)
        x = torch.randn(n, cin, h, w, device=dev, generator=gen)
        wt = torch.randn(cout, cin, 3, 3, device=dev, generator=gen) * (1.5 / (9 * cin) ** 0.5)
        b = torch.randn(cout, device=dev, generator=gen)
        gy = torch.randn(n, cout, ho, wo, device=dev, generator=gen)
        z, gz, dx, dw, db = torch.empty_like(gy), torch.empty_like(gy), torch.empty_like(x), torch.empty_like(wt), torch.empty_like(b)
        ws = torch.empty(L.dc_conv3x3_f32_wgrad_ws_bytes(n, cin, h, w, cout, s) // 4, dtype=torch.float32, device=dev)
        flops = 2.0 * n * ho * wo * cout * cin * 9
        forms = (ops.conv3x3_f32_route(cin, h, w, cout, s).form, train.conv3x3_f32_grad_route("dgrad", n, cin, h, w, cout, s).form,
                 train.conv3x3_f32_grad_route("wgrad", n, cin, h, w, cout, s).form)
        fns = {
            "fwd": lambda: lib.call("dc_conv3x3_nchw_f32", x.data_ptr(), x.stride(0), wt.data_ptr(), b.data_ptr(), z.data_ptr(), n, cin, h,
                                    w, cout, s, 0, st),
            "silu_grad": lambda: lib.call("dc_silu_grad_f32", z.data_ptr(), gy.data_ptr(), gz.data_ptr(), gy.numel(), st),
            "dgrad": lambda: lib.call("dc_conv3x3_f32_dgrad", gz.data_ptr(), wt.data_ptr(), dx.data_ptr(), n, cin, h, w, cout, s, st),
            "wgrad": lambda: lib.call("dc_conv3x3_f32_wgrad", x.data_ptr(), x.stride(0), gz.data_ptr(), dw.data_ptr(), db.data_ptr(),
                                      ws.data_ptr(), n, cin, h, w, cout, s, st),
            "t_fwd": lambda: F.conv2d(x, wt, b, stride=s, padding=1),
            "t_dgrad": lambda: torch.nn.grad.conv2d_input(x.shape, wt, gz, stride=s, padding=1),
            "t_wgrad": lambda: (torch.nn.grad.conv2d_weight(x, wt.shape, gz, stride=s, padding=1), gz.sum((0, 2, 3))),
        }
        cells = []
        for leg in legs:
            ms, lo, hi = device_ms(fns[leg], a.iters, a.repeats)
            rate = 3 * 4.0 * gy.numel() / (ms * 1e-3) / 1e12 if leg == "silu_grad" else flops / (ms * 1e-3) / 1e12
            cells.append(f"{ms:8.4f} [{lo:.4f}, {hi:.4f}] {rate:6.2f}".rjust(34))
        line = f"{cin}->{cout} {h}x{w} s{s} {'/'.join(forms)}".ljust(28) + "".join(cells)
        lines.append(line)
        print(line, flush=True)
        del x, wt, gy, z, gz, dx, dw, ws
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
