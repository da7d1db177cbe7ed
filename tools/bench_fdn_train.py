"""Time forward plus backward of the trainable FDN injection (diffcodec_amd.fdn_train, csrc/fdn_grad.hip) at the four production
shapes ([N,320,64,64], [N,320,32,32], [N,640,16,16], [N,1280,8,8]) at batch 16, next to the same expression in PyTorch-ROCm fp32
autograd on the same device:

    fdn          fdn_train.fdn alone: gradients to x, gamma and beta            | torch: F.group_norm(x, 32) * (1 + gamma) + beta
    FDN          fdn_train.FDN with its two train.Conv3x3: gradients to x, the  | torch: the same with two F.conv2d
                 local features and the four parameters

Event-timed on preallocated operands: median (and range) of `--repeats` windows of `--iters` forward + backward calls; nothing is
synchronised inside a window (the `FDN` rows, which the convolution gradients dominate, use windows of iters / 5).  The `fdn` rows
also state the rate of the derived HBM traffic (9 C-planes per forward + backward: the forward reads x, gamma, beta and writes y, the
backward reads g, x, gamma and writes g_x, g_gamma) at the measured time.  The table goes to `--out` (default
profiles/fdn_train_bench.txt).

    python tools/bench_fdn_train.py [--iters 50] [--repeats 7] [--batch 16] [--no-module]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

SHAPES = [(320, 64, 64), (320, 32, 32), (640, 16, 16), (1280, 8, 8)]          # (C, H, W) of fdn64, fdn32, fdn16, fdn08
PLANES = 9                                                                    # derived, not measured: see the module docstring


def device_ms(fn, iters, repeats):
    iters = max(1, iters)
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


def fdn_torch(x, gamma, beta):
    return F.group_norm(x, 32, None, None, 1e-5) * (1 + gamma) + beta


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--no-module", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fdn_train_bench.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_fdn_train needs the GPU"
    from diffcodec_amd import fdn_train as T
    dev = torch.device("cuda")
    gen = torch.Generator(device="cuda").manual_seed(0)
    n = a.batch
    legs = ["hip", "torch"]
    lines = [f"# tools/bench_fdn_train.py --batch {n} --iters {a.iters} --repeats {a.repeats}: ms per forward + backward, median [min, max] "
             f"of the windows (FDN rows: windows of {max(1, a.iters // 5)}); x = time over the HIP form's",
             f"# GB/s: {PLANES} C-planes of fp32 per forward + backward of fdn (derived traffic) over the HIP form's median time",
             f"# device: {torch.cuda.get_device_name(0)}, torch {torch.__version__}",
             "workload".ljust(30) + "".join(l.rjust(40) for l in legs) + "GB/s".rjust(10)]
    print("\n".join(lines), flush=True)

    def row(name, fns, iters, nbytes=None):
        cells, base = [], None
        for leg in legs:
            ms, lo, hi = device_ms(fns[leg], iters, a.repeats)
            base = ms if base is None else base
            cells.append(f"{ms:9.3f} [{lo:.3f}, {hi:.3f}] {ms / base:6.2f}x".rjust(40))
        rate = "" if nbytes is None else f"{nbytes / (base * 1e-3) / 1e9:10.0f}"
        lines.append(name.ljust(30) + "".join(cells) + rate)
        print(lines[-1], flush=True)

    for c, h, w in SHAPES:
        x, gamma, beta = (torch.randn(n, c, h, w, device=dev, generator=gen).requires_grad_(True) for _ in range(3))
        G = torch.randn(n, c, h, w, device=dev, generator=gen)
        leaves = [x, gamma, beta]
        row(f"fdn [{n},{c},{h},{w}]", {"hip": lambda: torch.autograd.grad(T.fdn(x, gamma, beta), leaves, G),
                                       "torch": lambda: torch.autograd.grad(fdn_torch(x, gamma, beta), leaves, G)},
            a.iters, nbytes=PLANES * x.numel() * 4)
        del x, gamma, beta, G, leaves

    if not a.no_module:
        for c, h, w in SHAPES:
            m = T.FDN(c, c).to(dev)
            x, local = (torch.randn(n, c, h, w, device=dev, generator=gen).requires_grad_(True) for _ in range(2))
            G = torch.randn(n, c, h, w, device=dev, generator=gen)
            params = list(m.parameters())
            wg, bg, wb, bb = m.conv_gamma.weight, m.conv_gamma.bias, m.conv_beta.weight, m.conv_beta.bias

            def module_torch():
                y = fdn_torch(x, F.conv2d(local, wg, bg, padding=1), F.conv2d(local, wb, bb, padding=1))
                return torch.autograd.grad(y, [x, local] + params, G)

            row(f"FDN [{n},{c},{h},{w}]", {"hip": lambda: torch.autograd.grad(m(x, local), [x, local] + params, G), "torch": module_torch},
                a.iters // 5)
            del m, x, local, G, params
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
