"""Time forward plus backward of the trainable control pyramid (diffcodec_amd.pyramid_train, csrc/pyramid_grad.hip): one level
(`warp_fuse`) at the four level shapes of a 512 x 512 frame at batch 16, and the whole `BiDirFeatureExtractor` at 16 x 512 x 512,
next to two other ways to get the same gradients on the same device:

    fused      pyramid_train.warp_fuse / pyramid_train.BiDirFeatureExtractor
    composed   what the package offered before the fused operator: train.Conv3x3, softsplat.softsplat(..., 'soft') under autograd
               (cat[in * exp(m), exp(m)], the 'sum' splat and its HIP backward, the divide) and the fusion in torch ops
    torch      PyTorch-ROCm fp32 autograd alone: F.conv2d and the scatter_add restatement of tests/splat_grad_ref.py; for the
               whole module it is handed each level's resized flows and masks, which are not timed

Gradients go to both feature maps and both metrics (level) or to every parameter (module).  Event-timed on preallocated operands:
median (and range) of `--repeats` windows of `--iters` forward + backward calls; nothing is synchronised inside a window.  The
table goes to `--out` (default profiles/pyramid_train_bench.txt).

    python tools/bench_pyramid_train.py [--iters 5] [--repeats 5] [--batch 16] [--no-torch] [--no-module]"""
import argparse
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

LEVELS = [(160, 64, 64), (160, 32, 32), (320, 16, 16), (640, 8, 8)]          # (C, H, W) of inject_channels (320, 320, 640, 1280) / 2


def device_ms(fn, iters, repeats):
    for _ in range(2):
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


def fuse_torch(wf, wl, cf, cb, of, ob):
    conf = torch.clamp(torch.cat([cf, cb], 1), min=0)
    w = conf / (conf.sum(1, keepdim=True) + 1e-6)
    fused = w[:, :1] * wf + w[:, 1:] * wl
    return torch.where(((of + ob) > 1.5).expand_as(fused), 0.5 * (wf + wl), fused)


def level_composed(first, last, mf, mb, ff, fb, of, ob):
    from diffcodec_amd.softsplat import softsplat
    return fuse_torch(softsplat(first, ff, mf, "soft") * (1 - of), softsplat(last, fb, mb, "soft") * (1 - ob), mf, mb, of, ob)


def module_composed(m, cond, flow):
    """pyramid_train.BiDirFeatureExtractor.forward with `level_composed` in the place of `warp_fuse`"""
    from diffcodec_amd import ops
    h = cond.shape[-2]
    f, l = m.first_pre_extractor(cond[:, 3:]), m.last_pre_extractor(cond[:, :3])
    outs = []
    for idx, r in enumerate((h // 8, h // 16, h // 32, h // 64)):
        f, l = m.extractors_first[idx](f), m.extractors_last[idx](l)
        with torch.no_grad():
            flow_f, flow_b = ops.flow_resize_normalize(flow[:, :2], r, r), ops.flow_resize_normalize(flow[:, 2:], r, r)
            occ_f, occ_b = ops.occlusion_mask(flow_f, flow_b), ops.occlusion_mask(flow_b, flow_f)
        outs.append(m.zero_convs[idx](level_composed(f, l, m.wrapper[idx](f), m.wrapper[idx](l), flow_f, flow_b, occ_f, occ_b)))
    return outs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-module", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pyramid_train_bench.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_pyramid_train needs the GPU"
    import pyramid_grad_ref as R
    from diffcodec_amd import pyramid_train as PT
    dev = torch.device("cuda")
    gen = torch.Generator(device="cuda").manual_seed(0)
    n = a.batch
    legs = ["fused", "composed"] + ([] if a.no_torch else ["torch"])
    lines = [f"# tools/bench_pyramid_train.py --batch {n} --size {a.size} --iters {a.iters} --repeats {a.repeats}: ms per forward + backward, "
             "median [min, max] of the windows; x = time over the fused form's",
             "# the torch leg of the module is handed each level's resized flows and occlusion masks, computed once outside the timed "
             "windows; the other two legs compute them inside",
             f"# device: {torch.cuda.get_device_name(0)}, torch {torch.__version__}",
             "workload".ljust(30) + "".join(l.rjust(40) for l in legs)]
    print("\n".join(lines), flush=True)

    def row(name, fns):
        cells, base = [], None
        for leg in legs:
            ms, lo, hi = device_ms(fns[leg], a.iters, a.repeats)
            base = ms if base is None else base
            cells.append(f"{ms:9.3f} [{lo:.3f}, {hi:.3f}] {ms / base:6.2f}x".rjust(40))
        lines.append(name.ljust(30) + "".join(cells))
        print(lines[-1], flush=True)

    for c, h, w in LEVELS:
        first, last = (torch.randn(n, c, h, w, device=dev, generator=gen).requires_grad_(True) for _ in range(2))
        mf, mb = (torch.randn(n, 1, h, w, device=dev, generator=gen).requires_grad_(True) for _ in range(2))
        ff, fb = (1.5 * torch.randn(n, 2, h, w, device=dev, generator=gen) for _ in range(2))
        of, ob = ((torch.rand(n, 1, h, w, device=dev, generator=gen) < 0.5).float() for _ in range(2))
        G = torch.randn(n, c, h, w, device=dev, generator=gen)
        leaves = [first, last, mf, mb]

        def go(fn):
            return lambda: torch.autograd.grad(fn(first, last, mf, mb, ff, fb, of, ob), leaves, G)

        row(f"level [{n},{c},{h},{w}]", {"fused": go(PT.warp_fuse), "composed": go(level_composed),
                                         "torch": go(lambda *t: R.level(*t, dtype=torch.float32))})
        del first, last, G

    if not a.no_module:
        s = a.size
        m = PT.BiDirFeatureExtractor().to(dev)
        with torch.no_grad():
            for z in m.zero_convs:                                         # fresh zero convs would leave every upstream gradient zero
                z.weight.normal_(0, 0.02, generator=gen)
        cond = torch.rand(n, 6, s, s, device=dev, generator=gen) * 2 - 1
        # a smooth forward flow and fb = -ff + a residual of 0.02 - 4 px (tests/pyramid_grad_ref.module_inputs): independent random
        # flows would occlude the coarse levels almost completely
        ff = torch.nn.functional.interpolate(0.15 * torch.randn(n, 2, s // 16, s // 16, device=dev, generator=gen), size=(s, s),
                                             mode="bicubic", align_corners=False)
        mag = torch.exp(torch.rand(n, 1, s, s, device=dev, generator=gen) * (math.log(4.0) - math.log(0.02)) + math.log(0.02))
        ang = torch.rand(n, 1, s, s, device=dev, generator=gen) * (2 * math.pi)
        flow = torch.cat([ff, -ff + torch.cat([mag * ang.cos(), mag * ang.sin()], 1)], 1).contiguous()
        params = list(m.parameters())
        sd = {k: v for k, v in m.named_parameters()}

        def loss_of(outs):
            return sum(o.sum() for o in outs)

        with torch.no_grad():
            aux = m(cond, flow, return_aux=True)[1]                        # the torch leg is handed the flows and masks: not timed

        def torch_module():
            return torch.autograd.grad(loss_of(R.extractor(sd, cond, aux, torch.float32)), params)

        row(f"module {n} x {s}x{s}", {"fused": lambda: torch.autograd.grad(loss_of(m(cond, flow)), params),
                                      "composed": lambda: torch.autograd.grad(loss_of(module_composed(m, cond, flow)), params),
                                      "torch": torch_module})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
