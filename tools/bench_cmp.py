"""Time HipCMP.flow (SkipLayer decoder, the semiauto_annot/resnet50_vip+mpii_liteflow architecture, seeded weights) at 512 x 512 for
N = 2 (the two directions of one frame) and N = 16, and report each convolution family's share and TFLOP/s against the
157.3 TFLOP/s fp32 matrix peak of the MI355X.

    python tools/bench_cmp.py [--out profiles/cmp_bench.txt] [--lib PATH]      (--lib: another build of the same ABI)

Whole-call times are the median of `--iters` eager calls and of as many replays of a captured graph, after warm-up; family times
come from a separate pass over HipCMP.staged_endpoints (the same launches, driven one by one) with lib.LaunchTimer (two events
round every launch), never from the timed calls."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cmp_ref as R  # noqa: E402
from diffcodec_amd import lib  # noqa: E402
from diffcodec_amd.flow_propagation import HipCMP  # noqa: E402

PEAK = 157.3


def timed(fn, iters):
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--lib", default=None, help="another build of libdiffcodec_hip.so (same ABI)")
    args = ap.parse_args()
    if args.lib:
        lib.LIB_PATH = os.path.abspath(args.lib)
    model = HipCMP.from_state_dict(R.synth_weights("skip"), R.CONFIGS["skip"], "cuda")
    lines = [f"HipCMP.flow, MotionDecoderSkipLayer, {args.size} x {args.size}, fp32 on v_mfma_f32_32x32x2_f32 "
             f"({torch.cuda.get_device_name(0)}); peak {PEAK} TFLOP/s"]
    for n in (2, 16):
        u8, sparse = R.inputs(n, args.size, args.size, 77)
        x, sp = u8.cuda(), sparse.cuda()
        for _ in range(3):
            model.flow(x, sp)
        torch.cuda.synchronize()
        med, best = timed(lambda: model.flow(x, sp), args.iters)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            model.flow(x, sp)
        g.replay()
        torch.cuda.synchronize()
        gmed, gbest = timed(g.replay, args.iters)
        model.staged_endpoints(x, sp)
        torch.cuda.synchronize()
        lib.TIMER = t = lib.LaunchTimer()
        model.staged_endpoints(x, sp)                                    # the same launches, one lib.call each
        torch.cuda.synchronize()
        lib.TIMER = None
        fam = t.summary()
        flops = sum(f["flops"] for f in fam.values())
        lines.append(f"N = {n:2d}: eager median {med:8.2f} ms (best {best:.2f}), graph replay median {gmed:8.2f} ms (best {gbest:.2f}) "
                     f"= {gmed / n:.2f} ms per image; {flops / 1e12:.3f} TFLOP in convolutions -> {flops / gmed / 1e9:.1f} TFLOP/s over the whole call")
        lines.append(f"  {'family':14s} {'launches':>8s} {'ms':>9s} {'TFLOP':>8s} {'TFLOP/s':>8s} {'of peak':>8s}")
        for name in ("stem", "sparse", "1x1", "3x3", "dilated 3x3", "decoder"):
            f = fam.get(name)
            if f:
                tf = f["flops"] / f["ms"] / 1e9
                lines.append(f"  {name:14s} {f['calls']:8d} {f['ms']:9.3f} {f['flops'] / 1e12:8.4f} {tf:8.1f} {100 * tf / PEAK:7.1f}%")
        other = {k: v for k, v in fam.items() if k.startswith("dc_cmp_")}
        lines.append(f"  {'pools, upsample, convert':24s} {sum(v['calls'] for v in other.values()):4d} launches {sum(v['ms'] for v in other.values()):9.3f} ms")
    lines.append("for comparison (README.md): decode 50.9 ms per frame; lpips.hip conv2-5 at 16 pairs 119-126 TFLOP/s, at one pair 27-77")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
