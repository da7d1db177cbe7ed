"""Time the guide-point sampler (csrc/guide_points.hip) on 16 synthetic flows at 512 x 512 and at 1080 x 1920 (working size
270 x 480): every stage entry on the device's own previous output, the fused dc_guide_watershed eager and as a captured graph's
replay, and next to them the host path the reference runs for one flow, timed on the same machine (scipy's convolve2d,
distance_transform_edt and maximum_filter where scipy imports, otherwise the numpy restatement of tests/guide_ref.py; the
elimination is the restatement's either way).

    python tools/bench_guides.py [--out profiles/guide_bench.txt] [--iters 20] [--lib PATH]

Times are medians of `--iters` runs between two events after warm-up; the host path is the median of 3."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import guide_ref as G  # noqa: E402
from diffcodec_amd import guide_points as GP  # noqa: E402
from diffcodec_amd import lib  # noqa: E402


def timed(fn, iters):
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def host_path(flow, ks):
    """one flow [2,H,W] on the host -> (ms, number of points, which arithmetic)"""
    try:
        from scipy import ndimage, signal
    except ImportError:
        ndimage = None
    hw2 = np.ascontiguousarray(flow.numpy().transpose(1, 2, 0))
    ds = G.working_ds(*hw2.shape[:2])

    def run():
        if ndimage is None:
            return len(G.watershed(flow, ks, big=True)[1])
        sobel = np.array([[1, 0, -1], [2, 0, -2], [1, 0, -1]], dtype=np.float32)
        sub = hw2[::ds, ::ds]
        edge = sum(np.sqrt(signal.convolve2d(sub[:, :, k], sobel, boundary="symm", mode="same") ** 2 +
                           signal.convolve2d(sub[:, :, k], sobel.T, boundary="symm", mode="same") ** 2) for k in range(2))
        edge = edge / max(edge.max(), 0.01) > 0.1
        dist = ndimage.distance_transform_edt(1 - edge.astype(np.float32))
        dist[dist < ndimage.maximum_filter(dist, footprint=np.ones((ks, ks)))] = 0.0
        dist[0, :] = dist[-1, :] = 0.0
        dist[:, 0] = dist[:, -1] = 0.0
        return len(G.greedy(*np.nonzero(dist > 0), (ks - 1) / 2)[0])

    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        n = run()
        ts.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ts), n, "scipy" if ndimage is not None else "numpy restatement"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--ks", type=int, default=15)
    ap.add_argument("--lib", default=None, help="another build of libdiffcodec_hip.so (same ABI)")
    args = ap.parse_args()
    if args.lib:
        lib.LIB_PATH = os.path.abspath(args.lib)
    N, ks = args.batch, args.ks
    stream = lambda: torch.cuda.current_stream().cuda_stream
    lines = [f"guide points ('grid' + 'watershed', nms_ks {ks}, stride 80) of {N} flows ({torch.cuda.get_device_name(0)}); ms, median of {args.iters}"]
    for H, W in ((512, 512), (1080, 1920)):
        flows = torch.stack([G.to_nchw(G.synth_flow(G.synth_params(100 + i, H, W, 8), H, W))[0] for i in range(N)])
        x = flows.cuda()
        ds, h, w = GP.working_size(H, W)
        cap = GP.max_points(h, w, ks)
        ws = GP.workspace(x)
        dev = lambda *shape, dtype: torch.empty(*shape, dtype=dtype, device="cuda")
        edge, d2, cand = dev(N, h, w, dtype=torch.uint8), dev(N, h, w, dtype=torch.int32), dev(N, h, w, dtype=torch.uint8)
        counts, points, sparse = dev(N, dtype=torch.int32), dev(N, cap, 2, dtype=torch.int32), dev(N, 4, H, W, dtype=torch.float32)
        stages = [
            ("edge", lambda: lib.call("dc_guide_edge", x.data_ptr(), N, H, W, ws.data_ptr(), None, edge.data_ptr(), stream())),
            ("edt", lambda: lib.call("dc_guide_edt", edge.data_ptr(), N, h, w, ws.data_ptr(), d2.data_ptr(), stream())),
            ("nms", lambda: lib.call("dc_guide_nms", d2.data_ptr(), N, h, w, ks, ws.data_ptr(), cand.data_ptr(), stream())),
            ("select", lambda: lib.call("dc_guide_select", cand.data_ptr(), N, h, w, ks, ds, ws.data_ptr(), counts.data_ptr(),
                                        points.data_ptr(), cap, stream())),
            ("scatter", lambda: lib.call("dc_guide_scatter", x.data_ptr(), N, H, W, 80, counts.data_ptr(), points.data_ptr(), cap,
                                         sparse.data_ptr(), stream())),
        ]
        fused = lambda: lib.call("dc_guide_watershed", x.data_ptr(), N, H, W, ks, 80, ws.data_ptr(), counts.data_ptr(), points.data_ptr(),
                                 cap, sparse.data_ptr(), stream())
        for _ in range(3):
            for _, fn in stages:
                fn()
            fused()
        torch.cuda.synchronize()
        per = [(name, timed(fn, args.iters)) for name, fn in stages]
        ncand = int(cand.sum())
        eager = timed(fused, args.iters)
        wrapped = timed(lambda: GP.sample_watershed(x, ks, stride=80), args.iters)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fused()
        g.replay()
        torch.cuda.synchronize()
        replay = timed(g.replay, args.iters)
        host_ms, host_n, how = host_path(flows[0], ks)
        lines.append(f"{H} x {W} (working size {h} x {w}, ds {ds}): {ncand} candidates, {int(counts.sum())} watershed points in {N} flows")
        lines.append("  " + "  ".join(f"{name} {ms:.3f}" for name, ms in per) + f"  (sum {sum(ms for _, ms in per):.3f})")
        lines.append(f"  fused dc_guide_watershed: eager {eager:.3f}, graph replay {replay:.3f} = {replay / N:.4f} per flow; "
                     f"sample_watershed (with its allocations) {wrapped:.3f}")
        lines.append(f"  host path ({how}), one flow ({host_n} points; the device {int(counts[0])}): {host_ms:.1f} -> {host_ms * N:.0f} for {N}; the device is {host_ms * N / replay:.0f}x faster")
    lines.append("for comparison (README.md): HipCMP.flow, which consumes these points, 27.8 ms for the two directions of a 512 x 512 frame")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
