"""Time the softsplat entry points (csrc/splat.hip, csrc/splat_grad.hip) at the two shapes that matter for training through the
warp: [32, 161, 64, 64] and [32, 641, 8, 8] (fp32 NCHW, smooth flow of sigma 1.5 px).

Per shape: forward 'soft' (dc_splat_norm_f32(soft, addeps): memset + four bin kernels + the gather), ingrad and flowgrad (one
kernel each), called back to back on preallocated operands and event-timed (median of `--repeats` windows of `--iters` calls: the
device time of one call including its launch gaps; no allocation, no synchronisation inside the window).  The algorithmic bytes
are counted from the shapes — every operand read once, every result written once, the corner reads of neighbouring sources
counted once because they share cache lines:
    forward   in + out (C planes each), flow, metric, and the bins (cell, sorted twice, two count tables) written and read once
    ingrad    outgrad + ingrad (C planes each), flow
    flowgrad  in + outgrad (C planes each), flow + flowgrad
and `share_of_hbm` is bytes / time over `--hbm-tbs` (6.3 TB/s, the achievable streaming rate of the MI355X).  The 8x8 shape moves
5 MB per call: it measures launch latency and occupancy, not bandwidth.

    python tools/bench_splat.py [--iters 50] [--repeats 7]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

SHAPES = [(32, 161, 64, 64), (32, 641, 8, 8)]


def device_ms(fn, iters, repeats):
    for _ in range(5):
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
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--hbm-tbs", type=float, default=6.3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_splat needs the GPU"
    from diffcodec_amd import lib, ops
    L = lib.load()
    st = torch.cuda.current_stream().cuda_stream
    for (n, c, h, w) in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(0)
        x = torch.randn(n, c, h, w, device="cuda", generator=g)
        og = torch.randn(n, c, h, w, device="cuda", generator=g)
        flow = 1.5 * torch.randn(n, 2, h, w, device="cuda", generator=g)
        metric = torch.randn(n, 1, h, w, device="cuda", generator=g)
        out, ingrad, flowgrad = torch.empty_like(x), torch.empty_like(x), torch.empty_like(flow)
        ws = torch.empty(int(L.dc_splat_ws_bytes(n, h, w)), dtype=torch.uint8, device="cuda")
        px = n * h * w
        legs = {
            "forward_soft": (lambda: lib.call("dc_splat_norm_f32", x.data_ptr(), flow.data_ptr(), metric.data_ptr(), 0, out.data_ptr(),
                                              ws.data_ptr(), n, c, h, w, ops.SPLAT_MODES["soft"], ops.SPLAT_EPS["addeps"], st),
                             4 * px * (2 * c + 3) + 2 * ws.numel()),
            "ingrad": (lambda: lib.call("dc_splat_ingrad_f32", flow.data_ptr(), og.data_ptr(), ingrad.data_ptr(), n, c, h, w, st),
                       4 * px * (2 * c + 2)),
            "flowgrad": (lambda: lib.call("dc_splat_flowgrad_f32", x.data_ptr(), flow.data_ptr(), og.data_ptr(), flowgrad.data_ptr(),
                                          n, c, h, w, st),
                         4 * px * (2 * c + 4)),
        }
        for name, (fn, nbytes) in legs.items():
            ms, lo, hi = device_ms(fn, a.iters, a.repeats)
            tbs = nbytes / (ms * 1e-3) / 1e12
            print(json.dumps(dict(kernel=name, shape=[n, c, h, w], ms_per_call=round(ms, 4), ms_min=round(lo, 4), ms_max=round(hi, 4),
                                  bytes_moved=nbytes, tb_per_s=round(tbs, 3), share_of_hbm=round(tbs / a.hbm_tbs, 3))), flush=True)


if __name__ == "__main__":
    main()
