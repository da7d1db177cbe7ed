"""Time PSNR + MS-SSIM (csrc/metrics.hip) per frame pair: uint8 NHWC frames (what the clip driver scores), a batch of 16 pairs at
512x512 and at 1080p.  Prints one JSON line per shape: event-timed milliseconds per call and per pair (host launch overhead
included).  Kernel times: run under `rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_metrics.py`.

    python tools/bench_metrics.py [--batch 16] [--iters 20]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_metrics needs the GPU"
    from diffcodec_amd import metrics as M
    g = torch.Generator(device="cuda").manual_seed(0)
    for h, w in ((512, 512), (1080, 1920)):
        x = torch.randint(0, 256, (a.batch, h, w, 3), dtype=torch.uint8, device="cuda", generator=g)
        noise = torch.randint(-8, 9, (a.batch, h, w, 3), device="cuda", generator=g)
        y = (x.int() + noise).clamp(0, 255).to(torch.uint8)
        for _ in range(3):
            M.ms_ssim(x, y, data_range=255, size_average=False)
            M.psnr(x, y)
        torch.cuda.synchronize()
        res = {}
        for name, fn in (("ms_ssim", lambda: M.ms_ssim(x, y, data_range=255, size_average=False)), ("psnr", lambda: M.psnr(x, y))):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / a.iters
            res[name] = dict(ms_per_call=round(ms, 4), ms_per_pair=round(ms / a.batch, 5))
        print(json.dumps(dict(shape=f"{h}x{w}", batch=a.batch, **res)), flush=True)


if __name__ == "__main__":
    main()
