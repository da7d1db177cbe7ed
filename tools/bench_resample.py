"""Time `resample.resize_u8` (csrc/resample.hip) at the scoring workload and the host path it replaces.

Device leg: 16 uint8 frames 1024x1920 -> 512x512 "bilinear" resident in HBM, event-timed over back-to-back calls (median of
`--repeats` windows of `--iters` calls; the two launches and the host launch overhead of one call are inside).  The bytes the
two-pass form must move are counted from the shapes: one read of the input, one write and one read of the uint8 intermediate
[N, H_in, W_out, 3], one write of the output; `share_of_hbm` is those bytes over the time against `--hbm-tbs` (6.3 TB/s, the
achievable streaming rate of the MI355X).  Kernel times alone: run under `rocprofv3 --kernel-trace --stats -d <dir> -- python
tools/bench_resample.py --no-host`.

Host leg, same box and frames: device -> host copy, Pillow's `Image.resize((512, 512), BILINEAR)` per frame, host -> device copy
(median of `--host-repeats` runs, host clock around work that ends in a device synchronise).  The device result is compared with
Pillow's bytes before anything is timed.  One more line gives the other two uses: 1 frame 270x480 -> 1080x1920 "lanczos" and 1
frame 1080x1920 -> 512x512 "bicubic".

    python tools/bench_resample.py [--frames 16] [--iters 50] [--repeats 7] [--no-host]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


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
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-repeats", type=int, default=5)
    ap.add_argument("--hbm-tbs", type=float, default=6.3)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_resample needs the GPU"
    from diffcodec_amd.resample import resize_u8
    g = torch.Generator(device="cuda").manual_seed(0)
    n, h, w, oh, ow = a.frames, 1024, 1920, 512, 512
    x = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device="cuda", generator=g)
    out = resize_u8(x, (oh, ow), "bilinear")

    def pillow_round_trip():
        from PIL import Image
        import numpy as np
        host = x.cpu().numpy()
        res = np.stack([np.asarray(Image.fromarray(f).resize((ow, oh), Image.BILINEAR)) for f in host])
        return torch.from_numpy(res).to("cuda")

    if not a.no_host:
        assert torch.equal(out, pillow_round_trip()), "device bytes differ from Pillow's"
    ms, lo, hi = device_ms(lambda: resize_u8(x, (oh, ow), "bilinear"), a.iters, a.repeats)
    moved = n * 3 * (h * w + 2 * h * ow + oh * ow)
    line = dict(resample=f"{h}x{w}->{oh}x{ow} bilinear", frames=n, ms_per_call=round(ms, 4), ms_min=round(lo, 4), ms_max=round(hi, 4),
                us_per_frame=round(ms * 1e3 / n, 2), bytes_moved=moved, tb_per_s=round(moved / (ms * 1e-3) / 1e12, 3),
                share_of_hbm=round(moved / (ms * 1e-3) / 1e12 / a.hbm_tbs, 3))
    if not a.no_host:
        runs = []
        for _ in range(a.host_repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pillow_round_trip()
            torch.cuda.synchronize()
            runs.append((time.perf_counter() - t0) * 1e3)
        line.update(host_round_trip_ms=round(statistics.median(runs), 2), host_min_ms=round(min(runs), 2), host_max_ms=round(max(runs), 2),
                    host_over_device=round(statistics.median(runs) / ms, 1))
    print(json.dumps(line), flush=True)
    small = torch.randint(0, 256, (1, 270, 480, 3), dtype=torch.uint8, device="cuda", generator=g)
    hd = torch.randint(0, 256, (1, 1080, 1920, 3), dtype=torch.uint8, device="cuda", generator=g)
    up, _, _ = device_ms(lambda: resize_u8(small, (1080, 1920), "lanczos"), a.iters, a.repeats)
    down, _, _ = device_ms(lambda: resize_u8(hd, (512, 512), "bicubic"), a.iters, a.repeats)
    print(json.dumps(dict(lanczos_270x480_to_1080x1920_ms=round(up, 4), bicubic_1080x1920_to_512x512_ms=round(down, 4))), flush=True)


if __name__ == "__main__":
    main()
