"""Time PSNR + MS-SSIM (csrc/metrics.hip) per frame pair: uint8 NHWC frames (what the clip driver scores), a batch of 16 pairs at
512x512 and at 1080p.  Prints one JSON line per shape: event-timed milliseconds per call and per pair (host launch overhead
included).  Kernel times: run under `rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_metrics.py`.

LPIPS leg (csrc/lpips.hip, seeded random weights): at 512x512 for 1 and 16 pairs and at 1080p for 1 pair, one JSON line with the
whole call (ms per call and per pair) and, per conv layer, the time of the layer's kernel alone on the call's 2N images
(dc_lpips_conv, back-to-back launches between two events) with its TFLOP/s.

FID leg (csrc/fid.hip, seeded random weights): 16 images and 1 image of 512x512, one JSON line with the whole `update` call (ms per
call and per image), `features` alone, the accumulate launch alone and, per conv block, the time of the block's kernel alone
(dc_fid_conv, back-to-back launches between two events) with its TFLOP/s; resize + pool + host is the remainder of `features`.

FVD leg (csrc/fvd.hip, seeded random weights): `features` of one 16 x 512 x 512 uint8 video and of a batch of 8, one JSON line each
with the milliseconds per call and per video and the TFLOP/s over the convolutions' 27.8 G multiply-adds per 16-frame video.

    python tools/bench_metrics.py [--batch 16] [--iters 20] [--no-lpips] [--no-fid] [--no-fvd] [--only-fvd] [--no-ssim] [--lib PATH]

`--lib` times another build of the same ABI (one process per library); `--no-ssim` skips the PSNR / MS-SSIM leg."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def lpips_leg(iters):
    import ctypes
    from diffcodec_amd import lib, metrics as M
    g = torch.Generator().manual_seed(0)
    sd = {}
    for l, (co, ci, k, pos) in enumerate(zip(M.LPIPS_CHANNELS, M.LPIPS_CIN, M.LPIPS_KERNEL, M.LPIPS_FEATURE_INDEX)):
        a = (ci * k * k) ** -0.5
        sd[f"features.{pos}.weight"] = (torch.rand(co, ci, k, k, generator=g) * 2 - 1) * 1.7 * a
        sd[f"features.{pos}.bias"] = (torch.rand(co, generator=g) * 2 - 1) * a
        sd[f"lin{l}.model.1.weight"] = torch.rand(1, co, 1, 1, generator=g)
    model = M.LPIPS.from_state_dict(sd).to("cuda")
    wts = model._weights(torch.device("cuda"))
    stream = torch.cuda.current_stream().cuda_stream

    def timed(fn):
        for _ in range(3):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters

    gd = torch.Generator(device="cuda").manual_seed(0)
    for h, w, n in ((512, 512, 1), (512, 512, 16), (1080, 1920, 1)):
        x = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device="cuda", generator=gd)
        y = (x.int() + torch.randint(-8, 9, (n, h, w, 3), device="cuda", generator=gd)).clamp(0, 255).to(torch.uint8)
        ms = timed(lambda: model(x, y))
        both = torch.cat([x, y])
        feats = model.features(both)
        sizes = M.lpips_map_sizes(h, w)
        strides = (ctypes.c_longlong * 4)(*M._nchw(both)[1])
        layers = {}
        for l, (co, ci, k) in enumerate(zip(M.LPIPS_CHANNELS, M.LPIPS_CIN, M.LPIPS_KERNEL)):
            hh, ww = sizes[l]
            if l == 0:
                src, a_h, a_w = both, h, w
            else:
                src = torch.nn.functional.max_pool2d(feats[l - 1], 3, 2) if l in (1, 2) else feats[l - 1]
                src, a_h, a_w = src.contiguous(), hh, ww
            out = torch.empty_like(feats[l])
            t = timed(lambda: lib.call("dc_lpips_conv", l, src.data_ptr(), int(l == 0), strides, 2 * n, a_h, a_w, 0, wts.data_ptr(),
                                       out.data_ptr(), stream))
            assert torch.equal(out, feats[l]), f"conv{l + 1} alone differs from the fused sequence"
            flop = 2.0 * (2 * n) * co * hh * ww * ci * k * k
            layers[f"conv{l + 1}"] = dict(us=round(t * 1e3, 1), tflops=round(flop / (t * 1e-3) / 1e12, 1))
        conv_ms = sum(v["us"] for v in layers.values()) / 1e3
        print(json.dumps(dict(lpips=f"{h}x{w}", pairs=n, ms_per_call=round(ms, 4), ms_per_pair=round(ms / n, 4),
                              conv_ms=round(conv_ms, 4), pool_tail_host_ms=round(ms - conv_ms, 4), **layers)), flush=True)


def fid_leg(iters):
    from diffcodec_amd import lib, metrics as M
    g = torch.Generator().manual_seed(0)
    sd = {}
    for name, ci, co in zip(M.FID_BLOCKS, M.FID_CIN, M.FID_COUT):
        sd[f"{name}.conv.weight"] = torch.randn(co, ci, 3, 3, generator=g) * (2.0 / (9 * ci)) ** 0.5
        sd[f"{name}.bn.weight"] = 0.5 + torch.rand(co, generator=g)
        sd[f"{name}.bn.bias"] = 0.3 * torch.randn(co, generator=g)
        sd[f"{name}.bn.running_mean"] = 0.2 * torch.randn(co, generator=g)
        sd[f"{name}.bn.running_var"] = 0.5 + torch.rand(co, generator=g)
    model = M.FrechetInceptionDistance.from_state_dict(sd).to("cuda")
    wts = model._weights(torch.device("cuda"))
    stream = torch.cuda.current_stream().cuda_stream

    def timed(fn):
        for _ in range(3):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters

    flop = [2.0 * 32 * 149 * 149 * 27, 2.0 * 32 * 147 * 147 * 288, 2.0 * 64 * 147 * 147 * 288]
    gd = torch.Generator(device="cuda").manual_seed(0)
    for n in (16, 1):
        x = torch.randint(0, 256, (n, 512, 512, 3), dtype=torch.uint8, device="cuda", generator=gd)
        maps = model.maps(x)
        layers = {}
        for l in range(3):
            out = torch.empty_like(maps[l + 1])
            t = timed(lambda: lib.call("dc_fid_conv", l, maps[l].data_ptr(), n, wts.data_ptr(), out.data_ptr(), stream))
            assert torch.equal(out, maps[l + 1]), f"conv{l + 1} alone differs from the fused sequence"
            layers[f"conv{l + 1}"] = dict(us=round(t * 1e3, 1), tflops=round(n * flop[l] / (t * 1e-3) / 1e12, 1))
        t_feat = timed(lambda: model.features(x))
        f = model.features(x)
        t_acc = timed(lambda: model.update_features(f, real=True))
        t_upd = timed(lambda: model.update(x, real=True))
        model.reset()
        conv_ms = sum(v["us"] for v in layers.values()) / 1e3
        print(json.dumps(dict(fid="512x512", images=n, update_ms_per_call=round(t_upd, 4), update_ms_per_image=round(t_upd / n, 4),
                              features_ms=round(t_feat, 4), conv_ms=round(conv_ms, 4), resize_pool_host_ms=round(t_feat - conv_ms, 4),
                              accumulate_us=round(t_acc * 1e3, 1), **layers)), flush=True)


def fvd_leg(iters):
    from diffcodec_amd import metrics as M
    g = torch.Generator().manual_seed(0)
    sd = {}
    for name, ci, co, k, _ in M.fvd_units():
        sd[f"{name}.conv3d.weight"] = torch.randn(co, ci, k, k, k, generator=g) * (2.0 / (ci * k ** 3)) ** 0.5
        sd[f"{name}.bn.weight"] = 0.5 + torch.rand(co, generator=g)
        sd[f"{name}.bn.bias"] = 0.2 * torch.randn(co, generator=g)
        sd[f"{name}.bn.running_mean"] = 0.2 * torch.randn(co, generator=g)
        sd[f"{name}.bn.running_var"] = 0.5 + torch.rand(co, generator=g)
    sd["logits.conv3d.weight"] = torch.randn(400, 1024, 1, 1, 1, generator=g) / 32
    sd["logits.conv3d.bias"] = 0.1 * torch.randn(400, generator=g)
    model = M.FrechetVideoDistance.from_state_dict(sd).to("cuda")
    # multiply-adds of the Unit3D convolutions for one 16-frame video
    macs, shapes, cin = 0.0, M.fvd_endpoint_shapes(16), {}
    vol = {row[0]: sh[1] * sh[2] * sh[3] for row, sh in zip(M.FVD_NET, shapes)}
    for name, ci, co, k, _ in M.fvd_units():
        macs += float(vol[name.split(".")[0]]) * ci * co * k ** 3
    macs += 1024 * 400
    gd = torch.Generator(device="cuda").manual_seed(0)
    for n in (1, 8):
        x = torch.randint(0, 256, (n, 16, 512, 512, 3), dtype=torch.uint8, device="cuda", generator=gd)
        for _ in range(2):
            model.features(x)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            model.features(x)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / iters
        print(json.dumps(dict(fvd="16x512x512", videos=n, features_ms=round(ms, 3), ms_per_video=round(ms / n, 3),
                              gmac_per_video=round(macs / 1e9, 1), tflops=round(2 * macs * n / (ms * 1e-3) / 1e12, 1))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-lpips", action="store_true")
    ap.add_argument("--no-fid", action="store_true")
    ap.add_argument("--no-fvd", action="store_true")
    ap.add_argument("--only-fvd", action="store_true")
    ap.add_argument("--no-ssim", action="store_true")
    ap.add_argument("--lib", default=None, help="another build of libdiffcodec_hip.so (same ABI)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_metrics needs the GPU"
    from diffcodec_amd import lib, metrics as M
    if a.lib:
        lib.LIB_PATH = os.path.abspath(a.lib)
    if a.only_fvd:
        return fvd_leg(a.iters)
    g = torch.Generator(device="cuda").manual_seed(0)
    for h, w in () if a.no_ssim else ((512, 512), (1080, 1920)):
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
    if not a.no_lpips:
        lpips_leg(a.iters)
    if not a.no_fid:
        fid_leg(a.iters)
    if not a.no_fvd:
        fvd_leg(a.iters)


if __name__ == "__main__":
    main()
