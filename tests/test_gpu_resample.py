"""GPU: Pillow's 8-bit resize of csrc/resample.hip (diffcodec_amd.resample.resize_u8) against the integer restatement
tests/resample_ref.py, which tests/test_resample_ref.py ties to Pillow's bytes.  Every comparison is on bytes: torch.equal /
np.array_equal, no tolerance.  The shapes are the smallest at which each thing can break (the list is in each test)."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import fid_ref
import fvd_ref
import lpips_ref
import resample_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
SPAN = 256          # output pixels of one row per workgroup (csrc/resample.hip RS_SPAN)


def _dev(a, size, name):
    from diffcodec_amd.resample import resize_u8
    return resize_u8(torch.from_numpy(a).to(DEV), size, name).cpu().numpy()


# 37x53 -> 64x41: mixed up / down, non-integer ratios, both passes;  48x90 -> 48x48: vertical pass skipped (the 960x512 scoring case in
# small);  90x48 -> 48x48: horizontal pass skipped;  5x3 -> 2x7, 1x1 -> 3x2, 9x9 -> 1x1: clamped bounds at both ends, one-sample axes;
# 7x200 -> 7x3: a Lanczos table row of 401 entries, every output sums all 200 input samples;  7x200 -> 7x5: 140, 180 and 200 taps, a
# long and ragged tap loop;  20x300 -> 10x600: an output row of 600 pixels, wider than the 256 one workgroup covers (three
# workgroups per row, the last one partly empty).
@pytest.mark.parametrize("case", range(len(R.SMALL_CASES)))
def test_small_shapes_all_filters(case):
    (_, size) = R.SMALL_CASES[case]
    if case == 7:
        assert size[1] > 2 * SPAN
    a = R.small_input(case)
    for name in R.FILTERS:
        got = _dev(a, size, name)
        assert got.dtype == np.uint8 and np.array_equal(got, R.resize(a, size, name)), (case, name)


def test_long_tap_loops_really_are_long_and_ragged():
    bounds, _, ksize = R.table(200, 3, "lanczos")
    assert ksize == 401 and bounds[:, 1].tolist() == [200, 200, 200]
    bounds, _, ksize = R.table(200, 5, "lanczos")
    assert ksize == 241 and bounds[:, 1].tolist() == [140, 180, 200, 180, 140]


@pytest.mark.parametrize("c", [1, 3, 4])
def test_channel_counts(c):
    for case in (0, 3):
        a = R.small_input(case, c)
        for name in R.FILTERS:
            assert np.array_equal(_dev(a, R.SMALL_CASES[case][1], name), R.resize(a, R.SMALL_CASES[case][1], name)), (case, name)


def test_batch_of_distinct_images():
    a = R.random_bytes((3, 37, 53, 3), 31)
    assert not np.array_equal(a[0], a[1]) and not np.array_equal(a[1], a[2])
    for name in R.FILTERS:
        got = _dev(a, (64, 41), name)
        assert got.shape == (3, 64, 41, 3)
        for i in range(3):
            assert np.array_equal(got[i], R.resize(a[i], (64, 41), name)), (name, i)


def test_saturated_checkerboard_clips_on_both_sides():
    a = R.checkerboard(37, 53)
    for name in R.FILTERS:
        raw = R.first_pass_unclipped(a, (64, 41), name)
        if name != "bilinear":                                   # the negative lobes overshoot: the clip at 0 and at 255 both act
            assert int(raw.min()) < 0 and int(raw.max()) > 255, (name, int(raw.min()), int(raw.max()))
        assert np.array_equal(_dev(a, (64, 41), name), R.resize(a, (64, 41), name)), name


def test_strided_window_is_read_in_place():
    from diffcodec_amd.resample import resize_u8
    big = torch.from_numpy(R.random_bytes((2, 60, 80, 3), 41)).to(DEV)
    win = big[:, 8:45, 16:69]
    assert tuple(win.shape) == (2, 37, 53, 3) and not win.is_contiguous()
    for name in R.FILTERS:
        got = resize_u8(win, (64, 41), name)
        assert got.is_contiguous() and torch.equal(got, resize_u8(win.contiguous(), (64, 41), name))
        assert np.array_equal(got.cpu().numpy(), R.resize(win.cpu().numpy(), (64, 41), name))
    one = big[0, 8:45, 16:69]                                     # [H,W,C] form, only the vertical pass: strided rows
    assert np.array_equal(resize_u8(one, (20, 53), "bicubic").cpu().numpy(), R.resize(one.cpu().numpy(), (20, 53), "bicubic"))


@pytest.mark.parametrize("size", [(64, 41), (37, 41), (64, 53)])
def test_output_inside_guard_bytes(size):
    """The C-ABI on an output (and scratch) that lie inside larger allocations, run once over a prefill of 0x00 and once over 0xFF:
    the guard bytes keep the prefill (nothing is written outside) and both results equal the restatement (every byte inside is
    written: a byte left alone would differ in one of the two runs)."""
    from diffcodec_amd import lib
    from diffcodec_amd.resample import coeffs
    n, hi, wi, c = 2, 37, 53, 3
    h, w = size
    a = R.random_bytes((n, hi, wi, c), 51)
    x = torch.from_numpy(a).to(DEV)
    want = torch.from_numpy(R.resize(a, size, "lanczos"))
    th = tuple(t.to(DEV) if torch.is_tensor(t) else t for t in coeffs(wi, w, "lanczos")) if w != wi else None
    tv = tuple(t.to(DEV) if torch.is_tensor(t) else t for t in coeffs(hi, h, "lanczos")) if h != hi else None
    guard = 4096
    nout, nws = n * h * w * c, lib.load().dc_resample_ws_bytes(n, hi, w, c)
    assert nws == n * hi * w * c
    strides = (ctypes.c_longlong * 4)(x.stride(0), x.stride(3), x.stride(1), x.stride(2))
    for fill in (0x00, 0xFF):
        obuf = torch.full((guard + nout + guard,), fill, dtype=torch.uint8, device=DEV)
        wbuf = torch.full((guard + nws + guard,), fill, dtype=torch.uint8, device=DEV)
        lib.call("dc_resample_u8", x.data_ptr(), strides, n, hi, wi, c, h, w,
                 th[1].data_ptr() if th else 0, th[0].data_ptr() if th else 0, th[2] if th else 0,
                 tv[1].data_ptr() if tv else 0, tv[0].data_ptr() if tv else 0, tv[2] if tv else 0,
                 wbuf[guard:].data_ptr(), obuf[guard:].data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        o, s = obuf.cpu(), wbuf.cpu()
        assert bool((o[:guard] == fill).all()) and bool((o[guard + nout:] == fill).all()), "output guard bytes overwritten"
        assert bool((s[:guard] == fill).all()) and bool((s[guard + nws:] == fill).all()), "scratch guard bytes overwritten"
        assert torch.equal(o[guard:guard + nout].reshape(n, h, w, c), want), fill


def test_workload_sizes():
    a = R.random_bytes((2, 1024, 1920, 3), 61)
    assert np.array_equal(_dev(a, (512, 512), "bilinear"), R.resize(a, (512, 512), "bilinear"))
    b = R.random_bytes((1, 270, 480, 3), 62)
    assert np.array_equal(_dev(b, (1080, 1920), "lanczos"), R.resize(b, (1080, 1920), "lanczos"))


def test_repeatable_graph_replay_and_host_tensors():
    from diffcodec_amd.resample import resize_u8
    a = torch.from_numpy(R.random_bytes((2, 37, 53, 3), 71))
    x = a.to(DEV)
    first = resize_u8(x, (64, 41), "bicubic")
    assert torch.equal(first, resize_u8(x, (64, 41), "bicubic"))
    host = resize_u8(a, (64, 41), "bicubic")
    assert not host.is_cuda and torch.equal(host, first.cpu())
    same = resize_u8(x, (37, 53), "bicubic")                      # equal sizes on both axes: a copy
    assert torch.equal(same, x) and same.data_ptr() != x.data_ptr()
    one = resize_u8(x[0], (64, 41), "bicubic")
    assert tuple(one.shape) == (64, 41, 3) and torch.equal(one, first[0])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                 # the tables are cached: nothing in the call synchronises
        captured = resize_u8(x, (64, 41), "bicubic")
    captured.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured, first)


# ------------------------------------------------------------------------------------------- scoring
H, W, S = 192, 352, (176, 176)          # 176: the smallest side MS-SSIM takes


class _Stub:
    """`n` decoded frames of seeded bytes (a smooth field, so the scores are ordinary values) and their ground truth, on the device"""

    def __init__(self, n, h, w, seed):
        g = torch.Generator().manual_seed(seed)
        coarse = torch.rand(n, 3, h // 16 + 2, w // 16 + 2, generator=g)
        base = torch.nn.functional.interpolate(coarse, size=(h, w), mode="bicubic", align_corners=False)
        q = lambda t: (t * 255).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
        self.truth = q(base + 0.05 * torch.rand(n, 3, h, w, generator=g))
        self.decoded = q(base + 0.08 * torch.randn(n, 3, h, w, generator=g))
        self.frames = {i + 1: self.decoded[i].to(DEV) for i in range(n)}

    def ground_truth(self, frame):
        return self.truth[frame - 1].to(DEV)


class _Resized:
    """the same clip with both sides resized by the restatement on the host"""

    def __init__(self, stub, size):
        self.truth = torch.from_numpy(R.resize(stub.truth.numpy(), size, "bilinear"))
        self.frames = {f: torch.from_numpy(R.resize(t.cpu().numpy(), size, "bilinear")).to(DEV) for f, t in stub.frames.items()}

    def ground_truth(self, frame):
        return self.truth[frame - 1].to(DEV)


@pytest.fixture(scope="module")
def models():
    from diffcodec_amd import metrics
    return (metrics.LPIPS.from_state_dict(lpips_ref.synth_weights(seed=20)).to(DEV),
            metrics.FrechetInceptionDistance.from_state_dict(fid_ref.synth_weights(seed=20)).to(DEV))


def test_score_size_equals_scoring_the_resized_frames(models):
    """the same kernels on the same bytes: anything but equal bits is a wiring fault"""
    from diffcodec_amd import clip_decode as CD, metrics
    lp, fid = models
    stub = _Stub(3, H, W, 81)
    small = _Resized(stub, S)
    fid.reset()
    got = CD.score_frames(stub.frames, stub, lpips=lp, fid=fid, score_size=S)
    got_state = [t.clone() for t in fid.state()]
    got_fid = fid.compute()
    fid.reset()
    want = CD.score_frames(small.frames, small, lpips=lp, fid=fid)
    assert sorted(got) == [1, 2, 3] and got == want and all(sorted(s) == ["lpips", "ms_ssim", "psnr"] for s in got.values())
    assert all(torch.equal(a, b) for a, b in zip(got_state, fid.state())) and got_fid == fid.compute()
    unresized = CD.score_frames(stub.frames, stub, lpips=lp)
    assert all(unresized[f]["psnr"] != got[f]["psnr"] for f in got)          # the resize does change what is scored
    # the reference's entry point on the same frames: the matching means, the same FID
    m = metrics.calculate_metrics_batch(stub.truth, stub.decoded, lpips=lp, fid=fid, size=S)
    assert sorted(m) == ["FID", "LPIPS", "MS-SSIM", "PSNR"]
    assert m["PSNR"] == sum(want[f]["psnr"] for f in (1, 2, 3)) / 3 and m["MS-SSIM"] == sum(want[f]["ms_ssim"] for f in (1, 2, 3)) / 3
    assert m["LPIPS"] == sum(want[f]["lpips"] for f in (1, 2, 3)) / 3 and m["FID"] == got_fid
    lists = metrics.calculate_metrics_batch([t for t in stub.truth], [t.to(DEV) for t in stub.decoded], size=S)
    assert sorted(lists) == ["MS-SSIM", "PSNR"] and lists["PSNR"] == m["PSNR"] and lists["MS-SSIM"] == m["MS-SSIM"]
    with pytest.raises(ValueError, match="ground truth"):                   # the shape check stays on the unresized pair
        CD.score_frames(stub.frames, small, score_size=S)
    fid.reset()


def test_fvd_through_score_size():
    """9 frames, the fewest the I3D path takes"""
    from diffcodec_amd import clip_decode as CD, metrics
    model = metrics.FrechetVideoDistance.from_state_dict(fvd_ref.synth_weights(1234)).to(DEV)
    stub = _Stub(9, H, W, 91)
    small = _Resized(stub, S)
    scores = {f: dict(psnr=30.0) for f in stub.frames}
    truth = {f: stub.ground_truth(f) for f in stub.frames}
    got = CD.fvd_of_frames(model, stub.frames, truth, scores, score_size=S)
    want = CD.fvd_of_frames(model, small.frames, {f: small.ground_truth(f) for f in small.frames}, scores)
    assert isinstance(got, float) and math.isfinite(got) and got > 0 and got == want
    assert got != CD.fvd_of_frames(model, stub.frames, truth, scores)
    m = metrics.calculate_metrics_batch(stub.truth, stub.decoded, fvd=model, size=S)
    assert sorted(m) == ["FVD", "MS-SSIM", "PSNR"] and m["FVD"] == got


# ------------------------------------------------------------------------------------------- loading
def test_device_resize_loads_the_same_bytes(tmp_path):
    from PIL import Image
    from diffcodec_amd import clip_decode as CD
    from diffcodec_amd.io_utils import load_controls_and_flows, write_flo
    g = np.random.default_rng(5)
    base = tmp_path / "v"
    sub = "optical_flow_gop_4_raft"
    for d in ("images", os.path.join("optical_flow", sub), os.path.join("optical_flow_bwd", sub)):
        os.makedirs(base / d)
    for i in (0, 4):
        Image.fromarray(R.random_bytes((45, 70, 3), 100 + i)).save(base / "images" / f"frame_{i:04d}.png")
    write_flo(str(base / "optical_flow" / sub / "flow_0000_0001.flo"), g.normal(0, 2, (45, 70, 2)))
    write_flo(str(base / "optical_flow_bwd" / sub / "flow_0004_0001.flo"), g.normal(0, 2, (45, 70, 2)))
    size = (32, 48)                                               # as the loaders pass it to Pillow: (w, h) = (32, 48)
    on = CD.DirectorySource(str(tmp_path), "v", 4, size, device=DEV, device_resize=True)
    off = CD.DirectorySource(str(tmp_path), "v", 4, size, device=DEV)
    a = load_controls_and_flows(*on.paths(1, 0, 4), size=size, device=DEV, device_resize=True)
    b = load_controls_and_flows(*on.paths(1, 0, 4), size=size, device=DEV, device_resize=False)
    assert a[0].is_cuda and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    ca, cb = on.controls(1, 0, 4), off.controls(1, 0, 4)
    assert torch.equal(ca[0], cb[0]) and torch.equal(ca[1], cb[1])
    ga, gb = on.ground_truth(4), off.ground_truth(4)
    assert ga.is_cuda and tuple(ga.shape) == (48, 32, 3) and torch.equal(ga, gb)
