"""CPU: the fp64 restatement of PSNR / SSIM / MS-SSIM (tests/metrics_ref.py) is pinned to independent evaluations, and
diffcodec_amd.metrics refuses what pytorch_msssim refuses before it touches a device."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import metrics_ref as R


def _pair(shape, seed, noise=20.0):
    g = torch.Generator().manual_seed(seed)
    n, c, h, w = shape
    base = F.interpolate(torch.rand(n, c, h // 8 + 2, w // 8 + 2, generator=g, dtype=torch.float64), size=(h, w), mode="bilinear",
                         align_corners=False) * 255.0
    return base, (base + noise * torch.randn(shape, generator=g, dtype=torch.float64)).clamp(0, 255)


def test_one_scale_matches_scipy_correlate1d():
    """window orientation and valid crop: SSIM / CS means of one scale against scipy.ndimage.correlate1d along axis 0 then 1"""
    from scipy.ndimage import correlate1d
    X, Y = _pair((2, 3, 37, 53), 0)
    ws, L, (k1, k2) = 7, 255.0, (0.01, 0.03)
    g = R.window(ws, 1.5)
    got_s, got_cs = R.ssim_cs(X, Y, L, g)
    gn, h = g.numpy(), ws // 2

    def filt(a):
        a = correlate1d(a, gn, axis=0, mode="constant")[h:a.shape[0] - h]
        return correlate1d(a, gn, axis=1, mode="constant")[:, h:a.shape[1] - h]

    for n in range(2):
        for c in range(3):
            x, y = X[n, c].numpy(), Y[n, c].numpy()
            mx, my = filt(x), filt(y)
            sxx, syy, sxy = filt(x * x) - mx * mx, filt(y * y) - my * my, filt(x * y) - mx * my
            cs = (2 * sxy + (k2 * L) ** 2) / (sxx + syy + (k2 * L) ** 2)
            s = (2 * mx * my + (k1 * L) ** 2) / (mx * mx + my * my + (k1 * L) ** 2) * cs
            assert mx.shape == (37 - ws + 1, 53 - ws + 1)
            assert abs(got_s[n, c].item() - s.mean()) < 1e-12 and abs(got_cs[n, c].item() - cs.mean()) < 1e-12


def test_asymmetric_window_orientation():
    """an asymmetric window distinguishes correlation from convolution and H from W"""
    from scipy.ndimage import correlate1d
    x = torch.rand(1, 1, 9, 11, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    g = torch.tensor([0.1, 0.2, 0.7], dtype=torch.float64)
    got = R.gaussian_filter(x, g)[0, 0].numpy()
    a = correlate1d(x[0, 0].numpy(), g.numpy(), axis=0, mode="constant")[1:-1]
    a = correlate1d(a, g.numpy(), axis=1, mode="constant")[:, 1:-1]
    assert np.abs(got - a).max() < 1e-15


@pytest.mark.parametrize("hw", [(8, 8), (9, 8), (8, 11), (13, 7), (1, 1), (2, 3)])
def test_pool_matches_avg_pool2d(hw):
    x = torch.rand(2, 3, *hw, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    ref = F.avg_pool2d(x, kernel_size=2, padding=[s % 2 for s in hw])
    assert torch.equal(R.pool(x), ref) or (R.pool(x) - ref).abs().max() < 1e-15


def test_identical_inputs_give_one():
    X, _ = _pair((2, 3, 170, 181), 3)
    assert R.ms_ssim(X, X).item() == 1.0
    assert R.ssim(X, X).item() == 1.0
    assert torch.isinf(R.psnr(X, X)).all()


def test_data_range_one_on_scaled_values_equals_255():
    X, Y = _pair((2, 3, 200, 170), 4)
    X, Y = X.round(), Y.round()
    for f in (R.ms_ssim, R.ssim):
        a = f(X / 255.0, Y / 255.0, data_range=1.0, size_average=False)
        b = f(X, Y, data_range=255, size_average=False)
        assert (a - b).abs().max().item() < 1e-12
    a, b = R.psnr(X / 255.0, Y / 255.0, 1.0), R.psnr(X, Y, 255.0)
    assert ((a - b).abs() / b).max().item() < 1e-12


def test_uint8_frames_are_nhwc():
    X, Y = _pair((1, 3, 170, 170), 5)
    xu, yu = X.round().to(torch.uint8).permute(0, 2, 3, 1).contiguous(), Y.round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    assert R.ms_ssim(xu, yu).item() == R.ms_ssim(X.round(), Y.round()).item()


def test_summarize_leaves_identical_frames_out():
    from diffcodec_amd import metrics as M
    s = M.summarize({1: dict(psnr=30.0, ms_ssim=0.9), 2: dict(psnr=float("inf"), ms_ssim=1.0), 3: dict(psnr=34.0, ms_ssim=0.8)})
    assert s == dict(psnr=32.0, ms_ssim=pytest.approx(0.85), frames=2, identical=1)
    e = M.summarize({})
    assert e["frames"] == 0 and e["identical"] == 0 and np.isnan(e["psnr"])


def test_module_raises_the_library_exceptions_before_touching_a_device(monkeypatch):
    """shape / dtype mismatch and an even window: ValueError; a side <= (ws - 1) * 16 in ms_ssim: AssertionError.  Nothing reaches
    the device (no library load, no copy)."""
    from diffcodec_amd import lib, metrics as M

    def no_device(*a, **k):
        raise AssertionError("touched the device")

    monkeypatch.setattr(lib, "load", no_device)
    monkeypatch.setattr(M, "_to_device", no_device)
    x = torch.rand(1, 3, 200, 200)
    with pytest.raises(ValueError):
        M.ms_ssim(x, torch.rand(1, 3, 200, 201))
    with pytest.raises(ValueError):
        M.ssim(x, x.double())
    with pytest.raises(ValueError):
        M.psnr(x, torch.rand(1, 3, 200, 199))
    with pytest.raises(ValueError, match="odd"):
        M.ms_ssim(x, x, win_size=10)
    with pytest.raises(ValueError, match="odd"):
        M.ssim(x, x, win=torch.ones(3, 1, 1, 4) / 4)
    with pytest.raises(AssertionError, match="larger than 160"):
        M.ms_ssim(torch.rand(1, 3, 160, 400), torch.rand(1, 3, 160, 400))
    with pytest.raises(AssertionError, match="larger than 96"):
        M.ms_ssim(x[..., :96, :], x[..., :96, :], win_size=7)
    with pytest.raises(ValueError):
        M.ssim(torch.rand(1, 1, 10, 40), torch.rand(1, 1, 10, 40))          # H < window: the library warns, here it is refused
    with pytest.raises(ValueError):
        M.ms_ssim(torch.rand(1, 1, 300, 300), torch.rand(1, 1, 300, 300), win_size=17)     # window > 15
    with pytest.raises(ValueError):
        M.ssim(torch.rand(2, 3, 40), torch.rand(2, 3, 40))                  # not 4-D
