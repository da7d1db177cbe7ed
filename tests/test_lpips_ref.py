"""CPU: the fp64 LPIPS restatement tests/lpips_ref.py against hand-computed values, and the host side of diffcodec_amd.metrics.LPIPS
(state-dict layouts, packing, argument checks, summarize) — no kernel runs."""
import math

import pytest
import torch

import lpips_ref as R


@pytest.fixture(scope="module")
def sd():
    return R.synth_weights(seed=3)


def _images(n, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, 3, h, w, generator=g), torch.rand(n, 3, h, w, generator=g)


def test_identical_inputs_give_zero(sd):
    x, _ = _images(2, 40, 37, 1)
    v, layers = R.lpips(sd, x, x.clone())
    assert torch.equal(v, torch.zeros(2, dtype=torch.float64)) and all(torch.equal(t, torch.zeros(2, dtype=torch.float64)) for t in layers)


def test_normalize_is_two_x_minus_one(sd):
    x, y = _images(1, 35, 33, 2)
    a, _ = R.lpips(sd, x, y, normalize=True)
    b, _ = R.lpips(sd, 2 * x.double() - 1, 2 * y.double() - 1)
    assert torch.equal(a, b) and a.item() > 0
    c, _ = R.lpips(sd, x, y)
    assert a.item() != c.item()


def test_uint8_frames_are_divided_by_255(sd):
    g = torch.Generator().manual_seed(4)
    u = torch.randint(0, 256, (1, 33, 31, 3), dtype=torch.uint8, generator=g)
    v = torch.randint(0, 256, (1, 33, 31, 3), dtype=torch.uint8, generator=g)
    a, _ = R.lpips(sd, u, v)
    b, _ = R.lpips(sd, u.permute(0, 3, 1, 2).double() / 255, v.permute(0, 3, 1, 2).double() / 255)
    assert torch.equal(a, b)


def test_map_sizes_from_the_minimum_image(sd):
    from diffcodec_amd import metrics as M
    x, _ = _images(1, 31, 31, 5)
    f = R.features(sd, x)
    assert [tuple(t.shape) for t in f] == [(1, 64, 7, 7), (1, 192, 3, 3), (1, 384, 1, 1), (1, 256, 1, 1), (1, 256, 1, 1)]
    assert M.lpips_map_sizes(31, 31) == [(7, 7), (3, 3), (1, 1), (1, 1), (1, 1)]
    for h, w in ((512, 512), (67, 95), (270, 480), (1080, 1920)):
        x, _ = _images(1, h, w, 6)
        assert M.lpips_map_sizes(h, w)[0] == tuple(R.features(sd, x)[0].shape[2:])
    assert M.lpips_map_sizes(512, 512) == [(127, 127), (63, 63), (31, 31), (31, 31), (31, 31)]
    assert M.lpips_map_sizes(67, 95) == [(16, 23), (7, 11), (3, 5), (3, 5), (3, 5)]


def test_conv1_padding_is_zero_in_the_scaled_space(sd):
    """a constant image equal to the shift is zero after scaling: every relu1 value is relu(bias), borders included"""
    x = torch.tensor(R.SHIFT, dtype=torch.float64).view(1, 3, 1, 1).expand(1, 3, 31, 31)
    f1 = R.features(sd, x)[0]
    b = sd["net.slice1.0.bias"].double()
    assert (f1 - torch.relu(b).view(1, -1, 1, 1)).abs().max().item() < 1e-15


def test_hand_computed_one_pixel_tail():
    # two channels, one pixel: x = (3, 4) -> (0.6, 0.8); y = (0, 2) -> (0, 1); w = (0.5, 2): 0.5 * 0.36 + 2 * 0.04 = 0.26
    fx = torch.tensor([3.0, 4.0], dtype=torch.float64).view(1, 2, 1, 1)
    fy = torch.tensor([0.0, 2.0], dtype=torch.float64).view(1, 2, 1, 1)
    w = torch.tensor([0.5, 2.0], dtype=torch.float64)
    assert abs(R.tail(fx, fy, w).item() - 0.26) < 1e-9
    # an all-zero pixel normalises to zero, not NaN: the distance is the weighted square of the other side's unit vector
    z = torch.zeros(1, 2, 1, 1, dtype=torch.float64)
    assert abs(R.tail(fx, z, w).item() - (0.5 * 0.36 + 2 * 0.64)) < 1e-9
    assert R.tail(z, z, w).item() == 0.0
    # NormFix: x / sqrt(sum (x^2 + 1e-8))
    nx, ny = math.sqrt(25 + 2e-8), math.sqrt(4 + 2e-8)
    want = 0.5 * (3 / nx) ** 2 + 2 * (4 / nx - 2 / ny) ** 2
    assert abs(R.tail(fx, fy, w, normfix=True).item() - want) < 1e-15
    assert R.tail(z, z, w, normfix=True).item() == 0.0
    # the spatial mean: two pixels, the second identical on both sides
    fx2, fy2 = torch.cat([fx, fx], 3), torch.cat([fy, fx], 3)
    assert abs(R.tail(fx2, fy2, w).item() - 0.13) < 1e-9


def test_both_state_dict_layouts_pack_to_the_same_tensor(sd):
    from diffcodec_amd import metrics as M
    feats, lins = R.synth_weights(seed=3, layout="torchvision")
    a = M.pack_lpips_weights(sd)
    b = M.pack_lpips_weights(feats, lins)
    c = M.pack_lpips_weights({**feats, **lins})
    assert a.dtype == torch.float32 and torch.equal(a, b) and torch.equal(a, c)
    m = M.LPIPS.from_state_dict(feats, lins)                      # checks the length against the library's layout
    assert torch.equal(m.packed, a) and M.LPIPS().load_state_dict(sd).packed.numel() == a.numel()
    # layout: conv1 K-major [364][64] with a zero last row, then its bias
    w1 = sd["net.slice1.0.weight"]
    assert torch.equal(a[:363 * 64].view(363, 64), w1.reshape(64, 363).t()) and not a[363 * 64:364 * 64].any()
    assert torch.equal(a[364 * 64:364 * 64 + 64], sd["net.slice1.0.bias"])
    assert torch.equal(a[-256:], sd["lin4.model.1.weight"].view(-1))
    w2 = sd["net.slice2.3.weight"]
    o2 = 364 * 64 + 64
    assert a[o2 + (5 * 25 + 7) * 192 + 17].item() == w2[17, 5, 1, 2].item()


def test_bad_arguments_raise(sd):
    from diffcodec_amd import metrics as M
    for key in ("net.slice3.6.weight", "net.slice5.10.bias", "lin2.model.1.weight"):
        bad = {k: v for k, v in sd.items() if k != key}
        with pytest.raises(ValueError, match=key.replace(".", r"\.")):
            M.LPIPS().load_state_dict(bad)
    bad = dict(sd)
    bad["net.slice2.3.weight"] = torch.zeros(192, 64, 3, 3)
    with pytest.raises(ValueError, match=r"net\.slice2\.3\.weight"):
        M.LPIPS.from_state_dict(bad)
    bad = dict(sd)
    bad["lin0.model.1.weight"] = torch.zeros(64)
    with pytest.raises(ValueError, match=r"lin0\.model\.1\.weight"):
        M.LPIPS.from_state_dict(bad)
    feats, lins = R.synth_weights(seed=3, layout="torchvision")
    with pytest.raises(ValueError, match=r"lin0\.model\.1\.weight"):
        M.LPIPS.from_state_dict(feats)
    with pytest.raises(NotImplementedError):
        M.LPIPS(net="vgg")
    with pytest.raises(NotImplementedError):
        M.LPIPS(version="0.0")
    m = M.LPIPS.from_state_dict(sd)
    with pytest.raises(ValueError, match="3-channel"):
        m(torch.zeros(1, 1, 64, 64), torch.zeros(1, 1, 64, 64))
    with pytest.raises(ValueError, match="31"):
        m(torch.zeros(1, 3, 30, 30), torch.zeros(1, 3, 30, 30))
    with pytest.raises(ValueError, match="31"):
        m.features(torch.zeros(1, 64, 30, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="same dimensions"):
        m(torch.zeros(1, 3, 64, 64), torch.zeros(1, 3, 64, 65))
    with pytest.raises(RuntimeError, match="no weights"):
        M.LPIPS()._weights(torch.device("cuda", 0))
    assert M.lib.load().dc_lpips_ws_bytes(1, 30, 31) == -1 and M.lib.load().dc_lpips_ws_bytes(1, 31, 30) == -1
    assert M.lib.load().dc_lpips_ws_bytes(1, 31, 31) > 0
    ws = M.lib.load().dc_lpips_ws_bytes(1, 512, 512)
    assert 24e6 < ws < 27e6                                        # about 12.4 MB of maps per image


def test_summarize_with_and_without_lpips():
    from diffcodec_amd import metrics as M
    plain = {1: dict(psnr=30.0, ms_ssim=0.9), 2: dict(psnr=32.0, ms_ssim=0.95), 3: dict(psnr=float("inf"), ms_ssim=1.0)}
    s = M.summarize(plain)
    assert set(s) == {"psnr", "ms_ssim", "frames", "identical"}                 # no lpips key when no score carries it
    assert s["psnr"] == 31.0 and abs(s["ms_ssim"] - 0.925) < 1e-15 and s["frames"] == 2 and s["identical"] == 1
    with_l = {f: dict(v, lpips=l) for (f, v), l in zip(plain.items(), (0.1, 0.3, 0.0))}
    s = M.summarize(with_l)
    assert set(s) == {"psnr", "ms_ssim", "lpips", "frames", "identical"} and s["frames"] == 2
    assert abs(s["lpips"] - 0.2) < 1e-15 and s["psnr"] == 31.0
    e = M.summarize({1: dict(psnr=float("inf"), ms_ssim=1.0, lpips=0.0)})
    assert e["frames"] == 0 and math.isnan(e["lpips"]) and math.isnan(e["psnr"])
