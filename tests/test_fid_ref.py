"""CPU: the fp64 FID restatement tests/fid_ref.py against hand-written loops, numpy and scipy, and the host side of
diffcodec_amd.metrics.FrechetInceptionDistance (argument checks, state-dict keys, packing, merge_state / compute) - no kernel runs."""
import math

import numpy as np
import pytest
import torch

import fid_ref as R


@pytest.fixture(scope="module")
def sd():
    return R.synth_weights(seed=3)


def _loop_resize(x, points):
    """the rule of the class docstring written out per output pixel, for [H,W] fp64 `x` at the (oy, ox) in `points`"""
    H, W = x.shape
    out = {}
    for oy, ox in points:
        py, px = oy * (H / 299), ox * (W / 299)
        y0, x0 = math.floor(py), math.floor(px)
        y1, x1 = min(y0 + 1, H - 1), min(x0 + 1, W - 1)
        ly, lx = py - y0, px - x0
        top = x[y0, x0] + (x[y0, x1] - x[y0, x0]) * lx
        bot = x[y1, x0] + (x[y1, x1] - x[y1, x0]) * lx
        out[(oy, ox)] = float(top + (bot - top) * ly)
    return out


def test_resize_identity_and_hand_written_loop():
    g = torch.Generator().manual_seed(1)
    x = torch.randint(0, 256, (2, 3, 299, 299), generator=g).double()
    assert torch.equal(R.resize(x), x)                                     # l = 0 everywhere
    points = [(0, 0), (1, 1), (149, 150), (150, 149), (297, 298), (298, 297), (298, 298), (0, 298), (298, 0), (17, 233)]
    for h, w in ((2, 3), (600, 301), (1, 1), (5, 7)):
        x = torch.randint(0, 256, (1, 2, h, w), generator=g).double()
        y = R.resize(x)
        assert y.shape == (1, 2, 299, 299)
        for c in range(2):
            for (oy, ox), want in _loop_resize(x[0, c], points).items():
                assert abs(y[0, c, oy, ox].item() - want) <= 1e-12 * max(1.0, abs(want)), (h, w, c, oy, ox)
    # the i1 clamp: upsampling 2 x 3, the last output row / column lies past the last input sample and blends it with itself
    x = torch.tensor([[1.0, 2.0, 4.0], [8.0, 16.0, 32.0]]).view(1, 1, 2, 3)
    y = R.resize(x)[0, 0]
    assert y[298, 298].item() == 32.0 and y[0, 0].item() == 1.0
    assert math.floor(298 * (2 / 299)) == 1 and math.floor(298 * (3 / 299)) == 2
    assert abs(y[298, 0].item() - 8.0) < 1e-12 and abs(y[0, 298].item() - 4.0) < 1e-12
    lx = 100 * (3 / 299) - 1
    assert abs(y[0, 100].item() - (2.0 + 2.0 * lx)) < 1e-12
    # downsampling 600 x 301 without the half-pixel offset: output (1, 0) sits at input row 600 / 299
    x = torch.arange(600 * 301, dtype=torch.float64).view(1, 1, 600, 301)
    ly = 600 / 299 - 2
    assert abs(R.resize(x)[0, 0, 1, 0].item() - (2 * 301 + 301 * ly)) < 1e-9


def test_input_forms_and_map_sizes(sd):
    g = torch.Generator().manual_seed(2)
    u = torch.randint(0, 256, (2, 37, 41, 3), dtype=torch.uint8, generator=g)
    m = R.maps(sd, u)
    assert [tuple(t.shape) for t in m] == [(2, 3, 299, 299), (2, 32, 149, 149), (2, 32, 147, 147), (2, 64, 147, 147), (2, 64, 73, 73)]
    assert all(t.dtype == torch.float64 for t in m)
    assert m[0].min().item() >= -1.0 and m[0].max().item() <= 127 / 128
    f = R.features(sd, u)
    assert f.shape == (2, 64) and torch.equal(f, m[4].mean((2, 3)))
    # a float image in [0,1] is truncated to 8 bits: u / 255 gives back u, and a value just below a step gives the step below
    assert torch.equal(R.as_u8_nchw64(u.permute(0, 3, 1, 2).float() / 255, normalize=True), R.as_u8_nchw64(u))
    assert R.as_u8_nchw64(torch.full((1, 3, 1, 1), 0.9999), normalize=True).unique().tolist() == [254.0]
    assert torch.equal(R.features(sd, u.permute(0, 3, 1, 2).float() / 255, normalize=True), f)
    # eval BatchNorm with eps 1e-3 on a constant image: conv of a constant, then the affine map, then the ReLU
    x = torch.full((1, 4, 4, 3), 192, dtype=torch.uint8)
    w = sd["Conv2d_1a_3x3.conv.weight"].double()
    bn = {k: sd[f"Conv2d_1a_3x3.bn.{k}"].double() for k in ("weight", "bias", "running_mean", "running_var")}
    want = torch.relu((0.5 * w.sum((1, 2, 3)) - bn["running_mean"]) / torch.sqrt(bn["running_var"] + 1e-3) * bn["weight"] + bn["bias"])
    assert (R.maps(sd, x)[1][0, :, 70, 70] - want).abs().max().item() < 1e-14


def _rows(n, seed, rank=64):
    g = torch.Generator().manual_seed(seed)
    a = torch.rand(n, rank, generator=g, dtype=torch.float64) @ torch.rand(rank, 64, generator=g, dtype=torch.float64) / rank
    b = a * (1 + 0.2 * torch.rand(n, 64, generator=g, dtype=torch.float64)) + 0.01
    return a, b


def _sqrtm_fid(a, b):
    """the form of the reference's frechet_distance (fvd.py:287-293): np.cov and scipy.linalg.sqrtm"""
    from scipy import linalg
    a, b = a.numpy(), b.numpy()
    mu1, mu2 = a.mean(0), b.mean(0)
    s1, s2 = np.cov(a, rowvar=False), np.cov(b, rowvar=False)
    covmean = linalg.sqrtm(s1.dot(s2))
    if np.iscomplexobj(covmean):
        covmean = covmean.real
    d = mu1 - mu2
    return float(d.dot(d) + np.trace(s1) + np.trace(s2) - 2 * np.trace(covmean))


@pytest.mark.parametrize("n", [72, 8])
def test_eigenvalue_form_matches_sqrtm(n):
    a, b = _rows(n, seed=n)
    v, want = R.fid(a, b), _sqrtm_fid(a, b)
    assert want > 1e-4 and abs(v - want) <= 1e-6 * want, (n, v, want)


def test_stats_from_sums_and_merge():
    a, _ = _rows(40, seed=5)
    n, s, sq = R.sums(a)
    mu, cov = R.stats(n, s, sq)
    assert np.abs(mu.numpy() - a.numpy().mean(0)).max() < 1e-14
    c = np.cov(a.numpy(), rowvar=False)
    assert np.abs(cov.numpy() - c).max() <= 1e-10 * np.abs(c).max()
    n1, s1, q1 = R.sums(a[:17])
    n2, s2, q2 = R.sums(a[17:])
    mu_m, cov_m = R.stats(n1 + n2, s1 + s2, q1 + q2)
    assert (mu_m - mu).abs().max().item() < 1e-14 and (cov_m - cov).abs().max().item() <= 1e-10 * np.abs(c).max()
    assert R.fid(a, a) < 1e-9


def _state(f):
    n, s, sq = R.sums(f)
    return torch.cat([torch.tensor([float(n)], dtype=torch.float64), s, sq.reshape(-1)])


def test_class_host_side(sd):
    from diffcodec_amd import metrics as M
    for feature in (192, 768, 2048, "64"):
        with pytest.raises(NotImplementedError):
            M.FrechetInceptionDistance(feature=feature)
    for key in ("Conv2d_1a_3x3.conv.weight", "Conv2d_2a_3x3.bn.running_var", "Conv2d_2b_3x3.bn.bias"):
        bad = {k: v for k, v in sd.items() if k != key}
        with pytest.raises(ValueError, match=key.replace(".", r"\.")):
            M.FrechetInceptionDistance().load_state_dict(bad)
    bad = dict(sd)
    bad["Conv2d_2b_3x3.conv.weight"] = torch.zeros(64, 32, 1, 1)
    with pytest.raises(ValueError, match=r"Conv2d_2b_3x3\.conv\.weight"):
        M.FrechetInceptionDistance.from_state_dict(bad)
    bad = dict(sd)
    bad["Conv2d_1a_3x3.bn.running_mean"] = torch.zeros(64)
    with pytest.raises(ValueError, match=r"Conv2d_1a_3x3\.bn\.running_mean"):
        M.FrechetInceptionDistance.from_state_dict(bad)
    m = M.FrechetInceptionDistance.from_state_dict(sd)                     # ignores Conv2d_3b_1x1.*; checks the library's length
    p = m.packed
    assert p.dtype == torch.float32 and p.numel() == 28 * 32 + 64 + 288 * 32 + 64 + 288 * 64 + 128 == M.lib.load().dc_fid_weight_floats()
    w1 = sd["Conv2d_1a_3x3.conv.weight"]
    assert torch.equal(p[:27 * 32].view(27, 32), w1.reshape(32, 27).t()) and not p[27 * 32:28 * 32].any()
    bn = {k: sd[f"Conv2d_1a_3x3.bn.{k}"].double() for k in ("weight", "bias", "running_mean", "running_var")}
    s = bn["weight"] / torch.sqrt(bn["running_var"] + 1e-3)
    assert torch.equal(p[896:928], s.float()) and torch.equal(p[928:960], (bn["bias"] - bn["running_mean"] * s).float())
    o3 = 960 + 288 * 32 + 64
    assert p[o3 + (5 * 9 + 7) * 64 + 17].item() == sd["Conv2d_2b_3x3.conv.weight"][17, 5, 2, 1].item()
    with pytest.raises(ValueError, match="normalize=True"):
        m.update(torch.zeros(1, 3, 8, 8), real=True)
    with pytest.raises(ValueError, match="uint8"):
        M.FrechetInceptionDistance.from_state_dict(sd, normalize=True).update(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), real=True)
    with pytest.raises(ValueError, match="3-channel"):
        m.features(torch.zeros(1, 8, 8, 4, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no weights"):
        M.FrechetInceptionDistance()._weights(torch.device("cuda", 0))
    L = M.lib.load()
    assert L.dc_fid_ws_bytes(0, 8, 8) == -1 and L.dc_fid_ws_bytes(1, 0, 8) == -1 and L.dc_fid_ws_bytes(1, 8, 0) == -1
    assert 12e6 < L.dc_fid_ws_bytes(1, 512, 512) == L.dc_fid_ws_bytes(1, 1, 1) < 12.5e6       # about 12.2 MB of maps per image
    assert L.dc_fid_features(None, 1, None, 1, 8, 8, None, None, None, None) == -1
    assert L.dc_fid_accumulate(None, 1, None, None) == -1


def test_compute_on_merged_state_and_too_few_samples():
    from diffcodec_amd import metrics as M
    a, b = _rows(72, seed=9)
    m = M.FrechetInceptionDistance()
    with pytest.raises(RuntimeError, match="More than one sample is required"):
        m.compute()
    m.merge_state(_state(a[:30]), _state(b[:50]))
    m.merge_state(_state(a[30:]), _state(b[50:]))
    real, fake = m.state()
    assert real[0].item() == 72 and fake[0].item() == 72 and real.dtype == torch.float64 and real.shape == (M.FID_STATE,)
    v, want = m.compute(), R.fid(a, b)
    assert isinstance(v, float) and want > 1e-4 and abs(v - want) <= 1e-9 * want, (v, want)
    m.reset()
    assert not m.state()[0].any() and not m.state()[1].any()
    # a set against itself is 0, also where the covariances are rank-deficient (8 and 2 rows of 64 features) and the product
    # cov_r cov_f has zero eigenvalues, and the value of such sets still agrees with the eigenvalue form
    for n in (8, 2):
        m.merge_state(_state(a[:n]), _state(a[:n]))
        assert abs(m.compute()) < 1e-9, n
        m.reset()
    m.merge_state(_state(a[:8]), _state(b[:8]))
    v, want = m.compute(), R.fid(a[:8], b[:8])
    assert want > 1e-4 and abs(v - want) <= 1e-6 * want, (v, want)
    m.reset()
    m.merge_state(_state(a), _state(b[:1]))                              # one sample on the fake side
    with pytest.raises(RuntimeError, match="More than one sample is required"):
        m.compute()
    with pytest.raises(ValueError, match="4161"):
        m.merge_state(torch.zeros(10), torch.zeros(10))
    assert M.summarize({1: dict(psnr=30.0, ms_ssim=0.9)}, fid=1.5)["fid"] == 1.5
    assert "fid" not in M.summarize({1: dict(psnr=30.0, ms_ssim=0.9)})
