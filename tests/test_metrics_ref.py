"""CPU: the fp64 restatement of PSNR / SSIM / MS-SSIM (tests/metrics_ref.py) is pinned to independent evaluations, and
diffcodec_amd.metrics refuses what pytorch_msssim refuses before it touches a device.  On the edge tables of tests/edge_cases.py the
bound of the GPU edge tests (R.ssim_bound through R.expected / R.check_out) passes an fp32 restatement of csrc/metrics.hip and
rejects structural faults planted in it; no faulty kernel is ever run on a device."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import edge_cases as E
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


# ------------------------------------------------------------------------------------------ the edge tables and their bound
def case_reference(c, seed):
    """(X, Y logical NCHW on the CPU, fp32 taps, expected) of a MetricCase, as tests/test_gpu_metrics.py forms them"""
    X, Y = E.metric_inputs(c, seed)
    g = E.metric_window(c.ws)
    return X, Y, g, R.case_expected(c, X, Y, g)


def _filter_f32(a, g, drop_last_tap=False):
    """the kernel's separable window in fp32: along W first, then along H, taps in index order"""
    ws = g.numel()
    taps = [float(v) for v in g]
    if drop_last_tap:
        taps[-1] = 0.0
    wo, ho = a.shape[-1] - ws + 1, a.shape[-2] - ws + 1
    h = torch.zeros(a.shape[:-1] + (wo,), dtype=torch.float32)
    for j in range(ws):
        h = h + np.float32(taps[j]) * a[..., j:j + wo]
    v = torch.zeros(a.shape[:-2] + (ho, wo), dtype=torch.float32)
    for j in range(ws):
        v = v + np.float32(taps[j]) * h[..., j:j + ho, :]
    return v


def _pool_f32(x, fault=None):
    """the kernel's pool: zero pad on the low side of an odd axis, ((a + b) + (c + d)) / 4 in fp32"""
    ph, pw = x.shape[-2] % 2, x.shape[-1] % 2
    ones = torch.ones_like(x)
    if fault == "pool_high":
        x, ones = F.pad(x, (0, pw, 0, ph)), F.pad(ones, (0, pw, 0, ph))
    else:
        x, ones = F.pad(x, (pw, 0, ph, 0)), F.pad(ones, (pw, 0, ph, 0))
    q = lambda t: (t[..., 0::2, 0::2] + t[..., 0::2, 1::2]) + (t[..., 1::2, 0::2] + t[..., 1::2, 1::2])
    return q(x) / q(ones) if fault == "pool_count" else q(x) * np.float32(0.25)


FAULTS = ("tap", "column", "area", "pool_high", "pool_count", "norelu", "cs_last", "weights_rev", "y_strides", "c2_k1")


def restate_f32(c, X, Y, g, fault=None):
    """csrc/metrics.hip restated with torch in fp32 (values shifted by L / 2, horizontal pass first, fp64 sums of the fp32 maps,
    the finalize in fp64) -> fp64 [N*C + N + 1]; `fault` plants one structural error."""
    assert fault is None or fault in FAULTS
    f32 = np.float32
    if fault == "y_strides":                                   # Y's storage read through X's strides
        _, lx, ly = E.METRIC_FORMS[c.form]
        gx, sx = E.metric_operand(X, lx, "cpu")
        gy, _ = E.metric_operand(Y, ly, "cpu")
        Y = E.metric_read(gy, tuple(Y.shape), sx).clone()
    shift = f32(0.5) * f32(c.L)
    k1, k2 = (float(f32(k)) for k in c.K)
    c1 = f32((k1 * float(f32(c.L))) ** 2)
    c2 = f32(((k1 if fault == "c2_k1" else k2) * float(f32(c.L))) ** 2)
    x, y = X.float(), Y.float()
    levels = c.levels or 1
    means = []
    for s in range(levels):
        if s:
            x, y = _pool_f32(x, fault), _pool_f32(y, fault)
        a, b = x - shift, y - shift
        drop = fault == "tap"
        mx, my = _filter_f32(a, g, drop), _filter_f32(b, g, drop)
        sxx = _filter_f32(a * a, g, drop) - mx * mx
        syy = _filter_f32(b * b, g, drop) - my * my
        sxy = _filter_f32(a * b, g, drop) - mx * my
        ux, uy = mx + shift, my + shift
        cs = (f32(2) * sxy + c2) / ((sxx + syy) + c2)
        lum = (f32(2) * (ux * uy) + c1) / ((ux * ux + uy * uy) + c1)
        sm = lum * cs
        ho, wo = cs.shape[-2:]
        area = (ho + 1) * wo if fault == "area" else ho * wo
        if fault == "column":
            sm, cs = sm[..., :-1], cs[..., :-1]
        means.append((sm.double().flatten(2).sum(-1) / area, cs.double().flatten(2).sum(-1) / area))
    relu = (lambda t: t) if fault == "norelu" else (lambda t: torch.where(t < 0, torch.zeros_like(t), t))
    if c.levels:
        w = [float(f32(v)) for v in c.weights]
        if fault == "weights_rev":
            w = w[::-1]
        v = torch.ones_like(means[0][0])
        for s in range(levels):
            base = means[s][1] if (s < levels - 1 or fault == "cs_last") else means[s][0]
            v = v * relu(base) ** w[s]
    else:
        v = means[0][0]
        if c.nonneg:
            v = relu(v)
    return torch.cat([v.reshape(-1), v.sum(1) / v.shape[1], (v.sum() / v.numel()).reshape(1)])


METRIC_TABLES = {"ssim": E.SSIM_CASES, "ms_ssim": E.MS_SSIM_CASES}
_ALL = [(t, i) for t in METRIC_TABLES for i in range(len(METRIC_TABLES[t]))]


@pytest.fixture(scope="module")
def references():
    return {(t, i): case_reference(METRIC_TABLES[t][i], i) for t, i in _ALL}


# fault -> the cases (table, label) on which it must be rejected
REJECTED_ON = {
    "tap": [("ssim", "3x2x35x67-ws3-pitched-noisy-L255-Kwide"), ("ssim", "3x2x43x75-ws11-f32_nchw-noisy-L255"),
            ("ssim", "2x1x1x1-ws1-u8_nhwc-noisy-L255"), ("ms_ssim", "2x3x161x161-ws11-lv5-mixed-noisy-L255")],
    "column": [("ssim", "3x2x47x79-ws15-mixed-noisy-L255"), ("ssim", "1x2x42x74-ws11-u8_nhwc-noisy-L255"),
               ("ssim", "3x2x33x65-ws1-u8_nchw-noisy-L255"), ("ms_ssim", "3x2x33x35-ws3-lv5-u8_nhwc-noisy-L255")],
    "area": [("ssim", "1x1x18x30-ws11-f32_nchw-noisy-L1"), ("ssim", "257x1x3x3-ws3-u8_nhwc-noisy-L255"),
             ("ssim", "1x1x1x16385-ws1-f32_nchw-noisy-L255"), ("ms_ssim", "1x3x47x90-ws7-lv1-f32_view-noisy-L255")],
    "pool_high": [("ms_ssim", "2x2x23x24-ws5-lv2-u8_nhwc-noisy-L255"), ("ms_ssim", "2x2x24x23-ws5-lv2-mixed-noisy-L1-Kwide"),
                  ("ms_ssim", "2x2x23x23-ws5-lv2-mixed-noisy-L1-Kwide"), ("ms_ssim", "3x2x33x35-ws3-lv5-f32_view-noisy-L1-Kwide")],
    "pool_count": [("ms_ssim", "2x2x23x23-ws5-lv2-u8_nhwc-noisy-L255"), ("ms_ssim", "2x2x24x23-ws5-lv2-u8_nhwc-noisy-L255"),
                   ("ms_ssim", "2x2x23x24-ws5-lv2-mixed-noisy-L1-Kwide"), ("ms_ssim", "2x1x129x2-ws1-lv8-u8_nhwc-noisy-L255")],
    "norelu": [("ssim", "2x3x21x70-ws7-f32_nchw-anti-L1-Kwide-nonneg"), ("ssim", "2x2x5x5-ws5-u8_nchw-anti-L255-nonneg"),
               ("ms_ssim", "3x2x33x35-ws3-lv5-f32_nchw-anti-L1")],
    "cs_last": [("ms_ssim", "3x2x33x35-ws3-lv5-u8_nhwc-extremes-L255"), ("ms_ssim", "1x3x47x90-ws7-lv1-f32_view-noisy-L255"),
                ("ms_ssim", "2x2x24x24-ws5-lv2-u8_nhwc-noisy-L255")],
    "weights_rev": [("ms_ssim", "3x2x33x35-ws3-lv5-u8_nhwc-noisy-L255"), ("ms_ssim", "1x1x45x77-ws5-lv3-pitched-noisy-L255"),
                    ("ms_ssim", "2x2x24x24-ws5-lv2-mixed-noisy-L1-Kwide")],
    "y_strides": [("ssim", "2x4x13x20-ws11-mixed-noisy-L255"), ("ssim", "1x2x42x74-ws11-mixed-noisy-L1-Kwide"),
                  ("ms_ssim", "2x3x161x161-ws11-lv5-mixed-noisy-L255"), ("ms_ssim", "2x2x23x24-ws5-lv2-mixed-noisy-L1-Kwide")],
    "c2_k1": [("ssim", "3x2x35x67-ws3-mixed-noisy-L255"), ("ssim", "3x2x37x69-ws5-u8_nhwc-noisy-L255"),
              ("ms_ssim", "3x2x33x35-ws3-lv5-u8_nhwc-noisy-L255")],
}


@pytest.mark.parametrize("t,i", _ALL, ids=[f"{t}-{METRIC_TABLES[t][i].label()}" for t, i in _ALL])
def test_ssim_bound_passes_the_fp32_restatement(references, t, i):
    """the check the GPU edge tests apply (R.expected + R.check_out) on this case's own inputs: an fp32 restatement of the kernel
    passes, far inside the bound (a worst case: anything near 1 means the derivation is wrong)"""
    c = METRIC_TABLES[t][i]
    X, Y, g, exp = references[(t, i)]
    v = R.check_out(restate_f32(c, X, Y, g), exp)
    assert v["ok"] and v["ratio"] <= 0.25, (c.label(), v)


@pytest.mark.parametrize("fault", FAULTS)
def test_ssim_bound_rejects_faults(references, fault):
    """each structural fault, planted in the restatement, fails the same check on every case named for it"""
    assert set(REJECTED_ON) == set(FAULTS)
    index = {(t, METRIC_TABLES[t][i].label()): (t, i) for t, i in _ALL}
    for name in REJECTED_ON[fault]:
        assert name in index, f"{name}: no such case"
        t, i = index[name]
        c = METRIC_TABLES[t][i]
        X, Y, g, exp = references[(t, i)]
        v = R.check_out(restate_f32(c, X, Y, g, fault), exp)
        assert not v["ok"], (fault, name, v)


def test_ms_ssim_table_keeps_its_bases_off_the_clamp(references):
    """a condition of the tables: every clamped base of a case that is neither `anti` nor `nan` stays at least 16 bounds above 0
    at every scale (so the first-order MS-SSIM bound holds and no clamp can flip), and every `anti` case whose answer is exactly 0
    has a clamped mean at least 16 bounds below 0 at some scale (so 0.0 is the only right answer)"""
    for (t, i), (X, Y, g, exp) in references.items():
        c = METRIC_TABLES[t][i]
        clamped = bool(c.levels) or c.nonneg
        if c.family == "nan" or not clamped:
            continue
        if c.family == "anti":
            assert c.exact == 0.0
            assert bool(((exp["base"] < -16 * exp["delta"]).any(0)).all()), c.label()
        else:
            assert bool((exp["base"] >= 16 * exp["delta"]).all()), (c.label(), exp["base"].min().item(), exp["delta"].max().item())
    for c in E.SSIM_CASES:
        if c.family == "anti" and not c.nonneg:                 # plain SSIM of the anti family: a negative value, held by the bound
            X, Y, g, exp = references[("ssim", E.SSIM_CASES.index(c))]
            assert bool((exp["v"] < -16 * exp["d"]).all()), c.label()


def test_nan_reference_marks_one_plane_and_its_sample():
    for t, cases in METRIC_TABLES.items():
        for i, c in enumerate(cases):
            if c.family != "nan":
                continue
            _, _, _, exp = case_reference(c, i)
            n0, c0 = E.nan_position(c)[:2]
            want = torch.zeros(c.n, c.c, dtype=torch.bool)
            want[n0, c0] = True
            assert torch.equal(torch.isnan(exp["v"]), want), c.label()
            out = restate_f32(c, *case_reference(c, i)[:3])
            assert R.check_out(out, exp)["ok"]
            zeroed = torch.nan_to_num(out, nan=0.0)                      # what fmax(v, 0) made of it
            assert not R.check_out(zeroed, exp)["ok"], c.label()


def test_psnr_reference_on_the_table():
    """R.psnr on the PSNR table: +inf for identical, the closed form for `extremes` and `onepixel`"""
    for i, c in enumerate(E.PSNR_CASES):
        X, Y = E.metric_inputs(c, i)
        p = R.psnr(X.double(), Y.double(), c.L)
        if c.family == "identical":
            assert torch.isinf(p).all()
        elif c.family == "extremes":
            assert p.abs().max().item() < 1e-12
        elif c.family == "onepixel":
            want = 10 * np.log10(255.0 ** 2 * (c.c * c.h * c.w))
            assert (p - want).abs().max().item() < 1e-5
