"""CPU: the fp64 restatement tests/fvd_ref.py against tests/golden/fvd_i3d.npz (what the reference's pytorch_i3d.py and fvd.py compute
with the same seeded weights; tools/make_fvd_goldens.py), and the host side of metrics.FrechetVideoDistance.

Measured when the golden was made: restatement against reference 2e-16 .. 2.5e-15 per endpoint and 4e-16 on the logits (both
fp64; the bar here is 1e-12), preprocess 1.3e-14 against the reference's fp64 run.  Frechet values: 450 rows 3.1e-15, two identical
rows per side 1.3e-16, 16 rows (rank-deficient) 7.0e-8, where the reference's sqrtm is itself 6.3e-8 off."""
import os
import sys

import numpy as np
import pytest
import torch

import fvd_ref as R

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import make_fvd_goldens as G  # noqa: E402  (the seeded inputs; its reference import happens only in main())

from diffcodec_amd import metrics  # noqa: E402

BAR = 1e-12


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "fvd_i3d.npz"))


@pytest.fixture(scope="module")
def sd(gold):
    return R.synth_weights(int(gold["weight_seed"]))


def _rel(a, b):
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("t", [10, 11])
def test_endpoints_and_logits_match_the_reference(gold, sd, t, record):
    """T = 10 and T = 11 take both branches of the SAME rule on the time axis"""
    with torch.no_grad():
        x = G.net_input(t, int(gold[f"t{t}_input_seed"]))
        eps = R.endpoints(x, sd)
        logits = R.head(eps[-1], sd)
    assert [tuple(e.shape[1:]) for e in eps] == metrics.fvd_endpoint_shapes(t)
    for e, (name, m) in enumerate(zip(metrics.FVD_ENDPOINTS, eps)):
        err = _rel(G.subsample(m), gold[f"t{t}_ep{e:02d}"])
        record(f"fvd_ref_t{t}_{name}", err)
        assert err <= BAR, (name, err)
        assert float((m != 0).double().mean()) >= 0.2, name               # a dead net would pass everything
    err = _rel(logits, gold[f"t{t}_logits"])
    record(f"fvd_ref_t{t}_logits", err)
    assert logits.shape == (1, 400) and err <= BAR and float(logits.std()) > 1


@pytest.mark.parametrize("name,h,w", [("wide", 40, 56), ("tall", 96, 64)])
def test_preprocess_matches_the_reference(gold, name, h, w, record):
    v = G.source_video(h, w, int(gold[f"prep_{name}_seed"]))
    mine = R.preprocess(v)[0]
    assert mine.shape == (3, 2, 224, 224)
    e64 = float((G.subsample(mine, 8000) - torch.from_numpy(gold[f"prep_{name}_f64"])).abs().max())
    e32 = float((G.subsample(mine, 8000) - torch.from_numpy(gold[f"prep_{name}_f32"]).double()).abs().max())
    record(f"fvd_ref_prep_{name}_vs_f64", e64)
    record(f"fvd_ref_prep_{name}_vs_f32", e32)
    assert e64 <= BAR
    assert e32 <= 1e-4                                                    # torch forms the source position in fp32: 1.3e-5 measured
    assert metrics.fvd_resized_size(h, w) == ((224, 314) if name == "wide" else (336, 224))


@pytest.mark.parametrize("name,bar", [("rows450", 1e-9), ("rows2", 1e-12), ("rows16", 1e-6)])
def test_frechet_value_matches_the_reference(gold, name, bar, record):
    fake, real = G.row_sets()[name]
    want = float(gold[f"frechet_{name}"])
    got = R.frechet(fake, real)
    record(f"fvd_ref_frechet_{name}", abs(got - want) / abs(want))
    assert abs(got - want) <= bar * abs(want), (got, want)
    if name == "rows2":                                                   # two identical rows per side: cov = 0, the value is |df|^2
        assert abs(got - float(((fake[0] - real[0]) ** 2).sum())) <= 1e-12 * got
    # the class forms the same statistics from rows added in pieces
    m = metrics.FrechetVideoDistance()
    m.update_features(fake[:1].float(), real=False)
    m.update_features(fake[1:].float(), real=False)
    m.update_features(real.float(), real=True)
    assert m.count(True) == real.shape[0] and m.count(False) == fake.shape[0]
    assert m.compute() == R.frechet(fake.float(), real.float())
    m.reset()
    assert m.count(True) == 0


def test_fid_value_keeps_its_bits():
    """the factored Frechet core is the arithmetic frechet_distance had"""
    g = torch.Generator().manual_seed(3)
    states = []
    for n in (5, 70):
        f = torch.randn(n, 64, generator=g, dtype=torch.float64)
        states.append(torch.cat([torch.tensor([float(n)], dtype=torch.float64), f.sum(0), (f.t() @ f).reshape(-1)]))
    stats = []
    for st in states:
        n = float(st[0])
        mu = st[1:65] / n
        stats.append((mu, (st[65:].view(64, 64) - n * torch.outer(mu, mu)) / (n - 1)))
    (mu_r, cov_r), (mu_f, cov_f) = stats
    d = mu_r - mu_f
    (a_r, u_r), (a_f, u_f) = torch.linalg.eigh(cov_r), torch.linalg.eigh(cov_f)
    c = torch.linalg.svdvals((u_r * a_r.clamp_min(0).sqrt()).t() @ (u_f * a_f.clamp_min(0).sqrt())).sum()
    assert metrics.frechet_distance(states[0], states[1]) == float((d * d).sum() + cov_r.trace() + cov_f.trace() - 2 * c)


def test_tables_and_packing():
    units = metrics.fvd_units()
    assert len(units) == 57 and units[0] == ("Conv3d_1a_7x7", 3, 64, 7, 2) and units[-1] == ("Mixed_5c.b3b", 832, 128, 1, 1)
    assert len(metrics.FVD_ENDPOINTS) == 16
    assert [metrics.fvd_same_pad(*a) for a in ((10, 7, 2), (11, 7, 2), (7, 3, 1), (5, 2, 2), (6, 2, 2), (7, 1, 1))] == \
        [(5, 2, 3), (6, 3, 3), (7, 1, 1), (3, 0, 1), (3, 0, 0), (7, 0, 0)]
    # one unit of each kernel class: rows in (ci, kt, kh, kw) order with the class's zero rows, zero columns past Cout
    g = torch.Generator().manual_seed(0)
    w7 = torch.randn(5, 2, 7, 7, 7, generator=g)
    p = metrics.pack_fvd_unit(w7, torch.ones(5), torch.zeros(5)).view(-1, 32)
    assert p.shape[0] == 2 * 7 * 50 + 2 and not p[:, 5:].any() and not p[49::50][:14].any()
    assert torch.equal(p[50 * (1 * 7 + 3) + 7 * 2 + 4, :5], w7[:, 1, 3, 2, 4])
    w3 = torch.randn(33, 6, 3, 3, 3, generator=g)
    p = metrics.pack_fvd_unit(w3, torch.arange(33.), -torch.arange(33.)).view(-1, 64)
    assert p.shape[0] == 2 * 108 + 2 and torch.equal(p[27 * 5 + 9 * 2 + 3 * 1 + 0, :33], w3[:, 5, 2, 1, 0]) and not p[162:216].any()
    assert torch.equal(p[216, :33], torch.arange(33.)) and torch.equal(p[217, :33], -torch.arange(33.)) and not p[216:, 33:].any()
    w1 = torch.randn(16, 40, 1, 1, 1, generator=g)
    p = metrics.pack_fvd_unit(w1, torch.ones(16), torch.ones(16)).view(-1, 32)
    assert p.shape[0] == 64 + 2 and torch.equal(p[:40, :16], w1.view(16, 40).t()) and not p[40:64].any()
    with pytest.raises(ValueError, match="1x1x1, 3x3x3 or 7x7x7"):
        metrics.pack_fvd_unit(torch.zeros(4, 4, 5, 5, 5), torch.ones(4), torch.ones(4))


def test_state_dict_keys_shapes_and_bn_eps(sd):
    packed = metrics.pack_fvd_weights(sd)
    from diffcodec_amd import lib
    assert packed.numel() == lib.load().dc_fvd_weight_floats() and packed.dtype == torch.float32
    extra = dict(sd)
    extra["Mixed_9z.unknown.weight"] = torch.zeros(3)
    assert torch.equal(metrics.pack_fvd_weights(extra), packed)           # unknown keys and num_batches_tracked are ignored
    m = metrics.FrechetVideoDistance.from_state_dict(sd)
    assert torch.equal(m.packed, packed) and m.bn_eps == 1e-5 and m.byte_range is False
    missing = {k: v for k, v in sd.items() if k != "Mixed_4e.b2b.bn.running_var"}
    with pytest.raises(ValueError, match="missing key 'Mixed_4e.b2b.bn.running_var'"):
        metrics.pack_fvd_weights(missing)
    bad = dict(sd)
    bad["logits.conv3d.weight"] = torch.zeros(400, 1024)
    with pytest.raises(ValueError, match="logits.conv3d.weight.*expected"):
        metrics.pack_fvd_weights(bad)
    # bn_eps is folded at pack time: s = g / sqrt(v + eps), t = b - m s of the first unit (rows 1050 and 1051 of its [.., 64] matrix)
    for eps in (1e-5, 1e-3):
        first = metrics.pack_fvd_weights(sd, eps)[:1052 * 64].view(1052, 64)
        g, b, mu, v = (sd[f"Conv3d_1a_7x7.bn.{q}"].double() for q in ("weight", "bias", "running_mean", "running_var"))
        s = g / torch.sqrt(v + eps)
        assert torch.equal(first[1050], s.float()) and torch.equal(first[1051], (b - mu * s).float())
    assert not torch.equal(metrics.FrechetVideoDistance.from_state_dict(sd, bn_eps=1e-3).packed, packed)


def test_operand_checks_need_no_gpu(sd):
    m = metrics.FrechetVideoDistance()
    with pytest.raises(RuntimeError, match="no weights"):
        m._weights(torch.device("cpu"))
    with pytest.raises(ValueError, match="at least 9 frames"):
        m.features(torch.zeros(1, 8, 32, 32, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="5-d"):
        m.features(torch.zeros(9, 32, 32, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="3-channel"):
        m.features(torch.zeros(1, 9, 1, 32, 32))
    with pytest.raises(ValueError, match="uint8 .* or floating"):
        m.features(torch.zeros(1, 9, 3, 32, 32, dtype=torch.int32))
    with pytest.raises(ValueError, match=r"\[N,400\]"):
        m.update_features(torch.zeros(2, 64), real=True)
    m.update_features(torch.zeros(2, 400), real=True)
    m.update_features(torch.zeros(1, 400), real=False)
    with pytest.raises(RuntimeError, match="More than one sample is required for both the real and fake distributed to compute FID"):
        m.compute()
    with pytest.raises(ValueError, match="at most 4096 frames"):
        m._chunks(1, 5000, 32, 32)
    with pytest.raises(ValueError, match="same shape"):
        metrics.calculate_fvd(torch.zeros(2, 9, 3, 8, 8), torch.zeros(2, 9, 3, 8, 9), m)
    assert metrics.summarize({1: dict(psnr=30.0, ms_ssim=0.9)}, fid=1.5, fvd=2.5)["fvd"] == 2.5
    assert "fvd" not in metrics.summarize({1: dict(psnr=30.0, ms_ssim=0.9)})


def test_decode_clip_refuses_fvd_without_a_whole_video():
    """gather=False with two ranks: no rank holds all the frames; raised before anything is decoded (the pipe is never touched)"""
    from diffcodec_amd import clip_decode as CD
    with pytest.raises(ValueError, match="no rank holds all its frames"):
        CD.decode_clip(None, None, 12, 11, 64, 64, None, rank=0, world=2, gather=False, score=True, fvd=metrics.FrechetVideoDistance())
