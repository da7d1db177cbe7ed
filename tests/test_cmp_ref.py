"""CPU: the fp64 restatement tests/cmp_ref.py against tests/golden/cmp_flow.npz (what the reference's own CMP module,
Fuser.convert_flow and CMP.eval upsample computed, tools/make_cmp_goldens.py), at 1e-12 of each endpoint's peak: fp64 against
fp64, the FVD restatement's bar.  Then the host side of diffcodec_amd.flow_propagation: state-dict handling, refused
architectures, the size rules, the grid points and PropagatedFlowSource with a stub model."""
import os

import numpy as np
import pytest
import torch

import cmp_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cmp_flow.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module", params=["skip", "plain"])
def run(request, golden):
    arch = request.param
    n, h, w, seed = (int(v) for v in golden[f"{arch}_case"])
    assert int(golden["weight_seed"]) == R.WEIGHT_SEED
    sd = R.synth_weights(arch)
    u8, sparse = R.inputs(n, h, w, seed)
    with torch.no_grad():
        return arch, R.endpoints(R.normalise(u8), sparse, sd, arch)


def test_restatement_matches_the_reference(run, golden):
    arch, ep = run
    for name in R.ENDPOINTS[arch]:
        want = torch.from_numpy(golden[f"{arch}_{name}"])
        got = R.subsample(ep[name])
        assert got.shape == want.shape, name
        peak = float(golden[f"{arch}_{name}_peak"])
        assert float((got - want).abs().max()) <= 1e-12 * peak, name
        # the reference's own fp32 run is as far from it as the golden says, and no further
        f32 = torch.from_numpy(golden[f"{arch}_{name}_f32"]).double()
        assert float((f32 - got).abs().max()) <= float(golden[f"{arch}_{name}_err32"]) + 1e-12 * peak, name


def test_golden_is_a_condition_that_measures_something(run, golden):
    arch, ep = run
    lg = ep["logits"]
    pk = torch.maximum(torch.softmax(lg[:, :99], 1).max(1).values, torch.softmax(lg[:, 99:], 1).max(1).values)
    onehot = float((pk > 0.99).double().mean())
    assert abs(onehot - float(golden[f"{arch}_onehot"])) < 1e-9
    assert onehot < 0.25 and float(ep["flow"].std()) > 5.0
    assert 4.0 < float(lg.std()) < 8.0
    assert os.path.getsize(GOLDEN) < 500_000


def test_conv_counts():
    from diffcodec_amd.flow_propagation import conv_table
    assert len(R.units("skip")) == len(conv_table(R.CONFIGS["skip"])) == 74
    assert len(R.units("plain")) == len(conv_table(R.CONFIGS["plain"])) == 63
    for arch in ("skip", "plain"):                                   # two tables written apart name the same tensors
        assert sorted(u[0] for u in R.units(arch)) == sorted(t[1] for t in conv_table(R.CONFIGS[arch]))
        assert sorted(str(u[1]) for u in R.units(arch)) == sorted(str(t[2]) for t in conv_table(R.CONFIGS[arch]))


# ------------------------------------------------------------------------------------------- state dicts
@pytest.fixture(scope="module")
def plain_sd():
    return R.synth_weights("plain")


def test_state_dict_prefixes_and_wrappers(plain_sd):
    from diffcodec_amd.flow_propagation import HipCMP
    cfg = R.CONFIGS["plain"]
    a = HipCMP.from_state_dict(plain_sd, cfg, device="cpu")
    b = HipCMP.from_state_dict({"module." + k: v for k, v in plain_sd.items()}, cfg, device="cpu")
    c = HipCMP.from_state_dict({"state_dict": {"module.module." + k: v for k, v in plain_sd.items()}, "step": 7}, cfg, device="cpu")
    d = HipCMP.from_state_dict({k: v for k, v in plain_sd.items() if not k.endswith("num_batches_tracked")}, cfg, device="cpu")
    assert len(a.packed) == 63
    for other in (b, c, d):
        assert all(torch.equal(a.packed[k], other.packed[k]) for k in a.packed)


def test_fold_is_the_restatements(plain_sd):
    from diffcodec_amd.flow_propagation import HipCMP
    m = HipCMP.from_state_dict(plain_sd, R.CONFIGS["plain"], device="cpu")
    for name, ck, bk in (("stem", "image_encoder.conv1", "image_encoder.bn1"), ("conv5", "image_encoder.conv5", None),
                         ("sparse1", "flow_encoder.features.0", "flow_encoder.features.1"),
                         ("decoder2.1", "flow_decoder.decoder2.4", "flow_decoder.decoder2.5"), ("head", "flow_decoder.head", None)):
        w, s, t = R.fold(plain_sd, ck, bk)
        co, K = w.shape[0], w[0].numel()
        rows, cop = (K + 31) // 32 * 32, (co + 31) // 32 * 32
        p = m.packed[name]
        assert p.shape == (rows + 2, cop) and p.dtype == torch.float32
        assert torch.equal(p[:K, :co], w.reshape(co, K).t().float())
        assert not p[K:rows].any() and not p[:, co:].any()           # zero rows, zero columns
        assert torch.equal(p[rows, :co], s.float()) and torch.equal(p[rows + 1, :co], t.float())


def test_missing_and_misshaped_keys_are_named(plain_sd):
    from diffcodec_amd.flow_propagation import HipCMP
    cfg = R.CONFIGS["plain"]
    for key in ("image_encoder.layer3.2.bn2.running_var", "flow_decoder.head.bias", "flow_encoder.features.4.weight"):
        sd = {k: v for k, v in plain_sd.items() if k != key}
        with pytest.raises(KeyError, match=key.replace(".", r"\.")):
            HipCMP.from_state_dict(sd, cfg, device="cpu")
    sd = dict(plain_sd)
    sd["image_encoder.layer2.0.conv2.weight"] = torch.zeros(128, 128, 1, 1)
    with pytest.raises(ValueError, match=r"image_encoder\.layer2\.0\.conv2\.weight"):
        HipCMP.from_state_dict(sd, cfg, device="cpu")
    sd = dict(plain_sd)
    sd["image_encoder.bn1.bias"] = torch.zeros(63)
    with pytest.raises(ValueError, match=r"image_encoder\.bn1\.bias"):
        HipCMP.from_state_dict(sd, cfg, device="cpu")
    with pytest.raises(KeyError):                                    # the other decoder's checkpoint
        HipCMP.from_state_dict(plain_sd, R.CONFIGS["skip"], device="cpu")


@pytest.mark.parametrize("field,value", [("image_encoder", "alexnet_fcn_32x"), ("image_encoder", "alexnet_fcn_8x"),
                                         ("image_encoder", "resnet101"), ("sparse_encoder", "shallownet32x"),
                                         ("flow_decoder", "MotionDecoderFlowNet")])
def test_refused_architectures_are_named(field, value):
    from diffcodec_amd.flow_propagation import conv_table
    cfg = dict(R.CONFIGS["skip"], **{field: value})
    with pytest.raises(NotImplementedError, match=value):
        conv_table(cfg)


def test_size_rules():
    from diffcodec_amd.flow_propagation import stage_sizes
    skip, plain = R.CONFIGS["skip"], R.CONFIGS["plain"]
    assert stage_sizes(skip, 64, 88) == ((32, 44), (16, 22), (8, 11))
    assert stage_sizes(skip, 72, 64) == ((36, 32), (18, 16), (9, 8))
    assert stage_sizes(skip, 512, 512)[2] == (64, 64)
    for h in (68, 56):
        with pytest.raises(ValueError):
            stage_sizes(skip, h, 64)
        with pytest.raises(ValueError):
            stage_sizes(skip, 64, h)
    assert stage_sizes(plain, 56, 32)[2] == (7, 4)                   # Plain pools by 4 at the most
    with pytest.raises(ValueError):
        stage_sizes(plain, 24, 64)
    with pytest.raises(ValueError):
        stage_sizes(plain, 68, 64)
    # the rule is the restatement's own failure: where the encoders disagree its torch.cat raises
    sd = R.synth_weights("plain")
    u8, sparse = R.inputs(1, 68, 64, 1)
    with pytest.raises(ValueError, match="disagree"), torch.no_grad():
        R.endpoints(R.normalise(u8), sparse, sd, "plain")


# ------------------------------------------------------------------------------------------- grid points
def flow_sampler_grid(h, w, stride):
    """the 'grid' branch of the reference's flow_sampler, restated with numpy as it is written there"""
    start_h = int((h - h // stride * stride) / 2)
    start_w = int((w - w // stride * stride) / 2)
    mesh = np.meshgrid(np.arange(start_h, h, stride), np.arange(start_w, w, stride))
    return sorted(zip(mesh[0].flat, mesh[1].flat))


@pytest.mark.parametrize("h,w,stride", [(64, 88, 8), (64, 88, 10), (65, 91, 8), (9, 11, 16), (9, 11, 1), (512, 512, 32), (37, 20, 7)])
def test_grid_points(h, w, stride):
    from diffcodec_amd.flow_propagation import grid_points
    want = flow_sampler_grid(h, w, stride)
    for pts in (grid_points(h, w, stride), R.grid_points(h, w, stride)):
        assert sorted((y, x) for y in pts[0] for x in pts[1]) == want
    g = torch.Generator().manual_seed(h)
    flow = torch.randn(1, 2, h, w, generator=g, dtype=torch.float64)
    sp = R.sparse_grid(flow, stride)
    ys, xs = zip(*want)
    assert int(sp[0, 2].sum()) == len(want) and torch.equal(sp[0, 2], sp[0, 3])
    assert torch.equal(sp[0, :2, list(ys), list(xs)], flow[0, :, list(ys), list(xs)])
    assert int((sp[0, :2] != 0).sum()) <= 2 * len(want)               # nothing off the grid


def test_sparse_from_points():
    from diffcodec_amd.flow_propagation import sparse_from_points
    sp = sparse_from_points([[1, 2], [3, 0]], [[1.5, -2.0], [0.25, 4.0]], 4, 5, device="cpu")
    assert sp.shape == (1, 4, 4, 5) and float(sp[0, 2].sum()) == 2
    assert sp[0, :, 1, 2].tolist() == [1.5, -2.0, 1.0, 1.0] and sp[0, :, 3, 0].tolist() == [0.25, 4.0, 1.0, 1.0]
    with pytest.raises(ValueError, match="distinct"):
        sparse_from_points([[1, 2], [1, 2]], [[0, 0], [1, 1]], 4, 5, device="cpu")
    with pytest.raises(ValueError, match="outside"):
        sparse_from_points([[4, 0]], [[0, 0]], 4, 5, device="cpu")


# ------------------------------------------------------------------------------------------- clip source
class StubSource:
    with_warp = True

    def controls(self, frame, prev, nxt):
        g = torch.Generator().manual_seed(frame)
        return torch.rand(1, 6, 16, 24, generator=g), torch.randn(1, 4, 16, 24, generator=g)

    def ground_truth(self, frame):
        return torch.full((16, 24, 3), frame, dtype=torch.uint8)

    def warp(self, frame):
        return torch.full((1, 3, 16, 24), float(frame))


class StubModel:
    """flow() = per sample (mean of the image, sum of the sparse flow channel 0): tells which anchor met which flow half"""

    def flow(self, image, sparse):
        self.seen = (image, sparse)
        n, h, w = image.shape[0], image.shape[1], image.shape[2]
        a = image.float().mean(dim=(1, 2, 3)).view(n, 1, 1, 1).expand(n, 1, h, w)
        b = sparse[:, 0].sum(dim=(1, 2)).view(n, 1, 1, 1).expand(n, 1, h, w)
        return torch.cat([a, b], 1)


def test_propagated_flow_source_pairs_anchors_and_flows(monkeypatch):
    from diffcodec_amd import flow_propagation as FP
    monkeypatch.setattr(FP, "sample_grid", lambda flow, stride: R.sparse_grid(flow.double(), stride).float())
    inner, model = StubSource(), StubModel()
    src = FP.PropagatedFlowSource(inner, model, stride=8)
    cond, flow = src.controls(5, 0, 8)
    cond0, flow0 = inner.controls(5, 0, 8)
    assert torch.equal(cond, cond0) and flow.shape == (1, 4, 16, 24)
    q = (cond0 * 255).round().clamp(0, 255).to(torch.uint8)
    image, sparse = model.seen
    assert image.dtype == torch.uint8 and image.shape == (2, 16, 24, 3) and sparse.shape == (2, 4, 16, 24)
    assert torch.equal(image[0], q[0, :3].permute(1, 2, 0)) and torch.equal(image[1], q[0, 3:].permute(1, 2, 0))
    fwd, bwd = R.sparse_grid(flow0[:, :2].double(), 8).float(), R.sparse_grid(flow0[:, 2:].double(), 8).float()
    assert torch.equal(sparse[0], fwd[0]) and torch.equal(sparse[1], bwd[0])
    # flow[:, :2] came from (previous anchor, forward samples), flow[:, 2:] from (next anchor, backward samples)
    assert torch.allclose(flow[0, 0], q[0, :3].float().mean().expand(16, 24)) and torch.allclose(flow[0, 1], fwd[0, 0].sum().expand(16, 24))
    assert torch.allclose(flow[0, 2], q[0, 3:].float().mean().expand(16, 24)) and torch.allclose(flow[0, 3], bwd[0, 0].sum().expand(16, 24))
    assert src.with_warp is True and torch.equal(src.warp(5), inner.warp(5)) and torch.equal(src.ground_truth(5), inner.ground_truth(5))
    with pytest.raises(AttributeError):
        src.noise
