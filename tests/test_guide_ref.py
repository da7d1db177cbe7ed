"""CPU: tests/guide_ref.py (numpy / torch, no scipy) is the reference's 'watershed' sampler: against tests/golden/guide_points.npz,
recorded from the reference's own flow_sampler by tools/make_guide_goldens.py, it reproduces every final mask under the recorded
seed, every candidate mask and every edge map; where scipy imports, the candidates also equal a direct scipy computation.  The
deterministic elimination rule gives a set with no two survivors in one box and an earlier survivor in the box of everything
removed.  Then what is specific to the guide family's C surface (include/diffcodec_guide_hip.h, lib.GUIDE_SIGNATURES;
tests/test_abi.py holds the pair to its header and to the built library): its name set; the refusals return -1 before any launch;
and a census: every launcher has a literal lib.call in tests/test_gpu_guide_points.py or in diffcodec_amd/guide_points.py."""
import os

import numpy as np
import pytest
import torch

import abi_check as A
import guide_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "guide_points.npz")
QUERIES = ("dc_guide_ws_bytes",)
STAGES = {"dc_guide_edge", "dc_guide_edt", "dc_guide_nms", "dc_guide_select", "dc_guide_scatter"}


@pytest.fixture(scope="module")
def golden():
    cases = G.load_golden(GOLDEN)
    for c in cases.values():
        c["flow"] = G.to_nchw(G.synth_flow(c["params"], c["H"], c["W"]))[0]
    return cases


# ------------------------------------------------------------------------------------------------ restatement against the golden
def test_golden_is_small_and_covers_the_paths(golden):
    assert os.path.getsize(GOLDEN) < 64 * 1024
    assert {G.working_ds(c["H"], c["W"]) for c in golden.values()} == {1, 2, 4}
    assert sum(int(c["cand"].sum()) > 100 for c in golden.values()) >= 2            # plateaus of ties
    assert {c["ks"] for c in golden.values()} >= {3, 15, 41, 49, 81}


def test_restatement_reproduces_the_final_masks_under_the_recorded_seed(golden):
    for name, c in golden.items():
        np.random.seed(c["seed"])
        got = G.final_mask(c["flow"], c["ks"], c["stride"], coin=np.random.rand)
        assert np.array_equal(got, c["mask"]), name


def test_restatement_reproduces_edge_maps_and_candidates(golden):
    for name, c in golden.items():
        norm32 = G.edge_magnitude(c["flow"][None], torch.float32)
        norm64 = G.edge_magnitude(c["flow"][None], torch.float64)
        assert float((norm64 - 0.1).abs().min()) >= 1e-4, name                         # the generator's gap, seen from here
        edge = G.edge_map(norm32)[0].numpy()
        assert np.array_equal(edge, c["edge"]) and np.array_equal(G.edge_map(norm64)[0].numpy(), c["edge"]), name
        assert np.array_equal(G.candidates(G.sqdist(edge), c["ks"]), c["cand"]), name


def test_a_flow_without_an_edge_has_no_watershed_point(golden):
    constant = [c for n, c in golden.items() if n.startswith("constant")]
    assert len(constant) == 3
    for c in constant:
        assert not c["edge"].any() and not c["cand"].any()
        gy, gx = G.grid_points(c["H"], c["W"], c["stride"])
        grid = np.zeros((c["H"], c["W"]), dtype=bool)
        grid[np.ix_(gy, gx)] = True
        assert np.array_equal(c["mask"], grid)
    d2 = G.sqdist(np.zeros((5, 7), dtype=bool))
    assert (d2 == G.NO_EDGE).all() and not G.candidates(d2, 3).any()


def test_candidates_equal_a_direct_scipy_computation_where_scipy_imports(golden):
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    rng = np.random.RandomState(0)
    random_edges = [(rng.rand(h, w) < p, ks) for h, w, p, ks in ((23, 31, 0.02, 5), (40, 24, 0.01, 15), (17, 19, 0.05, 81), (9, 64, 0.03, 7))]
    for edge, ks in [(c["edge"], c["ks"]) for c in golden.values() if c["edge"].any()] + random_edges:
        d2 = G.sqdist(edge)
        rows, cols = np.nonzero(edge)                                                  # the definition, pixel by pixel on a sample
        for y, x in zip(rng.randint(0, edge.shape[0], 16), rng.randint(0, edge.shape[1], 16)):
            assert d2[y, x] == ((rows - y) ** 2 + (cols - x) ** 2).min()
        if ndimage is None:
            continue
        dist = ndimage.distance_transform_edt(1 - edge.astype(np.float32))
        assert np.array_equal(np.rint(dist * dist).astype(np.int64), d2)
        res = dist.copy()
        res[dist < ndimage.maximum_filter(dist, footprint=np.ones((ks, ks)))] = 0.0      # the 'reflect' boundary
        res[0, :] = res[-1, :] = 0.0
        res[:, 0] = res[:, -1] = 0.0
        assert np.array_equal(res > 0, G.candidates(d2, ks))


def plateau_edges(h=48, w=70):
    """two parallel edge lines 16 apart: the medial line between them is a plateau of ties"""
    e = np.zeros((h, w), dtype=bool)
    e[:, 20] = e[:, 36] = True
    return e


def test_the_deterministic_rule(golden):
    cases = [(c["cand"], c["ks"]) for c in golden.values()]
    cases += [(G.candidates(G.sqdist(plateau_edges()), ks), ks) for ks in (3, 5, 15)]
    rng = np.random.RandomState(1)
    cases += [(rng.rand(40, 56) < 0.2, ks) for ks in (3, 7, 15, 81)]
    assert int(cases[-7][0].sum()) > 40
    for cand, ks in cases:
        d = (ks - 1) / 2
        ys, xs = np.nonzero(cand)
        sy, sx = G.neighbor_elim(ys, xs, d)
        gy, gx = G.greedy(ys, xs, d)
        assert np.array_equal(sy, gy) and np.array_equal(sx, gx)                       # the pair order with its default coin is the rule
        near = (np.abs(sy[:, None] - sy[None, :]) < d) & (np.abs(sx[:, None] - sx[None, :]) < d)
        assert not (near & ~np.eye(len(sy), dtype=bool)).any()                        # no two survivors in one box
        kept = set(zip(sy.tolist(), sx.tolist()))
        order = {p: i for i, p in enumerate(zip(ys.tolist(), xs.tolist()))}
        for y, x in zip(ys.tolist(), xs.tolist()):
            if (y, x) not in kept:                                                     # an earlier survivor lies in its box
                assert any(order[s] < order[(y, x)] and abs(s[0] - y) < d and abs(s[1] - x) < d for s in kept), (y, x)
        assert len(sy) <= -(-cand.shape[0] // int(d)) * -(-cand.shape[1] // int(d))   # one per d x d tile: the device's `cap`


def test_python_surface_rules_need_no_gpu(monkeypatch):
    from diffcodec_amd import flow_propagation as FP
    from diffcodec_amd import guide_points as GP
    assert FP.sample_watershed is GP.sample_watershed and FP.watershed_points is GP.watershed_points
    assert FP.stride_from_bg_ratio(1.0 / 6400) == int(np.sqrt(1.0 / (1.0 / 6400))) and GP.stride_from_bg_ratio(1.0) == 1
    assert GP.stride_from_bg_ratio(0.008) == 11
    assert GP.working_size(1080, 1920) == (4, 270, 480) and GP.working_size(24, 801) == (2, 12, 401) and GP.working_size(512, 512) == (1, 512, 512)
    assert GP.max_points(24, 40, 81) == 1 and GP.max_points(37, 53, 3) == 37 * 53 and GP.max_points(270, 480, 15) == 39 * 69
    flow = torch.zeros(1, 2, 8, 8)
    for bad in (dict(nms_ks=14), dict(nms_ks=1), dict(max_num_guide=5), dict(stride=0)):
        with pytest.raises(ValueError):
            GP.sample_watershed(flow, **bad)
    with pytest.raises(ValueError):
        GP.watershed_points(flow.double())
    with pytest.raises(ValueError):
        GP.stride_from_bg_ratio(0.0)
    with pytest.raises(RuntimeError):
        GP.sample_watershed(flow)                                                      # no CPU path

    class Inner:
        def controls(self, frame, prev, nxt):
            return torch.zeros(1, 6, 8, 8), torch.arange(4 * 64, dtype=torch.float32).view(1, 4, 8, 8)

    class Model:
        def flow(self, image, sparse):
            self.sparse = sparse
            return sparse[:, :2]

    calls = []
    monkeypatch.setattr(FP, "sample_grid", lambda flow, stride: calls.append(("grid", stride)) or torch.cat([flow, flow], 1))
    monkeypatch.setattr(FP, "sample_watershed", lambda flow, nms_ks=15, stride=None: calls.append(("watershed", nms_ks, stride)) or torch.cat([flow, -flow], 1))
    model = Model()
    FP.PropagatedFlowSource(Inner(), model, stride=4).controls(1, 0, 2)
    assert calls == [("grid", 4)]
    _, out = FP.PropagatedFlowSource(Inner(), model, stride=4, nms_ks=15).controls(1, 0, 2)
    assert calls == [("grid", 4), ("watershed", 15, 4)] and model.sparse.shape == (2, 4, 8, 8)
    assert torch.equal(out, Inner().controls(1, 0, 2)[1])                               # forward half first, then the backward half


# ------------------------------------------------------------------------------------------------ the C surface
@pytest.fixture(scope="module")
def lib():
    return A.built_lib()


def test_guide_names():
    from diffcodec_amd import lib
    names = set(lib.GUIDE_SIGNATURES)
    assert all(n.startswith("dc_guide_") for n in names) and names == STAGES | {"dc_guide_watershed", "dc_guide_ws_bytes"}
    assert set(QUERIES) <= names


def census(signatures):
    """-> (launchers with no literal lib.call in tests/test_gpu_guide_points.py or guide_points.py, queries guide_points.py never asks)"""
    from diffcodec_amd import guide_points
    return A.family_census(signatures, QUERIES, A.module_source("test_gpu_guide_points"), open(guide_points.__file__).read())


def test_every_launcher_is_called_by_the_gpu_tests_or_by_the_product():
    from diffcodec_amd import guide_points, lib
    uncalled, unnamed = census(lib.GUIDE_SIGNATURES)
    assert not uncalled, f"no literal lib.call in tests/test_gpu_guide_points.py or guide_points.py: {uncalled}"
    assert not unnamed, f"guide_points.py never asks: {unnamed}"
    assert census(dict(lib.GUIDE_SIGNATURES, dc_guide_imaginary=[]))[0] == ["dc_guide_imaginary"]
    tests = A.lib_calls(A.module_source("test_gpu_guide_points"))
    assert STAGES <= tests, STAGES - tests                                    # the per-stage entries are what the edge tests call
    assert "dc_guide_watershed" in A.lib_calls(open(guide_points.__file__).read())


def test_launchers_refuse_before_any_launch(lib):
    """no GPU needed: every refusal returns -1 before anything is launched"""
    l = lib.load()
    P = 256                                                                   # a non-null pointer nothing reads: the shape is refused first
    up = lambda v: (v + 255) // 256 * 256
    for N, H, W in ((1, 3, 3), (3, 37, 53), (2, 1080, 1920), (2, 24, 801)):
        ds = max(1, max(H, W) // 400)
        h, w = -(-H // ds), -(-W // ds)
        need = N * h * w * (4 + 4 + 4 + 1 + 1) + 4 * N * h + 4 * N + 4 * N * -(-h * w // 256) + 4 * N
        assert need <= l.dc_guide_ws_bytes(N, H, W) <= need + 9 * 256, (N, H, W)
        assert l.dc_guide_ws_bytes(N, H, W) == up(l.dc_guide_ws_bytes(N, H, W))
    for bad in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (-1, 8, 8), (70000, 8, 8)):
        assert l.dc_guide_ws_bytes(*bad) == -1, bad
    assert l.dc_guide_edge(None, 1, 8, 8, P, P, P, None) == -1 and l.dc_guide_edge(P, 1, 8, 8, None, P, P, None) == -1
    assert l.dc_guide_edge(P, 1, 8, 8, P, None, None, None) == -1 and l.dc_guide_edge(P, 0, 8, 8, P, P, P, None) == -1
    assert l.dc_guide_edge(P, 1, 0, 8, P, P, P, None) == -1 and l.dc_guide_edge(P, 1, 8, 0, P, P, P, None) == -1
    assert l.dc_guide_edt(None, 1, 8, 8, P, P, None) == -1 and l.dc_guide_edt(P, 1, 8, 8, P, None, None) == -1
    assert l.dc_guide_edt(P, 1, 8, 8, None, P, None) == -1 and l.dc_guide_edt(P, 0, 8, 8, P, P, None) == -1
    assert l.dc_guide_edt(P, 1, 0, 8, P, P, None) == -1 and l.dc_guide_edt(P, 1, 8, 800, P, P, None) == -1
    assert l.dc_guide_nms(None, 1, 8, 8, 3, P, P, None) == -1 and l.dc_guide_nms(P, 1, 8, 8, 3, P, None, None) == -1
    for ks in (4, 1, 2, 0, -3, 14):
        assert l.dc_guide_nms(P, 1, 8, 8, ks, P, P, None) == -1, ks
        assert l.dc_guide_select(P, 1, 8, 8, ks, 1, P, P, P, 64, None) == -1, ks
        assert l.dc_guide_watershed(P, 1, 8, 8, ks, 0, P, P, P, 64, None, None) == -1, ks
    assert l.dc_guide_nms(P, 1, 8, 0, 3, P, P, None) == -1 and l.dc_guide_nms(P, 0, 8, 8, 3, P, P, None) == -1
    assert l.dc_guide_select(None, 1, 8, 8, 3, 1, P, P, P, 64, None) == -1 and l.dc_guide_select(P, 1, 8, 8, 3, 1, P, None, P, 64, None) == -1
    assert l.dc_guide_select(P, 1, 8, 8, 3, 1, P, P, None, 64, None) == -1 and l.dc_guide_select(P, 1, 8, 8, 3, 0, P, P, P, 64, None) == -1
    assert l.dc_guide_select(P, 1, 8, 8, 3, 1, P, P, P, 63, None) == -1                # cap below ceil(8 / 1) * ceil(8 / 1)
    assert l.dc_guide_select(P, 1, 8, 8, 5, 1, P, P, P, 15, None) == -1 and l.dc_guide_select(P, 0, 8, 8, 5, 1, P, P, P, 16, None) == -1
    assert l.dc_guide_scatter(None, 1, 8, 8, 4, P, P, 4, P, None) == -1 and l.dc_guide_scatter(P, 1, 8, 8, 4, None, P, 4, P, None) == -1
    assert l.dc_guide_scatter(P, 1, 8, 8, 4, P, P, 4, None, None) == -1 and l.dc_guide_scatter(P, 1, 8, 8, -1, P, P, 4, P, None) == -1
    assert l.dc_guide_scatter(P, 1, 8, 8, 4, P, P, 0, P, None) == -1 and l.dc_guide_scatter(P, 1, 0, 8, 4, P, P, 4, P, None) == -1
    assert l.dc_guide_watershed(None, 1, 8, 8, 3, 0, P, P, P, 64, None, None) == -1
    assert l.dc_guide_watershed(P, 1, 8, 8, 3, 0, None, P, P, 64, None, None) == -1
    assert l.dc_guide_watershed(P, 1, 8, 8, 3, 0, P, None, P, 64, None, None) == -1
    assert l.dc_guide_watershed(P, 0, 8, 8, 3, 0, P, P, P, 64, None, None) == -1 and l.dc_guide_watershed(P, 1, 8, 0, 3, 0, P, P, P, 64, None, None) == -1
    assert l.dc_guide_watershed(P, 1, 8, 8, 3, -1, P, P, P, 64, None, None) == -1 and l.dc_guide_watershed(P, 1, 8, 8, 3, 0, P, P, P, 63, None, None) == -1
