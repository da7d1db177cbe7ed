"""GPU: csrc/guide_points.hip against tests/guide_ref.py (itself pinned to the reference by tests/test_guide_ref.py), per stage
and fused.

  edge      the normalised magnitude against the fp64 restatement at 4x the error of the same arithmetic in fp32 on the CPU; the
            byte map equal to the fp64 restatement's wherever the fp64 value is farther from 0.1 than that bar, with at most 0.5 %
            of the pixels left out (the fixtures leave out none).  Measured on the MI355X over the nine flows: device error 0 to
            1.5e-7 against 0 to 1.8e-7 for the CPU's fp32 (ratio 0.6 to 1.1; the CPU's bits in two cases), no pixel left out.
  edt, nms, select, scatter
            bit for bit, each fed the restatement's own input: 3x3 and 1x7 images, 37x53, an edge pixel in each corner, all and no
            edges, two parallel lines 16 apart (a plateau of ties), ks = 3, 15, 81, a 300x400 image (several blocks per row and
            per column), dense random candidate masks, N = 3 against N = 1.
  fused     equals the chain of stages and the golden's candidates; a 24x801 flow (ds = 2, ragged last column); eager equals a
            captured graph's replay; two runs are bit-identical; sample_watershed equals the union of sample_grid and the
            restatement; PropagatedFlowSource passes that operand on."""
import functools
import os

import numpy as np
import pytest
import torch

import edge_cases as E
import guide_ref as G
from diffcodec_amd import lib
from diffcodec_amd import guide_points as GP

pytestmark = pytest.mark.gpu

DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "guide_points.npz")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ws(N, H, W):
    """a guarded fp32 workspace of exactly dc_guide_ws_bytes holding the NaN pattern; `_done` checks its guards"""
    nbytes = lib.load().dc_guide_ws_bytes(N, H, W)
    assert nbytes > 0 and nbytes % 4 == 0
    ws = E.Guarded((nbytes // 4,), torch.float32, DEV)
    assert ws.view.data_ptr() % 256 == 0
    return ws


def _done(ws, what):
    torch.cuda.synchronize()
    ws.assert_intact(f"{what}: workspace")


# ------------------------------------------------------------------------------------------------ the stage entries
def dev_edge(flow):
    """flow [N,2,H,W] on the host -> (normalised magnitude, edge bytes) [N,h,w] from the device"""
    flow = flow.to(DEV).contiguous()
    N, _, H, W = flow.shape
    _, h, w = GP.working_size(H, W)
    mag = torch.full((N, h, w), -1.0, dtype=torch.float32, device=DEV)
    edge = torch.full((N, h, w), 7, dtype=torch.uint8, device=DEV)
    ws = _ws(N, H, W)
    lib.call("dc_guide_edge", flow.data_ptr(), N, H, W, ws.view.data_ptr(), mag.data_ptr(), edge.data_ptr(), _stream())
    _done(ws, "dc_guide_edge")
    return mag.cpu(), edge.cpu()


def dev_edt(edge):
    edge = torch.as_tensor(np.asarray(edge), dtype=torch.uint8).to(DEV).contiguous()
    N, h, w = edge.shape
    d2 = torch.full((N, h, w), -1, dtype=torch.int32, device=DEV)
    ws = _ws(N, h, w)
    lib.call("dc_guide_edt", edge.data_ptr(), N, h, w, ws.view.data_ptr(), d2.data_ptr(), _stream())
    _done(ws, "dc_guide_edt")
    return d2.cpu().numpy()


def dev_nms(d2, ks):
    d2 = torch.as_tensor(np.asarray(d2), dtype=torch.int32).to(DEV).contiguous()
    N, h, w = d2.shape
    cand = torch.full((N, h, w), 7, dtype=torch.uint8, device=DEV)
    ws = _ws(N, h, w)
    lib.call("dc_guide_nms", d2.data_ptr(), N, h, w, ks, ws.view.data_ptr(), cand.data_ptr(), _stream())
    _done(ws, "dc_guide_nms")
    return cand.cpu().numpy()


def dev_select(cand, ks, scale=1, slack=0):
    cand = torch.as_tensor(np.asarray(cand), dtype=torch.uint8).to(DEV).contiguous()
    N, h, w = cand.shape
    cap = GP.max_points(h, w, ks) + slack
    counts = torch.full((N,), -7, dtype=torch.int32, device=DEV)
    points = torch.full((N, cap, 2), -7, dtype=torch.int32, device=DEV)
    ws = _ws(N, h, w)
    lib.call("dc_guide_select", cand.data_ptr(), N, h, w, ks, scale, ws.view.data_ptr(), counts.data_ptr(), points.data_ptr(), cap, _stream())
    _done(ws, "dc_guide_select")
    return counts.cpu().numpy(), points.cpu().numpy()


def dev_scatter(flow, stride, counts, points):
    flow = flow.to(DEV).contiguous()
    N, _, H, W = flow.shape
    counts = torch.as_tensor(counts, dtype=torch.int32).to(DEV).contiguous()
    points = torch.as_tensor(points, dtype=torch.int32).to(DEV).contiguous()
    sparse = torch.full((N, 4, H, W), float("nan"), dtype=torch.float32, device=DEV)
    lib.call("dc_guide_scatter", flow.data_ptr(), N, H, W, stride, counts.data_ptr(), points.data_ptr(), points.shape[1], sparse.data_ptr(),
             _stream())
    torch.cuda.synchronize()
    return sparse.cpu()


def check_points(counts, points, want, scale=1):
    """want: per image the (ys, xs) of the survivors in order"""
    for n, (ys, xs) in enumerate(want):
        k = len(ys)
        assert counts[n] == k, (n, counts[n], k)
        assert np.array_equal(points[n, :k, 0], ys * scale) and np.array_equal(points[n, :k, 1], xs * scale), n
        assert (points[n, k:] == -1).all(), n


# ------------------------------------------------------------------------------------------------ fixtures
@functools.lru_cache(maxsize=None)
def golden():
    return G.load_golden(GOLDEN)


@functools.lru_cache(maxsize=None)
def gflow(name):
    """the golden case's flow [2,H,W], rebuilt from its parameters when a test first asks"""
    c = golden()[name]
    return G.to_nchw(G.synth_flow(c["params"], c["H"], c["W"]))[0]


def _flow(H, W, seed, discs=3):
    return G.to_nchw(G.synth_flow(G.synth_params(seed, H, W, discs), H, W))[0]


def _plateau(h=48, w=70):
    e = np.zeros((h, w), dtype=bool)
    e[:, 20] = e[:, 36] = True
    return e


@functools.lru_cache(maxsize=None)
def edge_patterns():
    rng = np.random.RandomState(3)
    corners = np.zeros((37, 53), dtype=bool)
    corners[0, 0] = corners[0, -1] = corners[-1, 0] = corners[-1, -1] = True
    one_column = np.zeros((24, 40), dtype=bool)
    one_column[5, 39] = True
    pats = {
        "3x3": rng.rand(3, 3) < 0.3, "3x3_centre": np.eye(3, dtype=bool) & (np.arange(3) == 1), "1x7": rng.rand(1, 7) < 0.3,
        "7x1": rng.rand(7, 1) < 0.3, "37x53": rng.rand(37, 53) < 0.02, "corners": corners, "all": np.ones((37, 53), dtype=bool),
        "none": np.zeros((37, 53), dtype=bool), "plateau": _plateau(), "24x40": rng.rand(24, 40) < 0.01, "one_pixel": one_column,
        "300x400": rng.rand(300, 400) < 0.0005, "65x257": rng.rand(65, 257) < 0.003,
    }
    for name in ("small", "bands", "odd"):
        pats["golden_" + name] = golden()[name]["edge"]
    return pats


@functools.lru_cache(maxsize=None)
def ref_d2(name):
    return G.sqdist(edge_patterns()[name])


# ------------------------------------------------------------------------------------------------ stage 1
EDGE_FLOWS = {
    "3x3": lambda: _flow(3, 3, 21, 1), "1x7": lambda: _flow(1, 7, 22, 1), "37x53": lambda: _flow(37, 53, 23), "64x96": lambda: _flow(64, 96, 24),
    "24x801": lambda: _flow(24, 801, 25), "130x270": lambda: _flow(130, 270, 26, 5), "zero": lambda: torch.zeros(2, 19, 23),
    "faint": lambda: _flow(37, 53, 27) * 1e-4, "golden_half_hd": lambda: gflow("half_hd"),
}


@pytest.mark.parametrize("name", sorted(EDGE_FLOWS))
def test_edge_magnitude_and_map(record, name):
    flow = EDGE_FLOWS[name]()[None]
    want = G.edge_magnitude(flow, torch.float64)
    cpu32 = G.edge_magnitude(flow, torch.float32)
    bar = 4.0 * float((cpu32.double() - want).abs().max())
    mag, edge = dev_edge(flow)
    err = float((mag.double() - want).abs().max())
    print(f"edge {name}: device error {err:.3e}, fp32 CPU error {bar / 4:.3e}, bits equal to the CPU fp32: {torch.equal(mag, cpu32)}")
    record(f"guide_edge_err/{name}", err)
    record(f"guide_edge_cpu32_err/{name}", bar / 4)
    assert mag.shape == want.shape and err <= bar, (err, bar)
    decided = (want - 0.1).abs() > bar
    left_out = 1.0 - float(decided.double().mean())
    print(f"edge {name}: {int((~decided).sum())} pixels within {bar:.3e} of the threshold")
    assert left_out <= 0.005
    assert torch.equal(edge.bool()[decided], G.edge_map(want)[decided]) and bool(((edge == 0) | (edge == 1)).all())


def test_edge_map_of_the_golden_flows():
    for name in ("small", "bands", "qvga", "full_hd", "constant"):
        c = golden()[name]
        _, edge = dev_edge(gflow(name)[None])
        assert np.array_equal(edge[0].numpy().astype(bool), c["edge"]), name


# ------------------------------------------------------------------------------------------------ stage 2
@pytest.mark.parametrize("name", sorted(edge_patterns()))
def test_squared_distance_bit_for_bit(name):
    got = dev_edt(edge_patterns()[name][None])
    assert got.dtype == np.int32 and np.array_equal(got[0], ref_d2(name))
    if name == "none":
        assert (got == G.NO_EDGE).all()


def test_squared_distance_of_a_batch():
    names = ("37x53", "corners", "none")
    got = dev_edt(np.stack([edge_patterns()[n] for n in names]))
    for i, n in enumerate(names):
        assert np.array_equal(got[i], ref_d2(n)), n


# ------------------------------------------------------------------------------------------------ stage 3
NMS_CASES = [(n, ks) for n in sorted(edge_patterns()) for ks in (3, 15, 81) if n not in ("300x400",)] + [("300x400", 15), ("24x40", 2001)]


@pytest.mark.parametrize("name,ks", NMS_CASES, ids=[f"{n}-ks{k}" for n, k in NMS_CASES])
def test_nms_bit_for_bit(name, ks):
    d2 = ref_d2(name)
    got = dev_nms(d2[None], ks)
    assert np.array_equal(got[0].astype(bool), G.candidates(d2, ks)) and ((got == 0) | (got == 1)).all()
    if min(d2.shape) < 3 or name in ("all", "none"):
        assert not got.any()                                          # the border removal (or the rule) empties everything


def test_nms_of_a_batch():
    d2 = np.stack([ref_d2(n) for n in ("37x53", "none", "corners")])
    got = dev_nms(d2, 15)
    for i in range(3):
        assert np.array_equal(got[i].astype(bool), G.candidates(d2[i], 15)), i


# ------------------------------------------------------------------------------------------------ stage 4
@functools.lru_cache(maxsize=None)
def cand_masks():
    rng = np.random.RandomState(5)
    masks = {"plateau_ks%d" % ks: (G.candidates(ref_d2("plateau"), ks), ks) for ks in (3, 5, 15)}
    for ks in (3, 7, 15, 81):
        masks["dense37x53_ks%d" % ks] = (rng.rand(37, 53) < 0.3, ks)
    masks["full37x53_ks5"] = (np.ones((37, 53), dtype=bool), 5)
    masks["dense300x400_ks15"] = (rng.rand(300, 400) < 0.2, 15)
    masks["sparse300x400_ks41"] = (rng.rand(300, 400) < 0.002, 41)
    masks["rows130x270_ks9"] = (np.repeat(rng.rand(130, 1) < 0.5, 270, 1), 9)
    masks["empty"] = (np.zeros((37, 53), dtype=bool), 15)
    masks["3x3"] = (np.ones((3, 3), dtype=bool), 3)
    masks["1x7"] = (np.ones((1, 7), dtype=bool), 3)
    masks["last_pixel"] = (np.arange(24 * 40).reshape(24, 40) == 24 * 40 - 1, 81)
    for name in ("bands", "bands_ks5", "odd", "qvga"):
        masks["golden_" + name] = (golden()[name]["cand"], golden()[name]["ks"])
    return masks


@pytest.mark.parametrize("name", sorted(cand_masks()))
def test_select_bit_for_bit(name):
    cand, ks = cand_masks()[name]
    ys, xs = G.greedy(*np.nonzero(cand), (ks - 1) / 2)
    scale = 3 if name.startswith("plateau") else 1
    counts, points = dev_select(cand[None], ks, scale, slack=5 if name == "empty" else 0)
    check_points(counts, points, [(ys, xs)], scale)
    if name == "plateau_ks15":                                        # the spacing, stated on the device's own output
        assert int(cand.sum()) > 40 and counts[0] > 3
        p = points[0, :counts[0]] // scale
        near = (np.abs(p[:, None, 0] - p[None, :, 0]) < 7) & (np.abs(p[:, None, 1] - p[None, :, 1]) < 7)
        assert int(near.sum()) == counts[0]


def test_select_of_a_batch_has_each_images_own_bits():
    names = ("dense37x53_ks15", "empty", "full37x53_ks5")
    cands = np.stack([cand_masks()[n][0] for n in names])
    counts, points = dev_select(cands, 15)
    check_points(counts, points, [G.greedy(*np.nonzero(c), 7) for c in cands])
    for i in range(3):
        c1, p1 = dev_select(cands[i:i + 1], 15)
        assert c1[0] == counts[i] and np.array_equal(p1[0], points[i])


# ------------------------------------------------------------------------------------------------ stage 5
@pytest.mark.parametrize("H,W,stride", [(37, 53, 0), (37, 53, 8), (9, 11, 1), (64, 88, 16), (3, 3, 5)])
def test_scatter_bit_for_bit(H, W, stride):
    rng = np.random.RandomState(H + stride)
    flow = torch.from_numpy(rng.randn(2, 2, H, W).astype(np.float32))
    cap = 12
    points = np.full((2, cap, 2), -1, dtype=np.int32)
    counts = np.array([5, 0], dtype=np.int32)
    points[0, :5] = np.stack([rng.randint(0, H, 5), rng.randint(0, W, 5)], 1)
    if stride:
        gy, gx = G.grid_points(H, W, stride)
        points[0, 0] = (gy[0], gx[-1])                                # a watershed point on a grid point
    points[1, :3] = (1, 1)                                            # past counts[1]: not a point
    got = dev_scatter(flow, stride, counts, points)
    for n in range(2):
        m = np.zeros((H, W), dtype=bool)
        if stride:
            m[np.ix_(*G.grid_points(H, W, stride))] = True
        m[points[n, :counts[n], 0], points[n, :counts[n], 1]] = True
        assert torch.equal(got[n], G.sparse_of(flow[n], m)), n


# ------------------------------------------------------------------------------------------------ the whole path
def chain(flow, ks, stride):
    """the five stage entries one after another, on the host's copies of each stage's output"""
    N, _, H, W = flow.shape
    ds, h, w = GP.working_size(H, W)
    _, edge = dev_edge(flow)
    d2 = dev_edt(edge.numpy())
    cand = dev_nms(d2, ks)
    counts, points = dev_select(cand, ks, ds)
    return cand, counts, points, dev_scatter(flow, 0 if stride is None else stride, counts, points)


FUSED = ["small", "bands", "bands_ks5", "odd", "qvga", "wide_window", "square512", "half_hd", "full_hd", "constant"]


@pytest.mark.parametrize("name", FUSED)
def test_fused_equals_the_chain_and_the_golden(name):
    c = golden()[name]
    flow, ks, stride = gflow(name)[None], c["ks"], c["stride"]
    cand, counts, points, sparse = chain(flow, ks, stride)
    assert np.array_equal(cand[0].astype(bool), c["cand"])
    ds = G.working_ds(c["H"], c["W"])
    ys, xs = G.greedy(*np.nonzero(c["cand"]), (ks - 1) / 2)
    check_points(counts, points, [(ys, xs)], ds)
    dflow = flow.to(DEV)
    fc, fp = GP.watershed_points(dflow, ks)
    fs = GP.sample_watershed(dflow, ks, stride=stride)
    torch.cuda.synchronize()
    assert np.array_equal(fc.cpu().numpy(), counts) and np.array_equal(fp.cpu().numpy(), points) and torch.equal(fs.cpu(), sparse)
    m = np.zeros((c["H"], c["W"]), dtype=bool)
    m[np.ix_(*G.grid_points(c["H"], c["W"], stride))] = True
    m[ys * ds, xs * ds] = True
    assert torch.equal(fs[0].cpu(), G.sparse_of(flow[0], m))
    if len(ys) == int(c["cand"].sum()):                               # no pair of candidates in one box: the coin was never drawn
        assert np.array_equal(m, c["mask"])


@pytest.mark.parametrize("H,W,ks,stride", [(24, 801, 3, 8), (24, 801, 15, None), (64, 88, 15, 8), (3, 3, 3, 2), (1, 7, 3, None), (37, 53, 81, 8)])
def test_sample_watershed_is_the_union_of_the_grid_and_the_restatement(H, W, ks, stride):
    from diffcodec_amd.flow_propagation import sample_grid
    flow = torch.stack([_flow(H, W, 40 + i, 4) for i in range(2)])
    dflow = flow.to(DEV)
    got = GP.sample_watershed(dflow, ks, stride=stride)
    counts, points = GP.watershed_points(dflow, ks)
    grid = sample_grid(dflow, stride).cpu() if stride else torch.zeros(2, 4, H, W)
    torch.cuda.synchronize()
    got, counts, points = got.cpu(), counts.cpu().numpy(), points.cpu().numpy()
    want_pts = []
    for n in range(2):
        _, ys, xs, ds = G.watershed(flow[n], ks, big=True)
        want_pts.append((ys, xs))
        m = np.zeros((H, W), dtype=bool)
        m[ys * ds, xs * ds] = True
        alone = G.sparse_of(flow[n], m)
        assert torch.equal(got[n], torch.where(grid[n, 2:3] > 0, grid[n], alone)), n
    check_points(counts, points, want_pts, G.working_ds(H, W))
    if (H, W) == (24, 801):
        assert G.working_ds(H, W) == 2 and sum(len(p[0]) for p in want_pts) > 0


def test_a_batch_has_the_bits_each_image_has_alone():
    flow = torch.stack([_flow(37, 53, 50), gflow("bands")[:, :37, :53], torch.zeros(2, 37, 53)]).to(DEV)
    counts, points = GP.watershed_points(flow, 5)
    sparse = GP.sample_watershed(flow, 5, stride=8)
    for n in range(3):
        c1, p1 = GP.watershed_points(flow[n:n + 1], 5)
        s1 = GP.sample_watershed(flow[n:n + 1], 5, stride=8)
        assert torch.equal(c1[0], counts[n]) and torch.equal(p1[0], points[n]) and torch.equal(s1[0], sparse[n]), n
    assert int(counts[1]) > 3 and int(counts[2]) == 0


def test_graph_replay_and_a_second_run_give_the_same_bits():
    flow = torch.stack([gflow("bands"), _flow(48, 80, 60)]).to(DEV)
    eager = GP.sample_watershed(flow, 15, stride=16)
    ec, ep = GP.watershed_points(flow, 15)
    again = GP.sample_watershed(flow, 15, stride=16)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        GP.sample_watershed(flow, 15, stride=16)                      # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = GP.sample_watershed(flow, 15, stride=16)
        cc, cp = GP.watershed_points(flow, 15)
    for _ in range(2):
        captured.fill_(float("nan"))
        cp.fill_(-9)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(captured, eager) and torch.equal(cc, ec) and torch.equal(cp, ep)
    assert torch.equal(again, eager) and int(ec.sum()) > 4


def test_propagated_flow_source_passes_the_watershed_operand_on():
    from diffcodec_amd.flow_propagation import PropagatedFlowSource, sample_grid

    class Inner:
        def controls(self, frame, prev, nxt):
            flow = torch.cat([gflow("bands"), _flow(48, 80, 61)], 0)[None].to(DEV)
            return torch.rand(1, 6, 48, 80, generator=torch.Generator().manual_seed(3)).to(DEV), flow

    class Model:
        def flow(self, image, sparse):
            self.sparse = sparse
            return sparse[:, :2] + sparse[:, 2:]

    inner, model = Inner(), Model()
    _, flow0 = inner.controls(1, 0, 2)
    both = torch.cat([flow0[:, :2], flow0[:, 2:]], 0).contiguous()
    PropagatedFlowSource(inner, model, stride=16, nms_ks=15).controls(1, 0, 2)
    assert torch.equal(model.sparse, GP.sample_watershed(both, 15, stride=16))
    assert int(model.sparse[:, 2].sum()) > int(sample_grid(both, 16)[:, 2].sum())
    PropagatedFlowSource(inner, model, stride=16).controls(1, 0, 2)
    assert torch.equal(model.sparse, sample_grid(both, 16))


# ------------------------------------------------------------------------------------------------ the caller-owned workspace
# (N, H, W, ks, stride): odd H and W that are multiples of neither the grid stride nor the NMS window; the 1 x 1 working image
WS_CASES = [(3, 37, 53, 5, 8), (2, 1, 1, 3, 2)]


def _ws_flows(N, H, W, seed):
    if H == 1:
        return torch.randn(N, 2, H, W, generator=torch.Generator().manual_seed(seed))
    return torch.stack([_flow(H, W, seed + i, 4) for i in range(N)])


@pytest.mark.parametrize("N,H,W,ks,stride", WS_CASES, ids=[f"n{c[0]}_{c[1]}x{c[2]}_ks{c[3]}" for c in WS_CASES])
def test_every_entry_on_a_guarded_workspace_of_any_contents(record, N, H, W, ks, stride):
    """the five stage entries, each fed the stage before it, and dc_guide_watershed, each on a guarded workspace of exactly
    dc_guide_ws_bytes under the NaN, zero and stale fills (the stale one left by the same entry on other flows): integer-exact, so
    equality under the fills covers the counts, the points and the scattered map; the chain's and the fused entry's outputs are the
    bits watershed_points / sample_watershed return.  (dc_guide_scatter takes no workspace: it runs under the same guards.)"""
    ds, h, w = GP.working_size(H, W)
    assert ds == 1
    cap = GP.max_points(h, w, ks)
    nbytes = lib.load().dc_guide_ws_bytes(N, H, W)
    flows = [_ws_flows(N, H, W, seed).to(DEV).contiguous() for seed in (70, 170)]
    # the other flows' stage outputs, through the stage entries on their own workspaces: what each prime launch is fed
    _, edge_p = dev_edge(flows[1].cpu())
    d2_p = dev_edt(edge_p.numpy())
    cand_p = dev_nms(d2_p, ks)
    counts_p, points_p = dev_select(cand_p, ks, ds)
    fed = {"edge": [flows[0], flows[1]], "edt": [None, edge_p.to(DEV)], "nms": [None, torch.from_numpy(d2_p).to(DEV)],
           "select": [None, torch.from_numpy(cand_p).to(DEV)],
           "scatter": [None, (torch.from_numpy(counts_p).to(DEV), torch.from_numpy(points_p).to(DEV))]}
    tag = f"{N}x{H}x{W} ks{ks}"

    def run(name, launch, outputs):
        outs, share = E.run_on_fills(launch, nbytes, outputs, f"dc_guide_{name} {tag}", device=DEV)
        record(f"ws_unwritten_share[dc_guide_{name} {tag}]", share)
        return outs

    def edge(ws, outs, prime):
        lib.call("dc_guide_edge", fed["edge"][int(prime)].data_ptr(), N, H, W, ws.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(), _stream())

    _, e = run("edge", edge, [((N, h, w), torch.float32), ((N, h, w), torch.uint8)])
    fed["edt"][0] = e

    def edt(ws, outs, prime):
        lib.call("dc_guide_edt", fed["edt"][int(prime)].data_ptr(), N, h, w, ws.data_ptr(), outs[0].data_ptr(), _stream())

    fed["nms"][0], = run("edt", edt, [((N, h, w), torch.int32)])

    def nms(ws, outs, prime):
        lib.call("dc_guide_nms", fed["nms"][int(prime)].data_ptr(), N, h, w, ks, ws.data_ptr(), outs[0].data_ptr(), _stream())

    fed["select"][0], = run("nms", nms, [((N, h, w), torch.uint8)])

    def select(ws, outs, prime):
        lib.call("dc_guide_select", fed["select"][int(prime)].data_ptr(), N, h, w, ks, ds, ws.data_ptr(), outs[0].data_ptr(),
                 outs[1].data_ptr(), cap, _stream())

    counts, points = run("select", select, [((N,), torch.int32), ((N, cap, 2), torch.int32)])
    fed["scatter"][0] = (counts, points)

    def scatter(ws, outs, prime):
        c, p = fed["scatter"][int(prime)]
        lib.call("dc_guide_scatter", flows[int(prime)].data_ptr(), N, H, W, stride, c.data_ptr(), p.data_ptr(), cap, outs[0].data_ptr(), _stream())

    sparse, = run("scatter", scatter, [((N, 4, H, W), torch.float32)])

    def fused(ws, outs, prime):
        lib.call("dc_guide_watershed", flows[int(prime)].data_ptr(), N, H, W, ks, stride, ws.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(),
                 cap, outs[2].data_ptr(), _stream())

    fc, fp, fs = run("watershed", fused, [((N,), torch.int32), ((N, cap, 2), torch.int32), ((N, 4, H, W), torch.float32)])
    wc, wp = GP.watershed_points(flows[0], ks)
    wsparse = GP.sample_watershed(flows[0], ks, stride=stride)
    for got in ((counts, points, sparse), (fc, fp, fs)):
        assert torch.equal(got[0], wc) and torch.equal(got[1], wp) and torch.equal(E.ws_bits(got[2]), E.ws_bits(wsparse))
    if H > 1:
        assert int(wc.sum()) > 0 and int(counts_p.sum()) > 0                                      # both sets of flows have points
