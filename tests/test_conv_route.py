"""CPU: the dispatcher's route query (dc_conv_route: host code, launches nothing) — its kernel codes match the header, the
query `ops.rowpanel_takes` that steers the transformer's proj_in agrees with the independent closed form of tests/block_ref.py on
every shape the models launch, and the split-K the library picks under DC_SPLITK_AUTO is the rule `ops.py` used to state
(tests/splitk_rule_ref.py), restricted to the splits the route accepts; `ops.conv_plan` of a picked split routes as its descriptor."""
import collections
import itertools
import math
import os
import re

import pytest

import block_ref
import edge_cases as E
import splitk_rule_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as g
    from diffcodec_amd import lib, ops as o
    if not os.path.exists(lib.LIB_PATH):
        g.build()
    return o


def _desc(ops, rows, per_sample, cin, cout, **kw):
    from diffcodec_amd.lib import ConvDesc
    n = rows // per_sample
    base = dict(x1=16, w=16, out=16, bias=16, N=n, H=1, W=per_sample, C1=cin, Cout=cout, ksize=1, stride=1, pad=0, Ho=1,
                Wo=per_sample, out_scale=1.0, splitk=1)
    base.update(kw)
    return ConvDesc(**base)


def test_route_names_match_the_header(ops):
    src = open(os.path.join(ROOT, "include", "diffcodec_hip.h")).read()
    codes = {int(v): k.lower() for k, v in re.findall(r"#define DC_ROUTE_([A-Z0-9_]+) (\d+)", src) if k != "INFO_INTS"}
    assert ops.ROUTE_NAMES == codes
    assert int(re.search(r"#define DC_ROUTE_INFO_INTS (\d+)", src).group(1)) == 5


# transformer widths x map sizes (512x512 frames / windows: latent 64x64 and its three down levels) x the samples of one launch
# (cfg-shared halves and full CFG batches of the 1 / 2 (C4 windows) / 11 / 16 / 44-frame legs)
SHAPES = [(c, hw, n) for c, hw in ((320, 4096), (640, 1024), (1280, 256), (1280, 64))
          for n in (1, 2, 4, 11, 16, 22, 32, 44, 88)]


@pytest.mark.parametrize("c,hw,n", SHAPES)
def test_rowpanel_takes_agrees_with_the_route(ops, c, hw, n):
    rows = n * hw
    want = block_ref.rowpanel_takes(rows, hw, c, c)
    assert ops.rowpanel_takes(rows, hw, c, c) == want
    from diffcodec_amd import lib
    r = ops.conv_route(_desc(ops, rows, hw, c, c, gn_ab=16, gn_batch=n))
    assert (r.kernel == "gemm_rowpanel") == want, (c, hw, n, r)
    # blocks.py asks for the statistics epilogue together with the affine on load exactly when the rule admits the shape; the
    # gather GEMM that takes the other shapes has no such epilogue, and the library refuses the combination there
    d = _desc(ops, rows, hw, c, c, gn_ab=16, gn_batch=n, stats_out=16)
    if want:
        assert ops.conv_route(d).kernel == "gemm_rowpanel"
    else:
        with pytest.raises(lib.HipLaunchError):
            ops.conv_route(d)
    for extra in ({}, {"stats_out": 16}):                    # the same GEMM without the affine on load
        r = ops.conv_route(_desc(ops, rows, hw, c, c, **extra))
        assert (r.kernel == "gemm_rowpanel") == want, (c, hw, n, extra, r)


@pytest.mark.parametrize("extra", [dict(residual=16), dict(stats_out=16), dict(row_add=16), dict(act=1)])
def test_folded_layernorm_partials_route_finalizes_first(ops, extra):
    """K = 320, M = 65536 with raw LayerNorm partials and an epilogue the row-panel kernel does not specialise: the library
    finalizes first (needs ln_scratch); the plain form stays on the row-panel kernel, which finalizes in its prologue."""
    r = ops.conv_route(_desc(ops, 65536, 4096, 320, 320, ln_stats=16, ln_colsum=16, ln_parts=4, **extra))
    assert r.ln_first and r.kernel != "gemm_rowpanel", r
    r = ops.conv_route(_desc(ops, 65536, 4096, 320, 320, ln_stats=16, ln_colsum=16, ln_parts=4))
    assert not r.ln_first and r.kernel == "gemm_rowpanel", r


def test_route_reports_the_split_k_fixpoint_and_refuses_invalid_descriptors(ops):
    from diffcodec_amd import lib
    # 3x3 stride-2 gather GEMM, K = 9 * 20 steps: split 7 owns ceil(180/7) = 26 steps -> 7 splits; 19 -> 10 steps each -> 18
    d = _desc(ops, 32 * 32, 32 * 32, 1280, 1280, ksize=3, stride=2, pad=1, N=1, H=64, W=64, Ho=32, Wo=32, splitk=19)
    r = ops.conv_route(d)
    assert r.kernel == "igemm" and r.splitk == 18, r
    with pytest.raises(lib.HipLaunchError):
        ops.conv_route(_desc(ops, 4096, 4096, 320, 320, Cout=330))


# ------------------------------------------------------------------------------------------- DC_SPLITK_AUTO
# 9 * 6 * 9 * 8 * 4 * 5 = 77,760 descriptors: the batches of the decode legs, square and ragged maps, every UNet width (and the
# skip concats), Cout from conv_out's 4 to the GEGLU-sized 10240, every conv form and every operand that steers the route
GRID_N = (1, 2, 4, 11, 16, 22, 32, 44, 88)
GRID_MAPS = ((8, 8), (16, 16), (32, 32), (64, 64), (12, 20), (13, 9))
GRID_CIN = (128, 256, 512, 320, 640, 960, 1280, 1920, 2560)
GRID_COUT = (4, 128, 256, 320, 512, 640, 1280, 10240)
GRID_FORMS = ((1, 1, 0), (3, 1, 0), (3, 1, 1), (3, 2, 0))              # (ksize, stride, upsample)
GRID_OPERANDS = ("plain", "residual", "row_add", "gn_silu", "concat")

# how often the frozen rule takes each of its branches on this grid, counted on the frozen rule alone (a changed grid or a changed
# reference shows here before it can make the equality below vacuous)
BRANCH_COUNTS = {"tiles >= 512": 25785, "short-K exit": 13860, "1x1 m >= 2048, kt < 128": 770, "target 1024 reached": 3345,
                 "target 256 reached": 6230, "tile kernel big-map target": 2600, "general fallback": 4280, "strided reached": 7200,
                 "strided fallback": 9810}


def _grid_desc(n, hw, cin, cout, form, operand, splitk):
    from diffcodec_amd.lib import ConvDesc
    (h, w), (k, stride, up) = hw, form
    ho, wo = ((((2 * h if up else h) - 1) // stride + 1), (((2 * w if up else w) - 1) // stride + 1)) if k == 3 else (h, w)
    kw = dict(x1=16, w=16, out=16, bias=16, N=n, H=h, W=w, C1=cin, Cout=cout, ksize=k, stride=stride, pad=1, upsample=up, Ho=ho, Wo=wo,
              out_scale=1.0, splitk=splitk)
    if operand == "residual":
        kw.update(residual=16)
    elif operand == "row_add":
        kw.update(row_add=16)
    elif operand == "gn_silu":
        kw.update(gn_ab=16, gn_silu=1, gn_batch=n)
    elif operand == "concat":                                          # both halves multiples of 64
        c1 = cin // 128 * 64
        kw.update(C1=c1, C2=cin - c1, x2=16)
    return ConvDesc(**kw)


def _branches(m, cin, cout, k, stride, rows_per_image, tile3, pick):
    """the branches of tests/splitk_rule_ref.py a launch takes, from the conditions alone, checked against the pick they lead to"""
    kt = (9 if k == 3 else 1) * (cin // 64)
    tiles = math.ceil(m / 64) * math.ceil(cout / (160 if cout % 160 == 0 else 128))
    if k == 3 and stride == 2:
        reached = tiles * pick >= 1024
        return ["strided reached" if reached else "strided fallback"]
    if tiles >= 512:
        assert pick == 1
        return ["tiles >= 512"]
    if kt < 64 and (m >= 2048 or kt < 32):
        assert pick == 1
        return ["short-K exit"]
    if not tile3 and m >= 2048 and kt < 128:
        assert pick == 1
        return ["1x1 m >= 2048, kt < 128"]
    big = tile3 and rows_per_image >= 1024
    target = 256 if big or m < 2048 else 1024
    reached = tiles * pick >= target
    return ["tile kernel big-map target"] * big + [f"target {target} reached" if reached else "general fallback"]


@pytest.fixture(scope="module")
def auto_grid(ops):
    """One sweep of the grid: for every descriptor the library accepts at split 1, the frozen rule's pick against what the
    library reports under DC_SPLITK_AUTO.  -> (counters, branch counts, refused-at-pick cases, disagreements)"""
    from diffcodec_amd import lib
    so = lib.load()
    count, branch, refused, wrong = collections.Counter(), collections.Counter(), [], []
    for case in itertools.product(GRID_N, GRID_MAPS, GRID_CIN, GRID_COUT, GRID_FORMS, GRID_OPERANDS):
        n, _, cin, cout, (k, stride, _), _ = case
        d1 = _grid_desc(*case, 1)
        try:
            r1 = ops.conv_route(d1)
        except lib.HipLaunchError:
            count["refused at split 1"] += 1
            continue
        count["accepted at split 1"] += 1
        m, rows = n * d1.Ho * d1.Wo, d1.Ho * d1.Wo
        pick = splitk_rule_ref.pick(m, cin, cout, k, stride, rows, lambda: r1.kernel == "conv3x3_tile")
        for b in _branches(m, cin, cout, k, stride, rows, k == 3 and stride == 1 and r1.kernel == "conv3x3_tile", pick):
            branch[b] += 1
        da, dp = _grid_desc(*case, ops.DC_SPLITK_AUTO), _grid_desc(*case, pick)
        try:
            rp = ops.conv_route(dp)
        except lib.HipLaunchError:                                     # the parent's own pick, refused: the launch now runs unsplit
            refused.append(case)
            rp, dp, pick = r1, d1, 1
        ra = ops.conv_route(da)
        ok = (ra == rp and ra.splitk == pick                           # the same route, and the pick is its own fixpoint
              and ra.kernel == r1.kernel                               # the family of the probe at split 1 is the family launched
              and ops.conv_instance(da) == ops.conv_instance(dp)
              and so.dc_conv_igemm_ws_bytes(da) == so.dc_conv_igemm_ws_bytes(dp) == (m * cout * 4 * pick if pick > 1 else 0)
              and so.dc_conv_gn_part_chunks(da) == so.dc_conv_gn_part_chunks(dp) and (pick == 1 or so.dc_conv_gn_part_chunks(da) == 0))
        if not ok:
            wrong.append((case, pick, tuple(ra), tuple(rp)))
        count["split above 1"] += pick > 1
    return count, branch, refused, wrong


def test_auto_split_is_the_frozen_rule_wherever_the_route_accepts_it(auto_grid):
    """dc_conv_route / dc_conv_instance / dc_conv_igemm_ws_bytes / dc_conv_gn_part_chunks under DC_SPLITK_AUTO equal the same
    queries with the frozen rule's pick explicit (with split 1 where the route refuses that pick), on every accepted descriptor"""
    count, _, _, wrong = auto_grid
    assert not wrong, (len(wrong), wrong[:5])
    assert count["accepted at split 1"] + count["refused at split 1"] == 77760 and count["refused at split 1"] == 6480, count
    assert count["split above 1"] > 0, count


def test_grid_takes_every_branch_of_the_frozen_rule(auto_grid):
    _, branch, _, _ = auto_grid
    assert all(branch[b] > 0 for b in BRANCH_COUNTS), branch
    assert dict(branch) == BRANCH_COUNTS


def test_only_cout_4_is_refused_at_the_frozen_pick(auto_grid):
    """conv_out-like launches (Cout = 4 on the halo-tile kernel) run unsplit only: the frozen rule picked above 1 for them and the
    library refused the launch; under DC_SPLITK_AUTO they run at split 1"""
    _, _, refused, _ = auto_grid
    assert len(refused) == 1310 and {c[3] for c in refused} == {4}, (len(refused), {c[3] for c in refused})


def test_unet_conv_out_runs_unsplit_under_auto(ops):
    """UNet conv_out (320 -> 4, GroupNorm + SiLU on load, fp32 out) on the latents of a 256x256 frame without CFG duplication"""
    d = _grid_desc(1, (8, 8), 320, 4, (3, 1, 0), "gn_silu", ops.DC_SPLITK_AUTO)
    d.out_f32 = 1
    r = ops.conv_route(d)
    assert (r.kernel, r.splitk) == ("conv3x3_tile", 1), r
    assert splitk_rule_ref.pick(64, 320, 4, 3, 1, 64, lambda: True) == 5


@pytest.mark.parametrize("splitk", [0, -2])
def test_other_values_below_one_still_mean_one(ops, splitk):
    from diffcodec_amd import lib
    case = (1, (8, 8), 1280, 1280, (3, 1, 0), "plain")
    one, d = _grid_desc(*case, 1), _grid_desc(*case, splitk)
    assert ops.conv_route(d) == ops.conv_route(one) and ops.conv_route(_grid_desc(*case, ops.DC_SPLITK_AUTO)).splitk == 20
    assert ops.conv_instance(d) == ops.conv_instance(one)
    assert lib.load().dc_conv_igemm_ws_bytes(d) == 0 and lib.load().dc_conv_gn_part_chunks(d) == lib.load().dc_conv_gn_part_chunks(one)


def test_auto_is_the_header_s_constant(ops):
    src = open(os.path.join(ROOT, "include", "diffcodec_hip.h")).read()
    assert int(re.search(r"#define DC_SPLITK_AUTO \((-?\d+)\)", src).group(1)) == ops.DC_SPLITK_AUTO


def test_conv_plan_of_a_picked_split_routes_as_its_descriptor(ops):
    """every edge case again with splitk=None, the library's pick (what ops.conv and ops.linear ask by default): the split in the plan's
    descriptor is explicit and the one the route of the final descriptor (slabs, finalize-first scratch, GroupNorm partials set)
    accepts, and the slabs are asked for exactly when it splits"""
    import dataclasses
    picked = set()
    for c in E.CONV_CASES:
        p = E.case_plan(dataclasses.replace(c, splitk=None))
        r = ops.conv_route(p.desc)
        assert p.desc.splitk == r.splitk >= 1 and bool(p.desc.splitk_ws) == (r.splitk > 1) == ("splitk" in dict(p.scratch)), c.label()
        picked.add(r.splitk)
    assert len(picked) > 2, picked
