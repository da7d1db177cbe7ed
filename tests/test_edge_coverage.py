"""CPU: the edge-case tables of tests/edge_cases.py cover every kernel instance the dispatchers can reach, every case routes to the
instance it declares, and the checks the GPU edge tests rely on (guarded buffers, the flat and peaked attention input families held
to oracle/launch_ref.py) reject the faults they are there to catch.  Caller-owned workspaces: E.run_on_fills rejects an overrun, a
read of an unwritten slot and an unwritten output; every dc_*_ws_bytes of the signature tables has a guarding GPU module
(WS_QUERY_TESTS) and grows with N no faster than N; ops.conv_plan asks for the scratch the library states, and plans every conv case
as the launch before the planner was recorded to (tests/golden/conv_plans.json)."""
import functools
import json
import math
import os
import re

import pytest
import torch

import abi_check as A
import edge_cases as E
from oracle import launch_ref as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


@pytest.fixture(scope="module")
def lib():
    return A.built_lib()


# ------------------------------------------------------------------------------------------ conv / linear routes
@pytest.fixture(scope="module")
def conv_keys(lib):
    return E.enumerate_conv_keys()


def uncovered(keys, cases):
    have = {c.key for c in cases}
    return sorted(E.key_str(k) if isinstance(k[0], str) else str(k) for k in keys if k not in have)


def test_conv_grid_spans_the_production_routes(conv_keys):
    """every (route, epi, split-K) triple the decodes launch (tests/golden/shadow_routes.json) is the projection of an enumerated key"""
    proj = {(k[0], k[2], k[3]) for k in conv_keys}
    shadow = json.load(open(os.path.join(ROOT, "tests", "golden", "shadow_routes.json")))
    for batch, routes in shadow.items():
        for kernel, epi, split in routes:
            assert (kernel, epi, split) in proj, (batch, kernel, epi, split)


def test_every_conv_case_targets_an_enumerated_instance(conv_keys):
    """the grid spans every flag the table uses: no case reaches an instance the enumeration misses"""
    extra = sorted({E.key_str(c.key) for c in E.CONV_CASES if c.key not in conv_keys})
    assert not extra, "table instances the descriptor grid does not reach:\n" + "\n".join(extra)


def test_every_conv_instance_has_a_case(conv_keys):
    missing = uncovered(conv_keys, E.CONV_CASES)
    assert not missing, "conv instances without an edge case:\n" + "\n".join(missing)


@pytest.mark.parametrize("i", range(len(E.CONV_CASES)), ids=[c.label() for c in E.CONV_CASES])
def test_conv_case_routes_where_it_declares(lib, i):
    c = E.CONV_CASES[i]
    got = E.conv_key(E.case_plan(c).desc)
    assert got == c.key, f"{c.label()}: declared {E.key_str(c.key)}, routes to {E.key_str(got)}"


def test_removing_a_sole_conv_case_names_its_instance(conv_keys):
    """the coverage check is sharp: dropping any case that is the only one of its instance fails and names that instance"""
    count = {}
    for c in E.CONV_CASES:
        count[c.key] = count.get(c.key, 0) + 1
    sole = [i for i, c in enumerate(E.CONV_CASES) if count[c.key] == 1 and c.key in conv_keys]
    assert sole
    for i in sole:
        cases = E.CONV_CASES[:i] + E.CONV_CASES[i + 1:]
        assert uncovered(conv_keys, cases) == [E.key_str(E.CONV_CASES[i].key)]


# ------------------------------------------------------------------------------------------ attention routes
@pytest.fixture(scope="module")
def attn_keys(lib):
    return E.enumerate_attention_keys()


def test_every_attention_instance_has_a_case(attn_keys):
    assert len(attn_keys) >= 40
    missing = uncovered(attn_keys, E.ATTN_CASES)
    assert not missing, "attention instances without an edge case:\n" + "\n".join(missing)


@pytest.mark.parametrize("i", range(len(E.ATTN_CASES)), ids=[c.label() for c in E.ATTN_CASES])
def test_attention_case_routes_where_it_declares(lib, i):
    c = E.ATTN_CASES[i]
    assert E.attention_key(c.b, c.heads, c.nq, c.nk, c.d) == c.key, c.label()


def test_attention_cases_have_a_query_tail():
    """every case leaves a partial last query block (Nq not a multiple of its instance's workgroup query span)"""
    for c in E.ATTN_CASES:
        assert c.nq % E.attention_query_span(c.key) != 0, c.label()


def test_small_conv_table_spans_both_kernels():
    """dc_conv_small_cin_bf16: the 4-pixel-strip kernel and the per-pixel one, W % 4 != 0, Cout % 8 != 0, stride 2;
    dc_conv_small_cout_bf16: every COUT template with and without GroupNorm on load and fp32 output, M % 4 != 0"""
    cin = [c for c in E.SMALL_CASES if c.kind == "small_cin"]
    assert {c.strip_kernel for c in cin} == {True, False}
    assert any(c.w % 4 for c in cin) and any(c.cout % 8 for c in cin) and any(c.stride == 2 for c in cin)
    cout = {(c.cout, c.gn, c.out_f32) for c in E.SMALL_CASES if c.kind == "small_cout"}
    assert cout >= {(co, gn, f32) for co in (3, 4, 8) for gn in (False, True) for f32 in (False, True)}
    assert all((c.n * c.ho * c.wo) % 4 for c in E.SMALL_CASES if c.kind == "small_cout")


def test_removing_a_sole_attention_case_names_its_instance(attn_keys):
    count = {}
    for c in E.ATTN_CASES:
        count[c.key] = count.get(c.key, 0) + 1
    for i, c in enumerate(E.ATTN_CASES):
        if count[c.key] == 1:
            assert uncovered(attn_keys, E.ATTN_CASES[:i] + E.ATTN_CASES[i + 1:]) == [str(c.key)]


def test_attention_route_refuses_what_the_launch_refuses(lib):
    from diffcodec_amd import ops
    for bad in ((0, 8, 64, 64, 40), (1, 8, 64, 0, 40), (1, 8, 64, 64, 48), (1, 0, 64, 64, 40)):
        with pytest.raises(lib.HipLaunchError):
            ops.attention_route(*bad)


# the attention launches of one denoising step (UNet + ControlNet transformer blocks at 64x64 / 32x32 / 16x16 / 8x8 latents; self
# attention over the map, cross attention over the 77-token text context), at the model batches of the 16-frame (32) and 1-frame (2) legs
def _decode_attention_shapes(batch):
    shapes = set()
    for hw, c in ((4096, 320), (1024, 640), (256, 1280), (64, 1280)):
        d = c // 8
        shapes.add((batch, 8, hw, hw, d))
        shapes.add((batch, 8, hw, 77, d))
    return shapes


@pytest.mark.parametrize("frames,batch", [(16, 32), (1, 2)])
def test_attention_routes_match_the_profiled_instances(lib, frames, batch):
    """hardware witness: the instances the route returns for a decode's attention shapes are the attn_kernel<...> instances a
    profile of that decode on the MI355X recorded (profiles/r04_kernel_stats_frames{16,1}.txt)"""
    prof = open(os.path.join(ROOT, "profiles", f"r04_kernel_stats_frames{frames}.txt")).read()
    seen = set()
    for m in re.finditer(r"attn_kernel<(\d+), (\d+), (true|false), (true|false), (true|false)>", prof):
        d, qb = int(m.group(1)), int(m.group(2))
        seen.add((d, qb) + tuple(int(x == "true") for x in m.group(3, 4, 5)))
    routed = {E.attention_key(*s) for s in _decode_attention_shapes(batch)}
    assert routed == seen, (sorted(routed), sorted(seen))


# ------------------------------------------------------------------------------------------ guarded buffers
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_guard_flags_writes_outside_the_view_and_unwritten_rows(dtype):
    g = E.Guarded((3, 5, 24), dtype, "cpu", pitch=32)
    g.fill(torch.randn(3, 5, 24))
    assert g.bad() == [] and g.unwritten() == 0
    flat = g.base
    for where, idx in (("after", g.guard + 3 * 5 * 32), ("before", g.guard - 1), ("gap", g.guard + 2 * 32 + 24)):
        h = E.Guarded((3, 5, 24), dtype, "cpu", pitch=32)
        h.fill(torch.randn(3, 5, 24))
        h.base[idx] = 1.0
        assert h.bad() and h.bad()[0][0] == where, (where, h.bad())
        with pytest.raises(AssertionError):
            h.assert_intact("out")
    # an output row the kernel never writes stays NaN: L.check rejects it, and the pattern count names it
    o = E.Guarded((4, 8), dtype, "cpu")
    ref = torch.randn(4, 8, dtype=F64)
    o.view[:3] = ref[:3].to(dtype)
    assert o.unwritten() == 8
    assert not L.check(o.view, ref, ref.abs(), dtype)["ok"]
    o.view[3] = ref[3].to(dtype)
    assert L.check(o.view, ref, ref.abs(), dtype)["ok"] and o.bad() == []
    assert flat.numel() == 2 * E.GUARD + 3 * 5 * 32


# ------------------------------------------------------------------------------------------ attention input families
def _attention_masked_wrong(q, k, v, heads, pad_to):
    """fp64 output of a kernel whose padded keys (up to `pad_to`, re-reading the last key) score 0 instead of -inf"""
    b, nq, c = q.shape
    d = c // heads
    nk = k.shape[1]
    idx = torch.clamp(torch.arange(pad_to), max=nk - 1)
    qq = q.to(F64).reshape(b, nq, heads, d).transpose(1, 2)
    kk = k.to(F64)[:, idx].reshape(b, pad_to, heads, d).transpose(1, 2)
    vv = v.to(F64)[:, idx].reshape(b, pad_to, heads, d).transpose(1, 2)
    s = qq @ kk.transpose(2, 3) * d ** -0.5
    s[..., nk:] = 0.0
    return (torch.softmax(s, -1) @ vv).transpose(1, 2).reshape(b * nq, c)


@pytest.mark.parametrize("nk", [65, 1000])
def test_flat_family_rejects_padded_keys_scoring_zero(nk):
    """the flat inputs of the GPU edge tests: padded keys of the ragged last tile that score 0 instead of -inf fail L.check"""
    q, k, v = (t.to(torch.bfloat16) for t in E.attention_inputs("flat", 2, 2, 16, nk, 40, torch.Generator().manual_seed(0)))
    rows = torch.arange(2 * 16)
    r, s = L.attention_ref(q, k, v, 2, rows)
    assert L.check(r.to(torch.bfloat16), r, s, torch.bfloat16)["ok"]
    wrong = _attention_masked_wrong(q, k, v, 2, (nk + 63) // 64 * 64).to(torch.bfloat16)
    v_ = L.check(wrong, r, s, torch.bfloat16)
    assert not v_["ok"], v_


def _attention_no_rescale(q, k, v, heads, tile=64):
    """online softmax whose running max moves but whose earlier accumulations are never rescaled (the stale-max fault)"""
    b, nq, c = q.shape
    d = c // heads
    nk = k.shape[1]
    qq = q.to(F64).reshape(b, nq, heads, d).transpose(1, 2)
    kk = k.to(F64).reshape(b, nk, heads, d).transpose(1, 2)
    vv = v.to(F64).reshape(b, nk, heads, d).transpose(1, 2)
    s = qq @ kk.transpose(2, 3) * d ** -0.5
    m = torch.full(s.shape[:-1] + (1,), -math.inf, dtype=F64)
    acc = torch.zeros(b, heads, nq, d, dtype=F64)
    l = torch.zeros_like(m)
    for t0 in range(0, nk, tile):
        st = s[..., t0:t0 + tile]
        m = torch.maximum(m, st.amax(-1, keepdim=True))
        p = torch.exp(st - m)
        acc = acc + p @ vv[:, :, t0:t0 + tile]
        l = l + p.sum(-1, keepdim=True)
    return (acc / l).transpose(1, 2).reshape(b * nq, c)


@pytest.mark.parametrize("nk", [200, 1000])
def test_peaked_family_rejects_a_stale_running_max(nk):
    """the peaked inputs of the GPU edge tests: a running max that moves without rescaling the earlier tiles fails L.check"""
    heads = 4
    assert any(j >= 64 for j in E.peaked_winners(heads, nk))           # some winner lies past the first tile
    q, k, v = (t.to(torch.bfloat16) for t in E.attention_inputs("peaked", 1, heads, 8, nk, 40, torch.Generator().manual_seed(0)))
    rows = torch.arange(8)
    r, s = L.attention_ref(q, k, v, heads, rows)
    assert L.check(r.to(torch.bfloat16), r, s, torch.bfloat16)["ok"]
    wrong = _attention_no_rescale(q, k, v, heads).to(torch.bfloat16)
    assert not L.check(wrong, r, s, torch.bfloat16)["ok"]


# ------------------------------------------------------------------------------------------ fp32 extractor conv routes
@pytest.fixture(scope="module")
def f32_keys(lib):
    return E.enumerate_f32_conv_keys()


def test_f32_conv_grid_finds_exactly_the_eleven_instances(f32_keys):
    want = {("f32conv", "mfma", s, co, pt) for s in (1, 2) for co, pt in ((64, 64), (64, 128), (32, 128))}
    want |= {("f32conv", "blk", s, 64, 256) for s in (1, 2)} | {("f32conv", "direct", s, 16, 256) for s in (1, 2, 4)}
    assert len(want) == E.F32_CONV_INSTANCES and set(f32_keys) == want, sorted(set(f32_keys) ^ want)


def test_every_f32_conv_instance_has_a_case(f32_keys):
    missing = uncovered(f32_keys, E.F32_CONV_CASES)
    assert not missing, "fp32 conv instances without an edge case:\n" + "\n".join(missing)
    extra = sorted({E.key_str(c.key) for c in E.F32_CONV_CASES if c.key not in f32_keys})
    assert not extra, "table instances the grid does not reach:\n" + "\n".join(extra)


@pytest.mark.parametrize("i", range(len(E.F32_CONV_CASES)), ids=[c.label() for c in E.F32_CONV_CASES])
def test_f32_conv_case_routes_where_it_declares(lib, i):
    c = E.F32_CONV_CASES[i]
    got = E.f32_conv_key(c.cin, c.h, c.w, c.cout, c.stride)
    assert got == c.key, f"{c.label()}: declared {E.key_str(c.key)}, routes to {E.key_str(got)}"


@pytest.mark.parametrize("shape,key,tile", E.F32_CONV_PYRAMID, ids=[str(p[0]) for p in E.F32_CONV_PYRAMID])
def test_f32_conv_pyramid_layers_keep_their_mfma_tiles(lib, shape, key, tile):
    """the extractor pyramid of a 512x512 frame: every many-channel layer stays on the MFMA form, on the tile its comment names"""
    cin, cout, hw, stride = shape
    r = E.f32_conv_route(cin, hw, hw, cout, stride)
    assert E.f32_conv_key(cin, hw, hw, cout, stride) == key and (r.cols_t, r.rows_t) == tile, (shape, r)


def _f32_route_restated(cin, h, w, cout, stride):
    """the routing rule of dc_conv3x3_nchw_f32 restated: (form, stride, co_tile, pixel_tile, cols_t, rows_t)"""
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    if stride in (1, 2) and cin >= 16 and cin % 8 == 0 and cout % 32 == 0 and not (stride == 2 and (h % 2 or w % 2)) and ho * wo >= 64:
        pt = 128 if ho * wo >= 128 else 64
        cols = min(wo, pt)
        if not (pt == 64 and cout % 64) and pt % cols == 0 and wo % cols == 0 and ho % (pt // cols) == 0:
            rows = pt // cols
            if 8 * ((rows - 1) * stride + 3) * ((cols - 1) * stride + 3) <= 26 * 256:
                return ("mfma", stride, 64 if (pt == 64 or cout % 64 == 0) else 32, pt, cols, rows)
    if stride != 4 and cout >= 64 and (wo >= 64 or (wo >= 32 and cout >= 160)):
        return ("blk", stride, 64, 256, 16, 16)
    return ("direct", stride, 16, 256, 16, 16)


def test_f32_conv_route_equals_the_restated_rule(lib):
    """routing did not move: over every table shape, the pyramid and a grid of ragged sizes the query returns what the rule of the
    launcher before the routing function existed (restated above) gives"""
    shapes = [(c.cin, c.h, c.w, c.cout, c.stride) for c in E.F32_CONV_CASES]
    shapes += [(ci, hw, hw, co, s) for (ci, co, hw, s), _, _ in E.F32_CONV_PYRAMID]
    # a 960x512 frame's pyramid levels and tile sizes that are not powers of two
    shapes += [(ci, h, w, co, s) for ci in (3, 16, 24, 160) for co in (32, 64, 160, 320) for s in (1, 2, 4)
               for (h, w) in ((512, 960), (256, 480), (128, 240), (64, 120), (32, 60), (16, 30), (8, 15), (96, 96), (48, 80), (1, 128),
                              (128, 1), (7, 9), (2, 32), (1, 1))]
    for sh in shapes:
        assert tuple(E.f32_conv_route(*sh)) == _f32_route_restated(*sh), sh


def test_removing_a_sole_f32_conv_case_names_its_instance(f32_keys):
    for key in f32_keys:
        cases = [c for c in E.F32_CONV_CASES if c.key != key]
        assert uncovered(f32_keys, cases) == [E.key_str(key)]
    count = {}
    for c in E.F32_CONV_CASES:
        count[c.key] = count.get(c.key, 0) + 1
    for i, c in enumerate(E.F32_CONV_CASES):
        if count[c.key] == 1:
            assert uncovered(f32_keys, E.F32_CONV_CASES[:i] + E.F32_CONV_CASES[i + 1:]) == [E.key_str(c.key)]


def test_f32_conv_route_refuses_what_the_launch_refuses(lib):
    from diffcodec_amd import ops
    for bad in ((16, 8, 8, 64, 3), (16, 8, 8, 64, 0), (0, 8, 8, 64, 1), (-8, 8, 8, 64, 1), (16, 0, 8, 64, 1), (16, 8, 0, 64, 2),
                (16, 8, 8, 0, 4), (16, 8, 8, 64, 8)):
        with pytest.raises(lib.HipLaunchError):
            ops.conv3x3_f32_route(*bad)
        # the launch: its own operand checks pass (non-null pointers, N = 1), the shape is refused before anything is launched
        assert lib.load().dc_conv3x3_nchw_f32(16, 0, 16, 16, 16, 1, *bad[:5], 0, None) == -1, bad
    assert ops.conv3x3_f32_route(16, 8, 8, 64, 1).form == "mfma"


def test_f32_conv_table_spans_the_tile_and_store_edges(lib):
    """the table still holds: MFMA tiles of 1, 8, 16, 64 and 128 columns; an MFMA grid with more than one tile in x, in y and in
    channels at once; blocked cases on the scalar-store arm (Wo % 4 != 0) and with a ragged 16-channel group; Cin off the
    8-channel staging step on the VALU forms; a stride-4 case whose last input row is read; an odd batch per instance"""
    mfma = [(c, E.f32_conv_route(c.cin, c.h, c.w, c.cout, c.stride)) for c in E.F32_CONV_CASES if c.key[1] == "mfma"]
    assert {r.cols_t for _, r in mfma} >= {1, 8, 16, 64, 128}
    assert {(r.cols_t, r.rows_t) for _, r in mfma} >= {(1, 64), (1, 128), (128, 1), (8, 16), (16, 4), (8, 8)}
    assert any(c.wo // r.cols_t > 1 and c.ho // r.rows_t > 1 and c.cout // r.co_tile > 1 for c, r in mfma)
    for s in (1, 2):
        assert any(c.cin // 8 >= 3 for c, r in mfma if c.stride == s)                       # more than the prologue + one chunk
    blk = [c for c in E.F32_CONV_CASES if c.key[1] == "blk"]
    for s in (1, 2):
        b = [c for c in blk if c.stride == s]
        assert any(c.wo % 4 for c in b) and any(c.wo % 4 == 0 for c in b) and any(c.cout % 16 for c in b)
        assert any(c.cin % 8 for c in b) and any(c.wo % 16 or c.ho % 16 for c in b)
    direct = [c for c in E.F32_CONV_CASES if c.key[1] == "direct"]
    assert any(c.cin == 1 for c in direct) and any(c.cout == 1 for c in direct) and any(c.cout % 16 for c in direct)
    s4 = [c for c in direct if c.stride == 4]
    assert s4 and any(c.last_row_read for c in s4) and sum(not c.last_row_read for c in s4) == 2 and any(c.cin % 2 for c in s4)
    assert all(c.last_row_read for c in E.F32_CONV_CASES if c.stride != 4)
    for key in {c.key for c in E.F32_CONV_CASES}:
        assert {c.n for c in E.F32_CONV_CASES if c.key == key} == {2, 3}, key
    assert max(c.m * c.cout for c in E.F32_CONV_CASES) * 4 <= 9 << 20                       # the largest operand stays below 9 MB


# ------------------------------------------------------------------------------------------ fp32 conv: the bound is sharp
def _trunc10(t):
    """fp32 values truncated to 10 mantissa bits (a reduced-precision matrix path)"""
    return (t.view(torch.int32) & ~0x1FFF).view(torch.float32)


@pytest.mark.parametrize("i", range(len(E.F32_CONV_CASES)), ids=[c.label() for c in E.F32_CONV_CASES])
def test_f32_conv_bound_passes_torch_and_rejects_faults(i):
    """the check the GPU edge test applies (L.conv3x3_nchw_f32_ref + L.check over every output pixel) on this case's own inputs:
    torch's fp32 conv (another accumulation order) passes, and a kernel that truncates its operands to 10 mantissa bits, drops the
    bias, skips the last input channel or skips the last input row fails"""
    import torch.nn.functional as F
    c = E.F32_CONV_CASES[i]
    x, w, b = E.f32_conv_inputs(c, i)
    rows = torch.arange(c.m)
    flat = lambda y: y.permute(0, 2, 3, 1).reshape(c.m, c.cout)
    xc, xr = x.clone(), x.clone()
    xc[:, -1] = 0
    xr[:, :, -1] = 0
    faults = {"10-bit operands": (_trunc10(x), _trunc10(w), b), "no bias": (x, w, None), "last channel skipped": (xc, w, b)}
    if c.last_row_read:
        faults["last row skipped"] = (xr, w, b)
    for silu in (True, False):
        act = F.silu if silu else (lambda t: t)
        r, s = L.conv3x3_nchw_f32_ref(x, w, b, rows, stride=c.stride, silu=silu)
        v = L.check(flat(act(F.conv2d(x, w, b, stride=c.stride, padding=1))), r, s, torch.float32)
        assert v["ok"], (c.label(), silu, v)
        for name, (fx, fw, fb) in faults.items():
            bad = flat(act(F.conv2d(fx, fw, fb, stride=c.stride, padding=1)))
            assert not L.check(bad, r, s, torch.float32)["ok"], (c.label(), silu, name)


# ------------------------------------------------------------------------------------------ control stage and elementwise tables
CONTROL_LAUNCHERS = ("splat_soft", "splat_sum", "occlusion_mask", "flow_resize_normalize", "flow_resize_divide", "fuse_warped")
ELEMENTWISE_LAUNCHERS = ("silu_f32", "add_f32", "lincomb", "f32_to_bf16", "add_bf16", "nchw_f32_to_nhwc_bf16", "nhwc_bf16_to_nchw_f32",
                         "nhwc_f32_to_nchw_f32", "transpose_bf16", "freeu_lowfreq", "freeu_backbone", "timestep_embedding",
                         "embed_tokens", "postprocess_image")
GRID_STRIDE = ("silu_f32", "add_f32", "lincomb", "f32_to_bf16", "add_bf16", "nchw_f32_to_nhwc_bf16", "nhwc_bf16_to_nchw_f32",
               "nhwc_f32_to_nchw_f32")                      # the elementwise kernels that loop over a capped grid


def _elems(name, case):
    if name == "lincomb":
        return case[0]
    if name == "add_bf16":
        return case // 8                                     # eight elements per thread
    return case if isinstance(case, int) else math.prod(case)


def test_control_tables_span_the_shapes_and_families():
    """the tables still hold: H = 1 and W = 1, h != w, an odd batch, every flow and metric family on every shape, one splat past a
    single grid (smooth only, and nothing else that large); the occlusion, resize and fusion tables square and non-square"""
    small = [c for c in E.SPLAT_CASES if c != E.SPLAT_LARGE]
    assert E.SPLAT_LARGE in E.SPLAT_CASES
    n, c, h, w, fam, _ = E.SPLAT_LARGE
    assert n * h * w > E.GRID_ELEMS and fam == "smooth" and E.GRID_ELEMS == 8192 * 256
    assert all(c[0] * c[2] * c[3] <= 4096 for c in small)                                  # collisions stay cheap everywhere else
    for fam in E.FLOW_FAMILIES:
        for mf in E.METRIC_FAMILIES:
            cs = [c for c in small if c[4] == fam and c[5] == mf]
            assert any(c[2] == 1 for c in cs) and any(c[3] == 1 for c in cs) and any(c[2] == c[3] == 1 for c in cs), (fam, mf)
            assert any(c[2] != c[3] and c[2] > 1 and c[3] > 1 for c in cs) and any(c[0] == 3 for c in cs) and any(c[0] % 2 == 0 for c in cs)
            assert any(c[0] * c[1] * c[2] * c[3] > 256 for c in cs), (fam, mf)             # more than one workgroup
    occ = E.OCCLUSION_CASES
    assert any(h == w for _, h, w, _ in occ) and any(h == 1 for _, h, w, _ in occ) and any(w == 1 for _, h, w, _ in occ)
    assert any(h > w > 1 for _, h, w, _ in occ) and any(w > h > 1 for _, h, w, _ in occ) and any(n == 3 for n, _, _, _ in occ)
    assert all(n * h * w <= E.GRID_ELEMS for n, h, w, _ in occ)
    fr = E.FLOW_RESIZE_CASES
    assert any(H != W for _, H, W, _, _ in fr) and any(h != w for _, _, _, h, w in fr) and any(n == 3 for n, *_ in fr)
    assert any(H == W == 1 for _, H, W, _, _ in fr) and any(h > H for _, H, W, h, w in fr) and any(h < H for _, H, W, h, w in fr)
    assert all(h > 1 and w > 1 for _, _, _, h, w in fr) and any(h == 1 and w == 1 for _, _, _, h, w in E.FLOW_RESIZE_DIVIDE_ONLY)
    assert E.FLOW_DIVISORS[0] != E.FLOW_DIVISORS[1]
    fu = E.FUSE_CASES
    assert any(h != w for _, _, h, w in fu) and any(h * w == 1 for _, _, h, w in fu) and any(n == 3 for n, *_ in fu)
    assert any(c == 320 for _, c, _, _ in fu)                                              # the production channel count


def test_elementwise_table_names_every_launcher_and_passes_one_grid():
    assert set(E.ELEMENTWISE_CASES) == set(ELEMENTWISE_LAUNCHERS)
    for name in GRID_STRIDE:
        sizes = [_elems(name, c) for c in E.ELEMENTWISE_CASES[name]]
        assert max(sizes) > E.GRID_ELEMS, name                                             # the second trip of the loop
        assert sum(s > E.GRID_ELEMS for s in sizes) <= (4 if name == "lincomb" else 1) and min(sizes) == 1, name   # large cases stay few
    assert {t for _, t in E.ELEMENTWISE_CASES["lincomb"]} == {1, 2, 3, 4}
    assert {t for n, t in E.ELEMENTWISE_CASES["lincomb"] if n > E.GRID_ELEMS} == {1, 2, 3, 4}
    for n in (1, 255, 257):
        for name in ("silu_f32", "add_f32", "f32_to_bf16"):
            assert n in E.ELEMENTWISE_CASES[name], (name, n)
    assert {-104.0, 104.0, 88.7, -88.7, 20.0, -20.0, 1e-30, -1e-30, 0.0} <= set(E.SILU_SPECIALS) and len(E.SILU_SPECIALS) == 10
    for name in ("nchw_f32_to_nhwc_bf16", "nhwc_bf16_to_nchw_f32", "nhwc_f32_to_nchw_f32"):
        cs = E.ELEMENTWISE_CASES[name]
        assert any(h != w for _, _, h, w in cs) and any(n == 3 for n, *_ in cs) and (1, 1, 1, 1) in cs
    assert any(r % 32 and c % 32 for _, r, c in E.ELEMENTWISE_CASES["transpose_bf16"])
    assert any(h != w for _, h, w, _ in E.ELEMENTWISE_CASES["freeu_lowfreq"])
    assert {c for _, _, c in E.ELEMENTWISE_CASES["freeu_backbone"]} == {16, 80}
    assert any(s > 0 for _, _, s in E.ELEMENTWISE_CASES["timestep_embedding"]) and len(E.TIMESTEP_TABLE) == 4
    emb = E.ELEMENTWISE_CASES["embed_tokens"]
    assert any(c % (128 * 8) for _, _, c, _ in emb) and any(c > 128 * 8 for _, _, c, _ in emb) and any(b == 3 for b, *_ in emb)
    pp = E.ELEMENTWISE_CASES["postprocess_image"]
    assert {(xs, f, u) for *_, xs, f, u in pp} == {(xs, f, u) for xs in (3, 4) for f, u in ((True, False), (False, True), (True, True))}
    x = E.postprocess_input(2, 3, 5, 7, 4)[..., :3]
    assert bool((x < -1).any()) and bool((x > 1).any()) and bool((x == 1).any()) and bool((x == -1).any())


def test_every_control_and_elementwise_launcher_has_an_edge_test():
    """tests/test_gpu_edges.py holds a `lib.call` of every one of them by its C name"""
    from diffcodec_amd import lib as l
    called = A.lib_calls(A.module_source("test_gpu_edges"))
    c_name = {"splat_soft": "dc_splat_soft_f32", "splat_sum": "dc_splat_sum_f32", "occlusion_mask": "dc_occlusion_mask_f32",
              "flow_resize_normalize": "dc_flow_resize_normalize_f32", "flow_resize_divide": "dc_flow_resize_divide_f32",
              "fuse_warped": "dc_fuse_warped_f32", "lincomb": "dc_lincomb4_f32", "freeu_lowfreq": "dc_freeu_lowfreq_nhwc_bf16",
              "freeu_backbone": "dc_freeu_backbone_nhwc_bf16", "timestep_embedding": "dc_timestep_embedding_f32",
              "embed_tokens": "dc_embed_tokens_bf16", "postprocess_image": "dc_postprocess_image"}
    for name in CONTROL_LAUNCHERS + ELEMENTWISE_LAUNCHERS:
        cn = c_name.get(name, "dc_" + name)
        assert cn in l.SIGNATURES, cn
        assert cn in called, f"{cn}: no lib.call in tests/test_gpu_edges.py"


def test_uint8_guard_flags_writes_outside_the_view():
    g = E.Guarded((2, 5, 3), torch.uint8, "cpu")
    assert g.bad() == [] and int((g.view == 0xA5).all())
    g.view.copy_(torch.arange(30, dtype=torch.uint8).reshape(2, 5, 3))
    assert g.bad() == []
    g.base[g.guard + 30] = 7
    assert g.bad() and g.bad()[0][0] == "after"
    with pytest.raises(AssertionError):
        g.assert_intact("u8")


# ------------------------------------------------------------------------------------------ metric tables
def metric_instances():
    """the instances the metric tables must reach: ssim_scale_kernel<T, WS> per window and element type, every level count of the
    MS-SSIM table's weights, both PSNR element types"""
    return ([("ssim", ws, t) for ws in range(1, 16, 2) for t in ("u8", "f32")] + [("ms_ssim", lv) for lv in sorted(E.MS_WEIGHTS)]
            + [("psnr", t) for t in ("u8", "f32")])


def metric_uncovered(ssim, ms, psnr):
    have = {E.ssim_instance(c) for c in ssim} | {("ms_ssim", c.levels) for c in ms} | {("psnr", c.dtype) for c in psnr}
    return [str(k) for k in metric_instances() if k not in have]


def test_every_metric_instance_has_a_case_and_removing_it_names_the_instance():
    assert metric_uncovered(E.SSIM_CASES, E.MS_SSIM_CASES, E.PSNR_CASES) == []
    assert sorted(E.MS_WEIGHTS) == [1, 2, 3, 5, 8] and all(len(w) == k for k, w in E.MS_WEIGHTS.items())
    tables = dict(ssim=E.SSIM_CASES, ms=E.MS_SSIM_CASES, psnr=E.PSNR_CASES)
    key = dict(ssim=E.ssim_instance, ms=lambda c: ("ms_ssim", c.levels), psnr=lambda c: ("psnr", c.dtype))
    soles = 0
    for name, cases in tables.items():
        for k in {key[name](c) for c in cases}:                      # without the cases of an instance, exactly that one is named
            rest = dict(tables, **{name: [c for c in cases if key[name](c) != k]})
            assert metric_uncovered(**rest) == [str(k)]
        count = {}
        for c in cases:
            count[key[name](c)] = count.get(key[name](c), 0) + 1
        for i, c in enumerate(cases):
            if count[key[name](c)] == 1:
                soles += 1
                assert metric_uncovered(**dict(tables, **{name: cases[:i] + cases[i + 1:]})) == [str(key[name](c))]
    assert soles >= 2                                                 # the level counts 1 and 3 have one case each


def test_metric_tables_span_the_tile_loop_stride_and_value_edges():
    """the tables still hold what they were built for (the shapes are the smallest at which each mechanism of csrc/metrics.hip can
    go wrong: 64 x 32 output tiles, 8 rows per wave, 256-wide loops over partials and over N, PSNR rows striding by 64 and columns
    by 256)"""
    ss, ms, ps = E.SSIM_CASES, E.MS_SSIM_CASES, E.PSNR_CASES
    out = lambda c: (c.h - c.ws + 1, c.w - c.ws + 1)
    for ws in range(1, 16, 2):
        for t in ("u8", "f32"):
            mine = [c for c in ss if E.ssim_instance(c) == ("ssim", ws, t)]
            assert any(out(c) == (1, 1) for c in mine), (ws, t)                                   # one output pixel
            assert any(out(c) == (33, 65) and (c.n, c.c) == (3, 2) for c in mine), (ws, t)        # 2 x 2 tiles, the last 1 x 1
    eleven = [c for c in ss if c.ws == 11]
    assert {(32, 64), (8, 20), (9, 65)} <= {out(c) for c in eleven} and any(c.c == 4 for c in eleven)
    assert any((out(c)[1] + 63) // 64 > 256 for c in ss)                                           # the reduce kernel's second trip
    assert any(c.n * c.c > 256 and c.n > 256 for c in ss)                                          # the finalize kernel's second trip
    assert {c.nonneg for c in ss} == {False, True}
    for table in (ss, ms):
        assert {c.form for c in table} == set(E.METRIC_FORMS)
        assert {c.family for c in table} == set(E.METRIC_FAMILIES_ALL)
        assert {c.L for c in table} == {255.0, 1.0} and {c.K for c in table} == {E.K_DEFAULT, E.K_WIDE}
        assert all(c.dtype == "f32" and c.n >= 2 for c in table if c.family == "nan")
        assert all(c.L == 255.0 for c in table if c.dtype == "u8")
        assert all(c.ws >= 3 for c in table if c.family == "anti")                                # ws = 1 has cs = 1 identically
    assert max(c.n * c.c * c.h * c.w for c in ss + ms) == 2 * 3 * 161 * 161                        # nothing above the smallest default-window frame
    shapes = {(c.n, c.c, c.h, c.w, c.ws, c.levels, c.form) for c in ms}
    assert {(3, 2, 33, 35, 3, 5, "u8_nhwc"), (1, 1, 225, 227, 15, 5, "u8_nchw"), (2, 3, 161, 161, 11, 5, "mixed"), (1, 3, 1, 1, 1, 8, "f32_nchw"),
            (2, 1, 129, 2, 1, 8, "u8_nhwc"), (1, 3, 47, 90, 7, 1, "f32_view"), (1, 1, 45, 77, 5, 3, "pitched")} <= shapes
    for hw in ((23, 24), (24, 23), (23, 23), (24, 24)):                                            # every padding parity of the first pool
        assert {c.dtype for c in ms if (c.h, c.w) == hw and c.levels == 2} == {"u8", "f32"}
    from diffcodec_amd import lib as l
    for c in ss + ms:                                                                              # the launcher takes every case
        assert l.load().dc_ssim_ws_bytes(c.n, c.c, c.h, c.w, c.ws, c.levels or 1) > 0, c.label()
    assert {c.c * c.h for c in ps} >= {1, 63, 64, 65, 129} and {c.w for c in ps} >= {1, 255, 256, 257, 513}
    assert all(c.n == 3 for c in ps) and {c.form for c in ps} == set(E.METRIC_FORMS)
    assert {"extremes", "onepixel", "identical"} <= {c.family for c in ps}
    assert any(c.family == "extremes" and c.dtype == "u8" for c in ps)
    labels = [c.label() for c in ss + ms + ps]
    assert len(set(labels)) == len(labels)


def test_metric_refusals_are_refused_by_the_size_query(lib):
    for label, args in E.METRIC_REFUSALS:
        assert lib.load().dc_ssim_ws_bytes(*args) == -1, label
    assert {a[4] for _, a in E.METRIC_REFUSALS} >= {10, 17} and {a[5] for _, a in E.METRIC_REFUSALS} >= {0, 9}
    assert any(a[0] * a[1] == 65536 for _, a in E.METRIC_REFUSALS)
    assert lib.load().dc_psnr_ws_bytes(0) == -1 and lib.load().dc_psnr_ws_bytes(65536) == -1 and lib.load().dc_psnr_ws_bytes(3) == 3 * 512


def test_float64_guard_flags_writes_outside_the_view_and_unwritten_elements():
    g = E.Guarded((7,), torch.float64, "cpu")
    assert g.bad() == [] and g.unwritten() == 7 and bool(torch.isnan(g.base).all())
    g.view[:6] = torch.arange(6, dtype=F64)
    g.view[2] = math.nan                                   # a NaN result is not the pattern
    assert g.unwritten() == 1 and g.bad() == []
    g.view[6] = math.inf
    assert g.unwritten() == 0
    for where, idx in (("before", g.guard - 1), ("after", g.guard + 7)):
        h = E.Guarded((7,), torch.float64, "cpu")
        h.base[idx] = 0.0
        assert h.bad() and h.bad()[0][0] == where
        with pytest.raises(AssertionError):
            h.assert_intact("out")
    h = E.Guarded((7,), torch.float64, "cpu")
    h.base[3] = math.nan                                   # another NaN in a guard element is a write
    assert h.bad() == [("before", 3 - h.guard)]


def test_new_launcher_tables_span_their_edges():
    """FDN modulate: one vector, C off a multiple of 64, Bp in {1, N, a divisor}, exactly one case past the 4096 x 256 cap; the
    .flo resize: H = 1, W = 1, a 1 x 1 and a one-column target, identity, up and down; the pack: one pixel and one case past a
    grid; the blend: every C, a single window, feather 0 and 2 feather = tile, th != tw with four-fold corners, ties and clipping"""
    vec = [n * hw * (c // 8) for n, _, hw, c in E.FDN_CASES]
    assert sum(v > E.FDN_VEC_CAP for v in vec) == 1 and min(vec) == 1 and all(c % 8 == 0 for *_, c in E.FDN_CASES)
    assert any(c % 64 for *_, c in E.FDN_CASES) and any(bp == 1 < n for n, bp, _, _ in E.FDN_CASES)
    assert any(bp == n > 1 for n, bp, _, _ in E.FDN_CASES) and any(n % bp for n, bp, _, _ in E.FDN_CASES)
    fl = E.FLOW_HW2_CASES
    assert any(h == 1 for h, *_ in fl) and any(w == 1 for _, w, _, _ in fl) and (5, 3, 1, 1) in fl and any(tw == 1 < th for _, _, th, tw in fl)
    assert any((h, w) == (th, tw) for h, w, th, tw in fl) and any(th > h and tw > w for h, w, th, tw in fl) and any(th < h for h, w, th, tw in fl)
    assert (1, 1) in E.PACK_CASES and sum(h * w > E.GRID_ELEMS for h, w in E.PACK_CASES) == 1
    bl = E.BLEND_CASES
    assert {c.c for c in bl} == {1, 2, 3, 4} and any(len(c.coords) == 1 and (c.th, c.tw) == (c.h, c.w) for c in bl)
    assert any(c.feather == 0 and len(c.coords) > 1 for c in bl) and any(2 * c.feather == c.th for c in bl)
    assert any(c.th != c.tw and c.h != c.w and len(c.coords) == 9 for c in bl)
    assert any(c.values == "ties" and c.scale == 1.0 and c.feather == 0 for c in bl) and any(c.values == "clip" for c in bl)
    for c in bl:
        cover = torch.zeros(c.h, c.w)
        for (y1, y2, x1, x2) in c.coords:
            assert (y2 - y1, x2 - x1) == (c.th, c.tw) and 0 <= y1 and y2 <= c.h and 0 <= x1 and x2 <= c.w
            cover[y1:y2, x1:x2] += 1
        assert cover.min() >= 1 and (len(c.coords) != 9 or cover.max() == 4), c.name
    t = E.blend_inputs(next(c for c in bl if c.values == "clip"), 0)
    assert bool((t < 0).any()) and bool((t > 1).any())


# ------------------------------------------------------------------------------------------ the census of launchers
_EDGES, _METRICS = "test_gpu_edges", "test_gpu_metrics"
# C name -> (test module, token[, holder]).  token = the C name: the module holds a literal lib.call of it.  Otherwise token = the
# name under which the module reaches a package wrapper, and holder = the package function ("f" or "Class.f") that must hold the
# literal lib.call of the C name.
LAUNCHER_TESTS = {n: (_EDGES, n) for n in (
    "dc_splat_soft_f32", "dc_splat_sum_f32", "dc_occlusion_mask_f32", "dc_flow_resize_normalize_f32", "dc_flow_resize_divide_f32",
    "dc_fuse_warped_f32", "dc_conv3x3_nchw_f32", "dc_nchw_f32_to_nhwc_bf16", "dc_nhwc_bf16_to_nchw_f32", "dc_nhwc_f32_to_nchw_f32",
    "dc_f32_to_bf16", "dc_row_stats_bf16", "dc_ln_finalize", "dc_conv_small_cin_bf16", "dc_conv_small_cout_bf16", "dc_gn_stats_nhwc_bf16",
    "dc_gn_finalize", "dc_gn_direct_nhwc_bf16", "dc_gn_apply_nhwc_bf16", "dc_fdn_modulate_nhwc_bf16", "dc_layernorm_bf16",
    "dc_attention_bf16", "dc_attention_causal_small_bf16", "dc_embed_tokens_bf16", "dc_softmax_rows_f32_to_bf16",
    "dc_timestep_embedding_f32", "dc_freeu_lowfreq_nhwc_bf16", "dc_freeu_backbone_nhwc_bf16", "dc_lincomb4_f32", "dc_transpose_bf16",
    "dc_vae_sample_latents", "dc_silu_f32", "dc_add_bf16", "dc_add_f32", "dc_postprocess_image", "dc_flow_hw2_resize_scale_f32",
    "dc_pack_sixch_u8_f32", "dc_blend_tiles_ramp_u8")}
LAUNCHER_TESTS.update({
    "dc_conv_igemm_bf16": (_EDGES, "conv", "conv"),                       # the descriptor is built by ops.conv
    "dc_cfg_ddim_step": (_EDGES, "cfg_ddim_step", "cfg_ddim_step"),
    "dc_cfg_unipc_step": (_EDGES, "cfg_unipc_step", "cfg_unipc_step"),
    "dc_latents_to_model_input": (_EDGES, "latents_to_model_input", "latents_to_model_input"),
    "dc_ssim": (_METRICS, "dc_ssim"), "dc_ms_ssim": (_METRICS, "dc_ms_ssim"), "dc_psnr": (_METRICS, "dc_psnr"),
    "dc_splat_norm_f32": ("test_gpu_softsplat", "dc_splat_norm_f32"),
    "dc_splat_ingrad_f32": ("test_gpu_softsplat", "dc_splat_ingrad_f32"),
    "dc_splat_flowgrad_f32": ("test_gpu_softsplat", "dc_splat_flowgrad_f32"),
    "dc_resample_u8": ("test_gpu_resample", "dc_resample_u8"),
    "dc_lpips_alex": ("test_gpu_lpips", "LPIPS", "LPIPS.__call__"),
    "dc_lpips_alex_features": ("test_gpu_lpips", "features", "LPIPS.features"),
    "dc_lpips_conv": ("test_gpu_lpips", "dc_lpips_conv"),
    "dc_fid_features": ("test_gpu_fid", "features", "FrechetInceptionDistance.features"),
    "dc_fid_maps": ("test_gpu_fid", "maps", "FrechetInceptionDistance.maps"),
    "dc_fid_conv": ("test_gpu_fid", "dc_fid_conv"),
    "dc_fid_accumulate": ("test_gpu_fid", "update_features", "FrechetInceptionDistance.update_features"),
    "dc_fvd_features": ("test_gpu_fvd", "features", "FrechetVideoDistance.features"),
    "dc_fvd_endpoints": ("test_gpu_fvd", "endpoints", "FrechetVideoDistance.endpoints"),
    "dc_fvd_preprocess": ("test_gpu_fvd", "preprocess", "FrechetVideoDistance.preprocess"),
    "dc_fvd_conv": ("test_gpu_fvd", "dc_fvd_conv"), "dc_fvd_maxpool": ("test_gpu_fvd", "dc_fvd_maxpool"),
})
NOT_LAUNCHERS = ("dc_conv_instance", "dc_gn_stats_chunks", "dc_gemm_row_stats_parts", "dc_conv_gn_part_chunks")


def is_launcher(name):
    return not (name.endswith(("_ws_bytes", "_route", "_weight_floats")) or name in NOT_LAUNCHERS)


@functools.lru_cache(maxsize=None)
def _names_used(path):
    """identifiers and attribute names of a module's syntax tree (a name in a comment or a string does not count)"""
    import ast
    tree = ast.parse(open(path).read())
    return {n.attr for n in ast.walk(tree) if isinstance(n, ast.Attribute)} | {n.id for n in ast.walk(tree) if isinstance(n, ast.Name)}


@functools.lru_cache(maxsize=None)
def _package_holders(cname):
    """the package functions ("f", "Class.f") whose body holds a literal lib.call of `cname`"""
    import ast
    import glob
    from diffcodec_amd import lib as l
    found = set()

    def calls(fn):
        return any(isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and n.func.attr == "call" and n.args and
                   isinstance(n.args[0], ast.Constant) and n.args[0].value == cname for n in ast.walk(fn))

    for path in glob.glob(os.path.join(os.path.dirname(l.__file__), "*.py")):
        tree = ast.parse(open(path).read())
        for node in tree.body:
            if isinstance(node, ast.FunctionDef) and calls(node):
                found.add(node.name)
            if isinstance(node, ast.ClassDef):
                found |= {f"{node.name}.{f.name}" for f in node.body if isinstance(f, ast.FunctionDef) and calls(f)}
    return found


@functools.lru_cache(maxsize=None)
def _literal_calls_in(path):
    return frozenset(A.lib_calls(open(path).read()))


def launcher_census(table):
    """-> the complaints, one per launcher of lib.SIGNATURES whose entry is missing or does not hold"""
    from diffcodec_amd import lib as l
    out = []
    for name in l.SIGNATURES:
        if not is_launcher(name):
            continue
        if name not in table:
            out.append(f"{name}: no entry in LAUNCHER_TESTS")
            continue
        module, token, *holder = table[name]
        path = os.path.join(ROOT, "tests", module + ".py")
        if not os.path.exists(path):
            out.append(f"{name}: tests/{module}.py does not exist")
        elif token == name:
            if name not in _literal_calls_in(path):
                out.append(f"{name}: no literal lib.call in tests/{module}.py")
        elif not holder or holder[0] not in _package_holders(name):
            out.append(f"{name}: the package function {holder[0] if holder else '?'} holds no literal lib.call of it")
        elif token not in _names_used(path):
            out.append(f"{name}: tests/{module}.py never names the wrapper {token}")
    out += [f"{name}: an entry for something that is not a launcher of lib.SIGNATURES" for name in table
            if name not in l.SIGNATURES or not is_launcher(name)]
    return out


def test_every_launcher_of_the_abi_has_a_gpu_test():
    assert launcher_census(LAUNCHER_TESTS) == []


def test_removing_a_census_entry_names_the_launcher():
    from diffcodec_amd import lib as l
    assert sum(is_launcher(n) for n in l.SIGNATURES) == len(LAUNCHER_TESTS)
    for name in LAUNCHER_TESTS:
        rest = {k: v for k, v in LAUNCHER_TESTS.items() if k != name}
        got = launcher_census(rest)
        assert len(got) == 1 and got[0].startswith(name + ":"), (name, got)
    broken = dict(LAUNCHER_TESTS, dc_psnr=("test_gpu_ops", "dc_psnr"), dc_fid_maps=("test_gpu_fid", "maps", "FrechetInceptionDistance.features"),
                  dc_fvd_features=("test_gpu_lpips", "endpoints", "FrechetVideoDistance.features"))
    assert [g.split(":")[0] for g in launcher_census(broken)] == ["dc_psnr", "dc_fid_maps", "dc_fvd_features"]


# ------------------------------------------------------------------------------------------ caller-owned workspaces: the helper
def _past(t, k):
    """element k of the storage counted from the first element of the 1-d view t (k < 0 or >= t.numel(): outside it)"""
    return torch.as_strided(t, (1,), (1,), t.storage_offset() + k)


def _fake(fault=None):
    """a launch on CPU tensors: the workspace's first 8 elements hold a 'map' of the input, the output is 2 x map[:4] (+ one
    element of the workspace nobody wrote, with fault = 'reads')"""
    def launch(ws, outs, prime):
        ws[:8] = 5.0 if prime else 1.0
        outs[0][:] = 2 * ws[:4]
        if fault == "past":
            _past(ws, ws.numel())[0] = 0.0
        elif fault == "before":
            _past(ws, -1)[0] = 0.0
        elif fault == "reads":
            outs[0][3] = outs[0][3] + 0.0 * ws[9]          # a padded tap: "a finite value times 0", true only on fresh memory
        elif fault == "reads_plain":
            outs[0][3] = ws[9]
        elif fault == "unwritten":
            outs[0][2] = torch.tensor(E.NAN_BITS[torch.float32], dtype=torch.int32).view(torch.float32)
        elif fault == "out_past":
            _past(outs[0], 4)[0] = 0.0
    return launch


def test_run_on_fills_passes_an_honest_launch_and_reports_the_unwritten_share():
    (out,), share = E.run_on_fills(_fake(), 64, [((4,), torch.float32)], "honest", device="cpu")
    assert out.tolist() == [2.0] * 4 and share == 0.5
    (out, kept), share = E.run_on_fills(_fake(), 64, [((4,), torch.float32)], "honest", device="cpu", keep=True)
    assert kept[:8].tolist() == [1.0] * 8 and bool(torch.isnan(kept[8:]).all())
    (cnt,), _ = E.run_on_fills(lambda ws, outs, prime: outs[0].fill_(3), 8, [((5,), torch.int32)], "integers", device="cpu", elem=torch.float64)
    assert cnt.dtype == torch.int32 and cnt.tolist() == [3] * 5


@pytest.mark.parametrize("fault,finite,match", [
    ("past", True, r"\[nan\] workspace of 64 bytes: guard elements overwritten.*'after', 16"),
    ("before", True, r"\[nan\] workspace of 64 bytes: guard elements overwritten.*'before', -1"),
    ("out_past", True, r"\[nan\] output 0: guard elements overwritten.*'after', 4"),
    ("reads", True, r"\[nan\] output 0: 1 of 4 elements are not finite"),
    ("reads", False, r"output 0 under the 'zeros' fill differs from the 'nan' fill in 1 of 4 elements"),
    ("reads_plain", False, r"\[nan\] output 0: 1 of 4 elements never written"),
    ("unwritten", True, r"\[nan\] output 0: 1 of 4 elements never written"),
])
def test_run_on_fills_rejects_what_it_exists_to_catch(fault, finite, match):
    with pytest.raises(AssertionError, match=match):
        E.run_on_fills(_fake(fault), 64, [((4,), torch.float32)], "fake", device="cpu", finite=finite)


def test_run_on_fills_rejects_a_stale_read_that_zeros_and_nan_agree_on():
    """an output that takes the sign of a workspace element nobody wrote this launch: NaN and 0 both give 0, the 5.0 a launch on
    other inputs left there does not"""
    def launch(ws, outs, prime):
        if prime:
            ws[:] = 5.0
        ws[:8] = 1.0
        outs[0][:] = 2 * ws[:4]
        outs[0][1] = float(ws[12] > 0)

    with pytest.raises(AssertionError, match="under the 'stale' fill differs"):
        E.run_on_fills(launch, 64, [((4,), torch.float32)], "fake", device="cpu")


def test_run_on_fills_rejects_a_kept_buffer_that_depends_on_the_fill_and_refuses_odd_sizes():
    def launch(ws, outs, prime):
        if prime:
            ws[:] = 5.0
        ws[:8] = 1.0
        ws[4] = ws[12].nan_to_num(0.0) + 1.0                # a kept element that takes what the buffer held
        outs[0][:] = 2.0

    with pytest.raises(AssertionError, match="output 1 under the 'stale' fill differs from the 'nan' fill in 1 of 16"):
        E.run_on_fills(launch, 64, [((4,), torch.float32)], "fake", device="cpu", keep=True)
    for nbytes in (0, -1, 62):
        with pytest.raises(AssertionError, match="dc_\\*_ws_bytes"):
            E.run_on_fills(_fake(), nbytes, [((4,), torch.float32)], "fake", device="cpu")
    with pytest.raises(AssertionError, match="no multiple of 8"):
        E.run_on_fills(_fake(), 60, [((4,), torch.float32)], "fake", device="cpu", elem=torch.float64)


# ------------------------------------------------------------------------------------------ ops.conv's scratch and the library's figure
CONV_QUERIES = ("dc_conv_route", "dc_conv_instance", "dc_conv_gn_part_chunks", "dc_conv_igemm_ws_bytes")


RECORDED_PLANS = json.load(open(os.path.join(ROOT, "tests", "golden", "conv_plans.json")))


def counted_plan(lib, monkeypatch, c, timer):
    """(E.case_plan(c) with lib.TIMER set or not, the library queries it made by name)"""
    counts, real = dict.fromkeys(CONV_QUERIES, 0), lib.load()

    class Counting:
        def __getattr__(self, name):
            counts[name] = counts.get(name, 0) + 1
            return getattr(real, name)

    monkeypatch.setattr(lib, "load", Counting)
    monkeypatch.setattr(lib, "TIMER", object() if timer else None)
    p = E.case_plan(c)
    monkeypatch.undo()
    return p, counts


@pytest.mark.parametrize("i", range(len(E.CONV_CASES)), ids=[c.label() for c in E.CONV_CASES])
def test_conv_plan_is_what_the_launch_was_recorded_to_be(lib, monkeypatch, i):
    """ops.conv_plan against the recording of ops.conv from before the planner (seams patched, host tensors, a stand-in for row_add,
    the timer set; recorded twice, identical): descriptor fields, which pointers are set, the scratches in order with their bytes,
    the output and the timer's meta are equal, and the plan, meta included, makes no more library queries than that launch did.
    Without the timer: no meta, and a route query only where a decision needs one (raw LayerNorm partials; every split is explicit)."""
    c = E.CONV_CASES[i]
    rec = RECORDED_PLANS["cases"][f"{i:03d} {c.label()}"]
    p, counts = counted_plan(lib, monkeypatch, c, timer=True)
    fields, present = E.desc_fields(p.desc)
    assert fields == dict(zip(RECORDED_PLANS["fields"], rec["desc"])), c.label()
    assert present == rec["present"], c.label()
    assert [[what, 4 * math.prod(shape)] for what, shape in p.scratch] == rec["scratch"], c.label()
    assert [list(p.out_shape), str(p.out_dtype).replace("torch.", "")] == rec["out"] and p.m == math.prod(p.out_shape[:3])
    fam, label, flops, nbytes = rec["meta"]
    assert p.meta == (RECORDED_PLANS["families"][fam], label, flops, nbytes), (c.label(), p.meta)
    assert all(counts[q] <= n for q, n in zip(CONV_QUERIES, rec["queries"])), (c.label(), counts, rec["queries"])
    q, untimed = counted_plan(lib, monkeypatch, c, timer=False)
    assert q.meta is None and E.desc_fields(q.desc) == (fields, present) and q.scratch == p.scratch
    assert untimed["dc_conv_route"] == (1 if isinstance(c.ln, int) else 0)
    assert untimed["dc_conv_gn_part_chunks"] == counts["dc_conv_gn_part_chunks"] and untimed["dc_conv_instance"] == 0


@pytest.mark.parametrize("i", E.CONV_SCRATCH_CASES, ids=[E.CONV_CASES[i].label() for i in E.CONV_SCRATCH_CASES])
def test_conv_asks_for_the_scratch_the_library_states(lib, i):
    """ops.conv_plan sizes the split-K workspace itself (splitk x M x Cout floats): pinned here to dc_conv_igemm_ws_bytes of the
    descriptor it built, for every case that is handed a scratch; the (mean, rstd) scratch is M pairs and the GroupNorm partials
    dc_conv_gn_part_chunks x N x Cout pairs, asked for exactly when the route finalizes first / the launch emits them"""
    from diffcodec_amd import ops
    c = E.CONV_CASES[i]
    p = E.case_plan(c)
    d, asked = p.desc, [(what, 4 * math.prod(shape)) for what, shape in p.scratch]
    assert E.conv_key(d) == c.key
    L_ = lib.load()
    r = ops.conv_route(d)
    want = []
    if d.splitk > 1:
        assert d.splitk_ws and r.splitk > 1 and L_.dc_conv_igemm_ws_bytes(d) > 0
        want.append(("splitk", L_.dc_conv_igemm_ws_bytes(d)))
    else:
        assert not d.splitk_ws and L_.dc_conv_igemm_ws_bytes(d) == 0
    if r.ln_first:
        assert d.ln_scratch
        want.append(("ln_scratch", c.m * 2 * 4))
    else:
        assert not d.ln_scratch
    if d.gn_part_out:
        want.append(("gn_part", L_.dc_conv_gn_part_chunks(d) * c.n * c.cout * 2 * 4))
    assert asked == want and want, (c.label(), asked, want)


def test_conv_scratch_cases_are_every_case_that_is_handed_one(lib):
    from diffcodec_amd import ops
    kinds = set()
    for i, c in enumerate(E.CONV_CASES):
        p = E.case_plan(c)
        r = ops.conv_route(p.desc)
        handed = r.splitk > 1 or r.ln_first or bool(p.desc.gn_part_out)
        assert handed == bool(p.scratch) == (i in E.CONV_SCRATCH_CASES), c.label()
        kinds |= {what for what, _ in p.scratch}
    assert kinds == {"splitk", "ln_scratch", "gn_part"}


# ------------------------------------------------------------------------------------------ the census of workspace queries
_HELPER = "run_on_fills"
_OWN_GUARDS = "Guarded"            # the module's own guard code around the workspace, written before the shared helper
# dc_*_ws_bytes -> [(test module, the token it must name: the shared helper or, for the exceptions below, E.Guarded, the launchers
# that consume the workspace and that the module must launch)].  A consumer is a literal lib.call of the C name, or, for
# dc_conv_igemm_bf16, the wrapper that builds its descriptor.
WS_QUERY_TESTS = {
    "dc_ssim_ws_bytes": [("test_gpu_metrics", _HELPER, ("dc_ssim", "dc_ms_ssim"))],
    "dc_psnr_ws_bytes": [("test_gpu_metrics", _HELPER, ("dc_psnr",))],
    "dc_lpips_ws_bytes": [("test_gpu_lpips", _HELPER, ("dc_lpips_alex",))],
    "dc_lpips_features_ws_bytes": [("test_gpu_lpips", _HELPER, ("dc_lpips_alex_features",))],
    "dc_fid_ws_bytes": [("test_gpu_fid", _HELPER, ("dc_fid_features",))],
    "dc_fvd_ws_bytes": [("test_gpu_fvd", _HELPER, ("dc_fvd_features", "dc_fvd_endpoints"))],
    "dc_cmp_ws_bytes": [("test_gpu_cmp", _HELPER, ("dc_cmp_forward", "dc_cmp_flow", "dc_cmp_endpoints"))],
    "dc_lpips_keep_ws_bytes": [("test_gpu_losses", _HELPER, ("dc_lpips_alex_keep", "dc_lpips_alex_backward"))],
    "dc_lpips_train_ws_bytes": [("test_gpu_losses", _HELPER, ("dc_lpips_alex_backward",))],
    "dc_guide_ws_bytes": [("test_gpu_guide_points", _HELPER, ("dc_guide_edge", "dc_guide_edt", "dc_guide_nms", "dc_guide_select",
                                                              "dc_guide_watershed"))],
    "dc_conv3x3_f32_wgrad_ws_bytes": [("test_gpu_conv_grad", _HELPER, ("dc_conv3x3_f32_wgrad",))],
    # through the seam of ops.conv (ops._scratch), handed guarded buffers for every case of E.CONV_SCRATCH_CASES
    "dc_conv_igemm_ws_bytes": [("test_gpu_edges", "CONV_SCRATCH_CASES", ("conv",))],
    # the exceptions: guarded workspaces of the declared size from before the helper
    "dc_splat_ws_bytes": [("test_gpu_edges", _OWN_GUARDS, ("dc_splat_soft_f32", "dc_splat_sum_f32")),
                          ("test_gpu_softsplat", _OWN_GUARDS, ("dc_splat_norm_f32", "dc_splat_ingrad_f32", "dc_splat_flowgrad_f32"))],
    "dc_resample_ws_bytes": [("test_gpu_resample", "guard", ("dc_resample_u8",))],      # guard bytes of its own around obuf and wbuf
    "dc_sobel_edge_ws_bytes": [("test_gpu_losses", _OWN_GUARDS, ("dc_sobel_edge_loss",))],
}
WS_EXCEPTIONS = ("dc_splat_ws_bytes", "dc_resample_ws_bytes", "dc_sobel_edge_ws_bytes", "dc_conv_igemm_ws_bytes")


def ws_census(table, signatures=None):
    """-> the complaints, one per dc_*_ws_bytes of the signature tables (lib.signatures()) whose entry is missing or does not hold"""
    from diffcodec_amd import lib as l
    sigs = l.signatures() if signatures is None else signatures
    out = []
    for name in sigs:
        if not name.endswith("_ws_bytes"):
            continue
        if name not in table:
            out.append(f"{name}: no entry in WS_QUERY_TESTS")
            continue
        for module, token, consumers in table[name]:
            path = os.path.join(ROOT, "tests", module + ".py")
            if not os.path.exists(path):
                out.append(f"{name}: tests/{module}.py does not exist")
                break
            used = _names_used(path)
            if name not in used:
                out.append(f"{name}: tests/{module}.py never names the query")
            elif token not in used:
                out.append(f"{name}: tests/{module}.py never names {token}")
            elif token != _HELPER and name not in WS_EXCEPTIONS:
                out.append(f"{name}: guarded by {token}, not by the shared helper, and not a listed exception")
            else:
                missing = [c for c in consumers if c not in _literal_calls_in(path) and c not in used]
                if not consumers or any(c not in sigs and c != "conv" for c in consumers):
                    out.append(f"{name}: tests/{module}.py is given no consumer of the signature tables")
                elif missing:
                    out.append(f"{name}: tests/{module}.py never launches {', '.join(missing)}")
                else:
                    continue
            break
    out += [f"{name}: an entry for something that is no dc_*_ws_bytes of the signature tables" for name in table
            if name not in sigs or not name.endswith("_ws_bytes")]
    return out


def test_every_workspace_query_has_a_guarding_gpu_test():
    assert ws_census(WS_QUERY_TESTS) == []


def test_removing_a_workspace_census_entry_names_the_query():
    from diffcodec_amd import lib as l
    sigs = l.signatures()
    assert sorted(n for n in sigs if n.endswith("_ws_bytes")) == sorted(WS_QUERY_TESTS)
    for name in WS_QUERY_TESTS:
        got = ws_census({k: v for k, v in WS_QUERY_TESTS.items() if k != name})
        assert len(got) == 1 and got[0].startswith(name + ":"), (name, got)
    got = ws_census(WS_QUERY_TESTS, dict(sigs, dc_new_ws_bytes=[]))                 # a new export without an entry
    assert got == ["dc_new_ws_bytes: no entry in WS_QUERY_TESTS"]
    broken = dict(WS_QUERY_TESTS, dc_fid_ws_bytes=[("test_gpu_fvd", _HELPER, ("dc_fid_features",))],
                  dc_fvd_ws_bytes=[("test_gpu_fvd", _HELPER, ("dc_fvd_features", "dc_fvd_preprocess_none"))],
                  dc_cmp_ws_bytes=[("test_gpu_cmp", _OWN_GUARDS, ("dc_cmp_flow",))],
                  dc_lpips_ws_bytes=[("test_gpu_lpips", _HELPER, ("dc_lpips_alex", "dc_lpips_alex_backward"))])
    assert [g.split(":")[0] for g in ws_census(broken)] == ["dc_lpips_ws_bytes", "dc_fid_ws_bytes", "dc_fvd_ws_bytes", "dc_cmp_ws_bytes"]


# ------------------------------------------------------------------------------------------ the size queries in N
# query -> [arguments with N left out (None)]: the shapes of the GPU workspace tests
WS_IN_N = {
    "dc_lpips_ws_bytes": [(None, 31, 31), (None, 67, 95)],
    "dc_lpips_features_ws_bytes": [(None, 31, 31), (None, 67, 95)],
    "dc_lpips_keep_ws_bytes": [(None, 31, 31), (None, 67, 95)],
    "dc_lpips_train_ws_bytes": [(None, 31, 31, 3)] + [(None, 67, 95, s) for s in (1, 2, 3)],
    "dc_fid_ws_bytes": [(None, 1, 1), (None, 64, 48)],
    "dc_fvd_ws_bytes": [(None, 9, 64, 48), (None, 11, 32, 32)],
    "dc_cmp_ws_bytes": [(a, None, h, w) for a in (0, 1) for h, w in ((64, 88), (72, 64))],
    "dc_guide_ws_bytes": [(None, 37, 53), (None, 24, 801)],
    "dc_ssim_ws_bytes": [(None, 3, 161, 161, 11, 5), (None, 2, 33, 35, 3, 5)],
    "dc_psnr_ws_bytes": [(None,)],
    "dc_splat_ws_bytes": [(None, 7, 9), (None, 24, 40)],
    "dc_resample_ws_bytes": [(None, 37, 53, 3)],
    "dc_sobel_edge_ws_bytes": [(None, 3, 17, 70)],
    "dc_conv3x3_f32_wgrad_ws_bytes": [(None, 32, 48, 48, 32, 1), (None, 64, 6, 10, 32, 2)],     # two of conv_grad_ref.CASES
}


@pytest.mark.parametrize("name", sorted(WS_IN_N))
def test_workspace_sizes_grow_with_n_and_never_faster_than_n(lib, name):
    """strictly increasing in N, and at most N x the size for one item: what _PackedNet._step relies on when it chunks a batch by
    the size for one item"""
    q = getattr(lib.load(), name)
    for args in WS_IN_N[name]:
        size = [q(*[n if a is None else a for a in args]) for n in range(1, 18)]
        assert size[0] > 0, (name, args, size[0])
        for n in range(2, 18):
            assert size[n - 2] < size[n - 1] <= n * size[0], (name, args, n, size[n - 2], size[n - 1], size[0])


# dc_guide_ws_bytes and dc_ssim_ws_bytes round the total up to a granule (256 / 512 bytes), so below one granule per item they
# cannot grow with every N: there the size never shrinks and stays within N x the size for one
WS_BELOW_A_GRANULE = {"dc_guide_ws_bytes": [(None, 1, 1)], "dc_ssim_ws_bytes": [(None, 1, 33, 35, 3, 1), (None, 1, 1, 1, 1, 8)]}


@pytest.mark.parametrize("name", sorted(WS_BELOW_A_GRANULE))
def test_rounded_workspace_sizes_never_shrink_with_n(lib, name):
    q = getattr(lib.load(), name)
    for args in WS_BELOW_A_GRANULE[name]:
        size = [q(*[n if a is None else a for a in args]) for n in range(1, 600)]
        assert size[0] > 0 and size[-1] > size[0], (name, args, size[0], size[-1])
        for n in range(2, 600):
            assert size[n - 2] <= size[n - 1] <= n * size[0], (name, args, n, size[n - 2], size[n - 1], size[0])


def test_every_n_taking_workspace_query_is_held_to_it():
    from diffcodec_amd import lib as l
    queries = {n for n in l.signatures() if n.endswith("_ws_bytes") and n != "dc_conv_igemm_ws_bytes"}
    assert set(WS_IN_N) == queries, f"in WS_IN_N or among the exports, not both: {sorted(set(WS_IN_N) ^ queries)}"
