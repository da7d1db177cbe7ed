"""CPU: what is specific to the train family (include/diffcodec_train_hip.h, lib.TRAIN_SIGNATURES; tests/test_abi.py holds the pair
to its header and to the built library, and keeps the five names out of the other families): its name set; every launcher has a
literal lib.call in tests/test_gpu_conv_grad.py or in diffcodec_amd/train.py; the size query refuses bad shapes and grows as its
header says; the routing: the production layers take the MFMA form for both gradients, the query refuses what the launch refuses,
and the case table of tests/conv_grad_ref.py reaches every instance the route can choose at batch 2 and at batch 3; and the module
surface of diffcodec_amd.train."""
import ctypes

import pytest
import torch

import abi_check as A
import conv_grad_ref as R

NAMES = ("dc_silu_grad_f32", "dc_conv3x3_f32_dgrad", "dc_conv3x3_f32_wgrad", "dc_conv3x3_f32_wgrad_ws_bytes", "dc_conv3x3_f32_grad_route")
QUERIES = ("dc_conv3x3_f32_wgrad_ws_bytes", "dc_conv3x3_f32_grad_route")


@pytest.fixture(scope="module")
def lib():
    return A.built_lib()


# ------------------------------------------------------------------------------------------ names and census
def test_train_names():
    from diffcodec_amd import lib
    assert sorted(lib.TRAIN_SIGNATURES) == sorted(NAMES) and set(QUERIES) <= set(NAMES)


def census(signatures):
    """-> (launchers with no literal lib.call in tests/test_gpu_conv_grad.py or train.py, queries train.py never asks)"""
    from diffcodec_amd import train
    return A.family_census(signatures, QUERIES, A.module_source("test_gpu_conv_grad"), open(train.__file__).read())


def test_every_launcher_is_called_by_the_gpu_tests_or_by_the_product():
    from diffcodec_amd import lib
    assert census(lib.TRAIN_SIGNATURES) == ([], [])
    assert census(dict(lib.TRAIN_SIGNATURES, dc_conv3x3_imaginary=[]))[0] == ["dc_conv3x3_imaginary"]
    tests = A.lib_calls(A.module_source("test_gpu_conv_grad"))
    assert set(NAMES) - set(QUERIES) <= tests                         # the edge tests call every launcher by hand
    from diffcodec_amd import train
    product = open(train.__file__).read()                             # the route is asked through lib.query, the size by its C name
    assert A.lib_calls(product, "query") == {"dc_conv3x3_f32_grad_route"} and "dc_conv3x3_f32_wgrad_ws_bytes(" in product
    assert A.family_census(lib.TRAIN_SIGNATURES, QUERIES, "", "lib.call('dc_conv3x3_f32_grad_route')")[1] == sorted(QUERIES)


# ------------------------------------------------------------------------------------------ the size query
BAD_SHAPES = [(0, 8, 8, 8, 8, 1), (65536, 8, 8, 8, 8, 1), (2, 0, 8, 8, 8, 1), (2, 65536, 8, 8, 8, 1), (2, 8, 0, 8, 8, 1), (2, 8, 8, 0, 8, 1),
              (2, 8, 16385, 8, 8, 1), (2, 8, 16384, 16385, 8, 1), (2, 8, 16384, 16384 + 1, 8, 2), (2, 8, 8, 8, 0, 1), (2, 8, 8, 8, 65536, 1),
              (2, 8, 8, 8, 8, 0), (2, 8, 8, 8, 8, 3), (2, 8, 8, 8, 8, 8), (2, 8, 8, 8, 8, -1)]


def test_size_query_refuses_bad_shapes_and_grows_with_the_batch(lib):
    l = lib.load()
    for bad in BAD_SHAPES + [(2, 65535, 8, 8, 65535, 1)]:            # the last one: dw would not fit 32-bit indices
        assert l.dc_conv3x3_f32_wgrad_ws_bytes(*bad) == -1, bad
    for _, cin, h, w, cout, s in R.CASES + [(0,) + p for p in R.PRODUCTION_LAYERS]:
        sizes = [l.dc_conv3x3_f32_wgrad_ws_bytes(n, cin, h, w, cout, s) for n in range(1, 18)]
        assert sizes[0] >= 4 * (cout * cin * 9 + cout)
        for n, (a, b) in enumerate(zip(sizes, sizes[1:]), start=1):
            assert a < b, (cin, h, w, cout, s, n)                      # strictly increasing in N
        assert all(sz <= n * sizes[0] and sz % 4 == 0 for n, sz in enumerate(sizes, start=1))
        # exactly what the route's partition needs: parts x dw, then one bias partial per image
        for n in (1, 2, 3, 9, 17):
            r = _route(lib, "wgrad", (n, cin, h, w, cout, s))
            assert sizes[n - 1] == 4 * (r.groups * r.parts_per_group * cout * cin * 9 + n * cout)


# ------------------------------------------------------------------------------------------ routing
def _route(lib, kind, case):
    from diffcodec_amd import train
    return train.conv3x3_f32_grad_route(kind, *case)


def _key(lib, kind, case):
    r = _route(lib, kind, case)
    return (kind, r.form, r.stride, r.ch_t)


def test_production_layers_take_the_mfma_form_for_both_gradients(lib):
    for layer in R.PRODUCTION_LAYERS:
        assert layer[0] >= 32 and layer[3] >= 32
        for n in (1, 2, 16):
            for kind in ("dgrad", "wgrad"):
                r = _route(lib, kind, (n,) + layer)
                assert r.form == "mfma" and r.stride == layer[4], (kind, n, layer, r)
    for case in R.MFMA_CASES:
        assert _route(lib, "dgrad", case).form == "mfma" and _route(lib, "wgrad", case).form == "mfma", case
    for case in R.GENERIC_CASES:
        assert _route(lib, "dgrad", case).form == "valu" and _route(lib, "wgrad", case).form == "valu", case


def test_query_refuses_what_the_launch_refuses(lib):
    from diffcodec_amd import train
    l = lib.load()
    P = 256                                                          # a non-null pointer nothing reads: the shape is refused first
    info = (ctypes.c_int * 8)()
    for bad in BAD_SHAPES:
        for kind in (0, 1):
            assert l.dc_conv3x3_f32_grad_route(kind, *bad, info) == -1 and list(info) == [0] * 8, bad
        assert l.dc_conv3x3_f32_dgrad(P, P, P, *bad, None) == -1, bad
        n, cin, h, w, cout, s = bad
        assert l.dc_conv3x3_f32_wgrad(P, cin * h * w, P, P, P, P, n, cin, h, w, cout, s, None) == -1, bad
        with pytest.raises(lib.HipLaunchError):
            train.conv3x3_f32_grad_route("dgrad", *bad)
    good = (2, 8, 8, 8, 8, 1)
    assert l.dc_conv3x3_f32_grad_route(2, *good, info) == -1 and l.dc_conv3x3_f32_grad_route(0, *good, None) == -1
    assert l.dc_conv3x3_f32_grad_route(0, *good, info) == 0
    assert l.dc_conv3x3_f32_dgrad(None, P, P, *good, None) == -1 and l.dc_conv3x3_f32_dgrad(P, P, None, *good, None) == -1
    assert l.dc_conv3x3_f32_wgrad(P, 8 * 64 - 1, P, P, P, P, 2, 8, 8, 8, 8, 1, None) == -1          # batch stride below one image
    assert l.dc_conv3x3_f32_wgrad(P, 8 * 64, P, P, P, None, 2, 8, 8, 8, 8, 1, None) == -1           # no workspace
    assert l.dc_conv3x3_f32_wgrad(P, 8 * 64, P, None, P, P, 2, 8, 8, 8, 8, 1, None) == -1
    assert l.dc_silu_grad_f32(P, P, P, 0, None) == -1 and l.dc_silu_grad_f32(None, P, P, 4, None) == -1


def reachable_keys(lib):
    """every instance the route chooses over a sweep of shapes on both sides of each of its rules"""
    keys = set()
    for kind in ("dgrad", "wgrad"):
        for s in (1, 2, 4):
            for cin in (1, 3, 8, 16, 24, 31, 32, 36, 40, 64, 72, 96, 128, 160, 320):
                for cout in (1, 3, 8, 31, 32, 36, 64, 160):
                    for h, w in ((1, 1), (5, 7), (8, 8), (16, 16), (33, 70)):
                        keys.add(_key(lib, kind, (2, cin, h, w, cout, s)))
    return keys


def coverage(lib, cases):
    """-> the (instance, batch) pairs no case of `cases` reaches"""
    have = {(_key(lib, kind, c), c[0]) for c in cases for kind in ("dgrad", "wgrad")}
    return sorted((k, n) for k in reachable_keys(lib) for n in (2, 3) if (k, n) not in have)


def test_case_table_reaches_every_instance_at_batch_2_and_3(lib):
    keys = reachable_keys(lib)
    assert keys == {("dgrad", "mfma", 1, 32), ("dgrad", "mfma", 1, 64), ("dgrad", "mfma", 2, 32), ("dgrad", "mfma", 2, 64),
                    ("dgrad", "valu", 0, 0), ("wgrad", "mfma", 1, 64), ("wgrad", "mfma", 2, 64), ("wgrad", "valu", 0, 0)}
    assert coverage(lib, R.CASES) == []
    # removing a sole case names its instance
    sole = (3, 64, 6, 10, 32, 2)
    assert coverage(lib, [c for c in R.CASES if c != sole]) == [(("dgrad", "mfma", 2, 64), 3)]
    sole = (2, 32, 12, 8, 32, 2)
    assert coverage(lib, [c for c in R.CASES if c != sole]) == [(("dgrad", "mfma", 2, 32), 2)]
    # the table's own notes hold: ragged tiles and three channel tiles; several K parts with a short last one
    r = _route(lib, "wgrad", (3, 32, 48, 48, 32, 1))
    steps = (48 // r.rows_t) * -(-48 // r.cols_t)
    assert r.parts_per_group > 1 and 0 < steps - (r.parts_per_group - 1) * r.steps_per_part < r.steps_per_part
    r = _route(lib, "dgrad", (3, 40, 12, 36, 96, 1))
    assert 36 % r.cols_t and 40 % r.ch_t
    for case in ((2, 40, 6, 20, 40, 1), (3, 32, 10, 34, 160, 2)):      # pixel tiles ragged both ways, at stride 1 and 2
        r = _route(lib, "dgrad", case)
        assert -(-case[3] // case[5]) % r.cols_t and -(-case[2] // case[5]) % r.rows_t, (case, r)


# ------------------------------------------------------------------------------------------ module surface
def test_module_surface(lib):
    from diffcodec_amd import ops, train
    m = train.Conv3x3(5, 7, stride=2, silu=True)
    ref = torch.nn.Conv2d(5, 7, 3, 2, 1)
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == [(k, tuple(v.shape)) for k, v in ref.state_dict().items()]
    m.load_state_dict(ref.state_dict())                                # a slice of a reference checkpoint loads
    assert torch.equal(m.weight, ref.weight) and torch.equal(m.bias, ref.bias)
    assert [n for n, _ in m.named_parameters()] == ["weight", "bias"] and (m.stride, m.silu) == (2, True)
    nb = train.Conv3x3(5, 7, bias=False)
    assert nb.bias is None and list(nb.state_dict()) == ["weight"]
    for bad in (dict(in_ch=0, out_ch=4), dict(in_ch=4, out_ch=0), dict(in_ch=4, out_ch=4, stride=3)):
        with pytest.raises(ValueError):
            train.Conv3x3(**bad)
    pc = ops.PackedConvF32(ref.weight, ref.bias, "cpu")
    p = train.Conv3x3.from_packed(pc, stride=2, silu=True)
    assert p.weight.data_ptr() == pc.w.data_ptr() and p.bias.data_ptr() == pc.bias.data_ptr()
    assert p.weight.requires_grad and (p.in_ch, p.out_ch, p.stride, p.silu) == (5, 7, 2, True)
    before = pc.w.clone()
    with torch.no_grad():
        p.weight.add_(1.0)                                             # an optimiser step is what the inference net reads next
    assert torch.equal(pc.w, before + 1.0)
    assert train.Conv3x3.from_packed(ops.PackedConvF32(ref.weight, None, "cpu")).bias is None
    with pytest.raises(ValueError):
        train.Conv3x3.from_packed(pc, stride=3)
    with pytest.raises(RuntimeError):                                  # no CPU path
        m(torch.zeros(1, 5, 4, 4))
    with pytest.raises(ValueError):
        train.conv3x3_f32(torch.zeros(1, 4, 4, 4), torch.zeros(7, 5, 3, 3))
    with pytest.raises(ValueError):
        train.conv3x3_f32(torch.zeros(1, 5, 4, 4), torch.zeros(7, 5, 3, 3), torch.zeros(6))
