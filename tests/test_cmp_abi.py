"""CPU: include/diffcodec_flow_hip.h, lib.FLOW_SIGNATURES and the built library agree; the first header and the first table carry
no dc_cmp_ name; and a census: every launcher of FLOW_SIGNATURES is called literally by tests/test_gpu_cmp.py or by a HipCMP
method (or sample_grid), so removing a call names the launcher that lost its cover."""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _symbols(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return src, sorted(set(re.findall(r"\b(dc_[a-z0-9_]+)\s*\(", src)))


def _arg_kinds(src, name):
    """'p' for a pointer parameter, else the scalar type's last word"""
    decl = re.search(r"\b(?:int|long long)\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S).group(1)
    return ["p" if "*" in a else a.split()[-2] for a in (" ".join(x.split()) for x in decl.split(","))]


def test_flow_header_is_what_the_binding_binds():
    from diffcodec_amd import lib
    src, hdr = _symbols("diffcodec_flow_hip.h")
    assert sorted(lib.FLOW_SIGNATURES) == hdr, set(hdr) ^ set(lib.FLOW_SIGNATURES)
    assert all(n.startswith("dc_cmp_") for n in hdr) and len(hdr) >= 6
    kind = {lib.vp: "p", lib.i32: "int", lib.i64: "long", lib.f32: "float", lib.f64: "double"}
    for name, args in lib.FLOW_SIGNATURES.items():
        want = _arg_kinds(src, name)
        got = [kind.get(a, "p") for a in args]                       # POINTER(...) types are pointers
        assert got == want, (name, got, want)


def test_first_header_and_table_are_untouched_by_cmp_names():
    from diffcodec_amd import lib
    _, hdr = _symbols("diffcodec_hip.h")
    assert not [n for n in hdr if n.startswith("dc_cmp_")]
    assert not [n for n in lib.SIGNATURES if n.startswith("dc_cmp_")]
    assert not set(lib.SIGNATURES) & set(lib.FLOW_SIGNATURES)


def test_library_exports_the_flow_symbols():
    import __graft_entry__ as g
    from diffcodec_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        g.build()
    l = lib.load()
    for name in lib.FLOW_SIGNATURES:
        assert hasattr(l, name) and getattr(l, name).argtypes == lib.FLOW_SIGNATURES[name], name


def _covered(text):
    return set(re.findall(r"lib\.call\(\s*\"(dc_cmp_[a-z0-9_]+)\"", text))


QUERIES = ("dc_cmp_ws_bytes", "dc_cmp_weight_floats")               # return a size, not a status: called through lib.load()


def census(signatures):
    """-> launchers with no literal lib.call in tests/test_gpu_cmp.py or in HipCMP / sample_grid, and queries the product never names"""
    from diffcodec_amd import flow_propagation as FP
    tests = open(os.path.join(ROOT, "tests", "test_gpu_cmp.py")).read()
    product = inspect.getsource(FP.HipCMP) + inspect.getsource(FP.sample_grid)
    launchers = set(signatures) - set(QUERIES)
    uncalled = sorted(launchers - _covered(tests) - _covered(product))
    unnamed = sorted(q for q in QUERIES if q in signatures and (q + "(") not in product)
    return uncalled, unnamed


def test_every_launcher_is_called_by_the_gpu_tests_or_by_the_product():
    from diffcodec_amd import lib
    uncalled, unnamed = census(lib.FLOW_SIGNATURES)
    assert not uncalled, f"no literal lib.call in tests/test_gpu_cmp.py or HipCMP / sample_grid: {uncalled}"
    assert not unnamed, f"HipCMP never asks: {unnamed}"
    assert set(QUERIES) <= set(lib.FLOW_SIGNATURES) and len(lib.FLOW_SIGNATURES) == 12


def test_census_names_a_launcher_that_loses_its_cover():
    from diffcodec_amd import lib
    uncalled, _ = census(dict(lib.FLOW_SIGNATURES, dc_cmp_imaginary=[]))
    assert uncalled == ["dc_cmp_imaginary"]


def test_size_queries_refuse_what_the_host_rules_refuse():
    """dc_cmp_ws_bytes is -1 exactly where flow_propagation.stage_sizes raises (no GPU needed: the plan is host arithmetic)"""
    import __graft_entry__ as g
    from diffcodec_amd import lib
    from diffcodec_amd.flow_propagation import conv_table, stage_sizes
    import cmp_ref as R
    if not os.path.exists(lib.LIB_PATH):
        g.build()
    l = lib.load()
    for arch, name in ((0, "skip"), (1, "plain")):
        for h in range(24, 100):
            try:
                stage_sizes(R.CONFIGS[name], h, 64)
                ok = True
            except ValueError:
                ok = False
            assert (l.dc_cmp_ws_bytes(arch, 2, h, 64) > 0) == ok == (l.dc_cmp_ws_bytes(arch, 2, 64, h) > 0), (name, h)
        floats = sum(((ci * k * k + 31) // 32 * 32 + 2) * ((co + 31) // 32 * 32) for _, _, _, ci, co, k in conv_table(R.CONFIGS[name]))
        assert l.dc_cmp_weight_floats(arch, 99) == floats
    assert l.dc_cmp_ws_bytes(0, 2, 68, 64) == -1 and l.dc_cmp_ws_bytes(0, 2, 56, 64) == -1 and l.dc_cmp_ws_bytes(2, 2, 64, 64) == -1
    assert l.dc_cmp_ws_bytes(0, 0, 64, 64) == -1 and l.dc_cmp_weight_floats(0, 113) == -1 and l.dc_cmp_weight_floats(3, 99) == -1
