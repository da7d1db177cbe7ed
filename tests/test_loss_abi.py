"""CPU: include/diffcodec_loss_hip.h, lib.LOSS_SIGNATURES and the built library agree, argument kinds included; the first two
headers and tables carry none of the new names; the size queries refuse what the launchers refuse; and a census: every launcher
of LOSS_SIGNATURES has a literal lib.call in tests/test_gpu_losses.py or in diffcodec_amd/losses.py."""
import ast
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUERIES = ("dc_lpips_dgrad_weight_floats", "dc_lpips_keep_ws_bytes", "dc_lpips_train_ws_bytes", "dc_sobel_edge_ws_bytes")


def _symbols(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return src, sorted(set(re.findall(r"\b(dc_[a-z0-9_]+)\s*\(", src)))


def _arg_kinds(src, name):
    """'p' for a pointer parameter, else the scalar type's last word; [] for (void)"""
    decl = re.search(r"\b(?:int|long long)\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S).group(1)
    args = [" ".join(x.split()) for x in decl.split(",")]
    return [] if args == ["void"] else ["p" if "*" in a else a.split()[-2] for a in args]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from diffcodec_amd import lib as l
    if not os.path.exists(l.LIB_PATH):
        g.build()
    return l


def test_loss_header_is_what_the_binding_binds():
    from diffcodec_amd import lib
    src, hdr = _symbols("diffcodec_loss_hip.h")
    assert sorted(lib.LOSS_SIGNATURES) == hdr, set(hdr) ^ set(lib.LOSS_SIGNATURES)
    assert all(n.startswith(("dc_lpips_", "dc_sobel_")) for n in hdr) and len(hdr) == 12
    kind = {lib.vp: "p", lib.i32: "int", lib.i64: "long", lib.f32: "float", lib.f64: "double"}
    for name, args in lib.LOSS_SIGNATURES.items():
        got = [kind.get(a, "p") for a in args]                       # POINTER(...) types are pointers
        assert got == _arg_kinds(src, name), (name, got, _arg_kinds(src, name))


def test_first_two_headers_and_tables_carry_none_of_the_new_names():
    from diffcodec_amd import lib
    new = set(lib.LOSS_SIGNATURES)
    for header in ("diffcodec_hip.h", "diffcodec_flow_hip.h"):
        assert not new & set(_symbols(header)[1]), header
    assert not new & set(lib.SIGNATURES) and not new & set(lib.FLOW_SIGNATURES)


def test_library_exports_the_loss_symbols(lib):
    l = lib.load()
    for name, args in lib.LOSS_SIGNATURES.items():
        assert hasattr(l, name) and getattr(l, name).argtypes == args, name
    for name in QUERIES:
        assert name in lib.LOSS_SIGNATURES


def _lib_calls(source):
    """C names that are the literal first argument of a `lib.call(...)` expression (from the syntax tree)"""
    names = set()
    for node in ast.walk(ast.parse(source)):
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == "call" and \
                isinstance(node.func.value, ast.Name) and node.func.value.id == "lib" and node.args and \
                isinstance(node.args[0], ast.Constant) and isinstance(node.args[0].value, str):
            names.add(node.args[0].value)
    return names


def census(signatures):
    """-> (launchers with no literal lib.call in tests/test_gpu_losses.py or losses.py, queries losses.py never asks)"""
    from diffcodec_amd import losses
    tests = open(os.path.join(ROOT, "tests", "test_gpu_losses.py")).read()
    product = open(losses.__file__).read()
    called = _lib_calls(tests) | _lib_calls(product)
    uncalled = sorted(set(signatures) - set(QUERIES) - called)
    unnamed = sorted(q for q in QUERIES if q in signatures and (q + "(") not in product)
    return uncalled, unnamed


def test_every_launcher_is_called_by_the_gpu_tests_or_by_the_product():
    from diffcodec_amd import lib
    uncalled, unnamed = census(lib.LOSS_SIGNATURES)
    assert not uncalled, f"no literal lib.call in tests/test_gpu_losses.py or losses.py: {uncalled}"
    assert not unnamed, f"losses.py never asks: {unnamed}"
    uncalled, _ = census(dict(lib.LOSS_SIGNATURES, dc_lpips_imaginary=[]))
    assert uncalled == ["dc_lpips_imaginary"]
    stages = {"dc_lpips_tail_grad", "dc_lpips_conv_dgrad", "dc_lpips_pool_grad", "dc_lpips_conv1_dgrad"}
    tests = _lib_calls(open(os.path.join(ROOT, "tests", "test_gpu_losses.py")).read())
    assert stages <= tests, stages - tests                            # the per-stage entries are what the edge tests call


def test_size_queries_and_launchers_refuse_bad_shapes(lib):
    """no GPU needed: every refusal returns -1 before anything is launched"""
    from diffcodec_amd.metrics import lpips_map_sizes
    l = lib.load()
    floats = sum(co * k * k * ci for co, ci, k in ((192, 64, 5), (384, 192, 3), (256, 384, 3), (256, 256, 3)))
    assert l.dc_lpips_dgrad_weight_floats() == floats
    assert l.dc_lpips_keep_ws_bytes(2, 64, 64) == l.dc_lpips_ws_bytes(2, 64, 64) > 0
    assert l.dc_lpips_keep_ws_bytes(2, 30, 64) == -1 and l.dc_lpips_keep_ws_bytes(0, 64, 64) == -1
    for sides, m in ((1, 3), (2, 3), (3, 6)):
        sizes = lpips_map_sizes(67, 95)
        need = sum(m * c * h * w * 4 for c, (h, w) in zip((64, 192, 384, 256, 256), sizes))
        need += m * 64 * sizes[1][0] * sizes[1][1] * 4 + m * 192 * sizes[2][0] * sizes[2][1] * 4
        got = l.dc_lpips_train_ws_bytes(3, 67, 95, sides)
        assert need <= got <= need + 7 * 256, (sides, need, got)
    for bad in ((3, 67, 95, 0), (3, 67, 95, 4), (0, 67, 95, 1), (3, 30, 95, 1), (3, 67, 30, 3)):
        assert l.dc_lpips_train_ws_bytes(*bad) == -1, bad
    P = 256                                                          # a non-null pointer nothing reads: the shape is refused first
    assert l.dc_lpips_alex_keep(P, P, None, 2, 64, 64, 0, P, P, P, None) == -1
    assert l.dc_lpips_alex_backward(P, P, 2, 64, 64, 0, 0, P, P, P, P, P, None) == -1
    assert l.dc_lpips_alex_backward(P, P, 2, 64, 64, 0, 3, P, P, P, P, None, None) == -1
    assert l.dc_lpips_alex_backward(P, P, 2, 30, 64, 0, 1, P, P, P, P, None, None) == -1
    assert l.dc_lpips_tail_grad(5, P, 2, 49, 1, P, P, P, None) == -1 and l.dc_lpips_tail_grad(0, P, 2, 0, 1, P, P, P, None) == -1
    assert l.dc_lpips_conv_dgrad(0, P, 2, 7, 7, P, None, None, P + 4, None) == -1
    assert l.dc_lpips_conv_dgrad(2, P, 2, 7, 7, P, None, None, P, None) == -1         # y must not be gin
    assert l.dc_lpips_pool_grad(P, P, None, 4, 2, 7, P + 4, None) == -1
    assert l.dc_lpips_conv1_dgrad(P, 2, 3, 64, 64, 0, P, P, P, None) == -1 and l.dc_lpips_conv1_dgrad(P, 2, 1, 64, 30, 0, P, P, P, None) == -1
    assert l.dc_sobel_edge_ws_bytes(2, 3, 17, 65) == 2 * 3 * 2 * 2 * 8 and l.dc_sobel_edge_ws_bytes(2, 3, 0, 65) == -1
    assert l.dc_sobel_edge_loss(P, P, None, 2, 3, 17, 65, 1, P, None, P, None) == -1
    assert l.dc_sobel_edge_loss(P, P, (lib.i64 * 8)(), 2, 3, 17, 65, 3, P, P, P, None) == -1
    assert l.dc_sobel_edge_loss(P, P, (lib.i64 * 8)(), 2, 3, 17, 65, 1, None, P, P, None) == -1
    assert l.dc_sobel_edge_grad(P, P, (lib.i64 * 8)(), 2, 3, 17, 65, 2, P, 0, 1.0, P, None) == -1
    assert l.dc_sobel_edge_grad(P, P, (lib.i64 * 8)(), 2, 0, 17, 65, 0, P, 0, 1.0, P, None) == -1


def test_losses_module_surface(lib):
    """the constructor rules need no GPU"""
    from diffcodec_amd import losses
    import lpips_ref
    for kw in (dict(spatial=True), dict(net="vgg"), dict(version="0.0")):
        with pytest.raises(NotImplementedError):
            losses.NormFixLPIPS(**kw)
    m = losses.NormFixLPIPS.from_state_dict(lpips_ref.synth_weights(seed=20), lpips=False)
    assert m.train() is m and m.eval() is m and m.normfix and not m.lpips
    assert bool((m.packed[-sum(lpips_ref.CHANNELS):] == 1).all())          # the unweighted form: lin vectors of ones
    w = lpips_ref.synth_weights(seed=20)["net.slice2.3.weight"]
    d = losses.pack_lpips_dgrad_weights(lpips_ref.synth_weights(seed=20))[:192 * 25 * 64].view(192, 5, 5, 64)
    assert float(d[7, 1, 3, 9]) == float(w[7, 9, 3, 1])                     # [(co, ky, kx)][ci] = w[co][ci][4 - ky][4 - kx]
    with pytest.raises(ValueError):
        losses.SobelEdgeLoss("median")
    with pytest.raises(RuntimeError):
        losses.NormFixLPIPS()._weights(__import__("torch").device("cpu"))
