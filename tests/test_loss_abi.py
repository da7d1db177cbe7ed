"""CPU: what is specific to the loss family (include/diffcodec_loss_hip.h, lib.LOSS_SIGNATURES; tests/test_abi.py holds the pair to
its header and to the built library, and keeps the families disjoint): its name set; the size queries refuse what the launchers
refuse; and a census: every launcher of LOSS_SIGNATURES has a literal lib.call in tests/test_gpu_losses.py or in
diffcodec_amd/losses.py."""
import pytest

import abi_check as A

QUERIES = ("dc_lpips_dgrad_weight_floats", "dc_lpips_keep_ws_bytes", "dc_lpips_train_ws_bytes", "dc_sobel_edge_ws_bytes")


@pytest.fixture(scope="module")
def lib():
    return A.built_lib()


def test_loss_names():
    from diffcodec_amd import lib
    assert all(n.startswith(("dc_lpips_", "dc_sobel_")) for n in lib.LOSS_SIGNATURES) and len(lib.LOSS_SIGNATURES) == 12
    assert set(QUERIES) <= set(lib.LOSS_SIGNATURES)


def census(signatures):
    """-> (launchers with no literal lib.call in tests/test_gpu_losses.py or losses.py, queries losses.py never asks)"""
    from diffcodec_amd import losses
    return A.family_census(signatures, QUERIES, A.module_source("test_gpu_losses"), open(losses.__file__).read())


def test_every_launcher_is_called_by_the_gpu_tests_or_by_the_product():
    from diffcodec_amd import lib
    uncalled, unnamed = census(lib.LOSS_SIGNATURES)
    assert not uncalled, f"no literal lib.call in tests/test_gpu_losses.py or losses.py: {uncalled}"
    assert not unnamed, f"losses.py never asks: {unnamed}"
    uncalled, _ = census(dict(lib.LOSS_SIGNATURES, dc_lpips_imaginary=[]))
    assert uncalled == ["dc_lpips_imaginary"]
    stages = {"dc_lpips_tail_grad", "dc_lpips_conv_dgrad", "dc_lpips_pool_grad", "dc_lpips_conv1_dgrad"}
    tests = A.lib_calls(A.module_source("test_gpu_losses"))
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
