"""CPU: what is specific to the flow family (include/diffcodec_flow_hip.h, lib.FLOW_SIGNATURES; tests/test_abi.py holds the pair to
its header and to the built library, and keeps dc_cmp_ names out of the other families): its name set, and a census: every launcher
of FLOW_SIGNATURES is called literally by tests/test_gpu_cmp.py or by a HipCMP method (or sample_grid), so removing a call names
the launcher that lost its cover; the size queries refuse what the host rules refuse."""
import inspect

import abi_check as A

QUERIES = ("dc_cmp_ws_bytes", "dc_cmp_weight_floats")               # return a size, not a status: called through lib.load()


def test_flow_names():
    from diffcodec_amd import lib
    assert all(n.startswith("dc_cmp_") for n in lib.FLOW_SIGNATURES) and len(lib.FLOW_SIGNATURES) == 12
    assert set(QUERIES) <= set(lib.FLOW_SIGNATURES)


def census(signatures):
    """-> launchers with no literal lib.call in tests/test_gpu_cmp.py or in HipCMP / sample_grid, and queries the product never names"""
    from diffcodec_amd import flow_propagation as FP
    product = inspect.getsource(FP.HipCMP) + inspect.getsource(FP.sample_grid)
    return A.family_census(signatures, QUERIES, A.module_source("test_gpu_cmp"), product)


def test_every_launcher_is_called_by_the_gpu_tests_or_by_the_product():
    from diffcodec_amd import lib
    uncalled, unnamed = census(lib.FLOW_SIGNATURES)
    assert not uncalled, f"no literal lib.call in tests/test_gpu_cmp.py or HipCMP / sample_grid: {uncalled}"
    assert not unnamed, f"HipCMP never asks: {unnamed}"


def test_census_names_a_launcher_that_loses_its_cover():
    from diffcodec_amd import lib
    uncalled, _ = census(dict(lib.FLOW_SIGNATURES, dc_cmp_imaginary=[]))
    assert uncalled == ["dc_cmp_imaginary"]


def test_size_queries_refuse_what_the_host_rules_refuse():
    """dc_cmp_ws_bytes is -1 exactly where flow_propagation.stage_sizes raises (no GPU needed: the plan is host arithmetic)"""
    from diffcodec_amd.flow_propagation import conv_table, stage_sizes
    import cmp_ref as R
    l = A.built_lib().load()
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
