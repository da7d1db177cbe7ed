"""CPU: what is specific to the pyramid family (include/diffcodec_pyramid_hip.h, lib.PYRAMID_SIGNATURES; tests/test_abi.py holds the
pair to its header and to the built library): its name set (no size query: every intermediate is a named output); every launcher has
a literal lib.call in tests/test_gpu_pyramid_grad.py or in diffcodec_amd/pyramid_train.py; null pointers and bad shapes are refused
before any launch; and the module surface of diffcodec_amd.pyramid_train."""
import pytest
import torch

import abi_check as A

NAMES = ("dc_pyramid_exp_f32", "dc_pyramid_fuse_grad_f32", "dc_pyramid_warp_grad_f32")


@pytest.fixture(scope="module")
def lib():
    return A.built_lib()


def test_pyramid_names():
    from diffcodec_amd import lib
    assert sorted(lib.PYRAMID_SIGNATURES) == sorted(NAMES)
    assert all(n.startswith("dc_pyramid_") for n in NAMES) and not [n for n in NAMES if n.endswith("_ws_bytes")]
    assert ("diffcodec_pyramid_hip.h", lib.PYRAMID_SIGNATURES) in lib.ABI


def census(signatures):
    from diffcodec_amd import pyramid_train
    return A.family_census(signatures, (), A.module_source("test_gpu_pyramid_grad"), open(pyramid_train.__file__).read())


def test_every_launcher_is_called_by_the_gpu_tests_or_by_the_product():
    from diffcodec_amd import lib, pyramid_train
    assert census(lib.PYRAMID_SIGNATURES) == ([], [])
    assert census(dict(lib.PYRAMID_SIGNATURES, dc_pyramid_imaginary=[]))[0] == ["dc_pyramid_imaginary"]
    assert set(NAMES) <= A.lib_calls(open(pyramid_train.__file__).read())                  # the product launches all three
    assert set(NAMES) <= A.lib_calls(A.module_source("test_gpu_pyramid_grad"))             # and the edge tests call each by hand


BAD_SHAPES = [(0, 3, 4, 4), (65536, 3, 4, 4), (2, 0, 4, 4), (2, 65536, 4, 4), (2, 3, 0, 4), (2, 3, 4, 0), (2, 3, 16385, 4), (2, 3, 4, 16385),
              (1, 1, 16384, 16385), (1, 1, 16384 + 1, 16384), (-1, 3, 4, 4), (2, 3, -4, 4)]


def test_launchers_refuse_null_pointers_and_bad_shapes(lib):
    l = lib.load()
    P = 256                                                          # a non-null pointer nothing reads: the argument is refused first
    good = (2, 3, 4, 4)
    assert l.dc_pyramid_exp_f32(None, P, 4, None) == -1 and l.dc_pyramid_exp_f32(P, None, 4, None) == -1
    assert l.dc_pyramid_exp_f32(P, P, 0, None) == -1 and l.dc_pyramid_exp_f32(P, P, -3, None) == -1
    fuse = [P] * 15
    for bad in BAD_SHAPES:
        assert l.dc_pyramid_fuse_grad_f32(*fuse, *bad, None) == -1, bad
        assert l.dc_pyramid_warp_grad_f32(*[P] * 9, *bad, None) == -1, bad
    for i in (0, 1, 2, 3, 4, 5, 6, 9, 10):                            # g, wf, wl, cf, cb, occ_f, occ_b, g_cf, g_cb
        args = list(fuse)
        args[i] = None
        assert l.dc_pyramid_fuse_grad_f32(*args, *good, None) == -1, i
    args = list(fuse)
    args[7] = args[8] = None                                         # neither side wanted
    assert l.dc_pyramid_fuse_grad_f32(*args, *good, None) == -1
    for den, outs in ((7, (11, 12)), (8, (13, 14))):                  # a side's den without one of its outputs
        for o in outs:
            args = list(fuse)
            args[o] = None
            assert l.dc_pyramid_fuse_grad_f32(*args, *good, None) == -1, (den, o)
    for i in (1, 2, 3, 4):                                           # e, flow, g, coef
        args = [P] * 9
        args[i] = None
        assert l.dc_pyramid_warp_grad_f32(*args, *good, None) == -1, i
    args = [P] * 9
    args[7] = args[8] = None                                         # no output
    assert l.dc_pyramid_warp_grad_f32(*args, *good, None) == -1
    for i in (0, 5, 6):                                              # x, gden, g_conf are read when gm is given
        args = [P] * 9
        args[i] = None
        assert l.dc_pyramid_warp_grad_f32(*args, *good, None) == -1, i


# ------------------------------------------------------------------------------------------ module surface
def _reference_keys(inject):
    import pyramid_grad_ref as R
    return {k: tuple(v.shape) for k, v in R.state_dict(inject, 0).items()}


def test_module_keys_and_shapes_are_the_inference_extractors():
    from diffcodec_amd import controlnet, pyramid_train
    import pyramid_grad_ref as R
    inject = (24, 24, 40, 40)
    m = pyramid_train.BiDirFeatureExtractor(inject)
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert got == _reference_keys(inject)
    want = set()
    for side in ("first", "last"):
        want |= {f"{side}_pre_extractor.{i}" for i in (0, 2, 4, 6, 8)} | {f"extractors_{side}.{i}.0" for i in range(4)}
    want |= {f"wrapper.{i}.metric_net.{j}" for i in range(4) for j in (0, 2)} | {f"zero_convs.{i}" for i in range(4)}
    assert set(got) == {k + s for k in want for s in (".weight", ".bias")}
    for i in range(4):                                                # zero_module
        assert not m.zero_convs[i].weight.any() and not m.zero_convs[i].bias.any()
    assert m.first_pre_extractor[0].weight.any() and all(p.requires_grad for p in m.parameters())
    full = pyramid_train.BiDirFeatureExtractor()
    assert tuple(full.zero_convs[3].weight.shape) == (1280, 640, 3, 3) and tuple(full.extractors_first[0][0].weight.shape) == (160, 64, 3, 3)
    # a round trip: the module's state dict is what the inference extractor reads, and a checkpoint slice loads into the module
    sd = R.state_dict(inject, 1)
    m.load_state_dict(sd)
    ext = controlnet.BiDirFeatureExtractor({"feature_extractor." + k: v for k, v in m.state_dict().items()}, "feature_extractor.", "cpu")
    assert torch.equal(ext.zero[2].w, sd["zero_convs.2.weight"]) and torch.equal(ext.metric[1][1].bias, sd["wrapper.1.metric_net.2.bias"])
    assert torch.equal(ext.pre["last"][3].w, sd["last_pre_extractor.6.weight"])
    with pytest.raises(ValueError):
        pyramid_train.BiDirFeatureExtractor((24, 24, 40))


def test_from_inference_shares_storage():
    from diffcodec_amd import controlnet, pyramid_train
    import pyramid_grad_ref as R
    inject = (24, 24, 40, 40)
    sd = R.state_dict(inject, 2)
    ext = controlnet.BiDirFeatureExtractor(sd, "", "cpu")
    m = pyramid_train.BiDirFeatureExtractor.from_inference(ext)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == _reference_keys(inject)
    assert m.zero_convs[1].weight.data_ptr() == ext.zero[1].w.data_ptr()
    assert m.wrapper[3].metric_net[2].bias.data_ptr() == ext.metric[3][1].bias.data_ptr()
    assert m.first_pre_extractor[2].weight.data_ptr() == ext.pre["first"][1].w.data_ptr() and m.first_pre_extractor[2].stride == 2
    assert m.extractors_last[2][0].weight.data_ptr() == ext.ext["last"][2].w.data_ptr() and m.extractors_last[2][0].silu
    before = ext.zero[0].w.clone()
    with torch.no_grad():
        m.zero_convs[0].weight.add_(1.0)                               # an optimiser step is what the inference net reads next
    assert torch.equal(ext.zero[0].w, before + 1.0)


def test_cpu_operands_and_flow_gradients_are_refused():
    from diffcodec_amd import pyramid_train
    m = pyramid_train.BiDirFeatureExtractor((24, 24, 40, 40))
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(torch.zeros(1, 6, 64, 64), torch.zeros(1, 4, 64, 64))
    x, mt, fl, oc = torch.zeros(1, 3, 4, 4), torch.zeros(1, 1, 4, 4), torch.zeros(1, 2, 4, 4), torch.zeros(1, 1, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        pyramid_train.warp_fuse(x, x, mt, mt, fl, fl, oc, oc)
    with pytest.raises(ValueError, match="expected"):
        pyramid_train.warp_fuse(x, x, mt, mt, fl, oc, oc, oc)
    with pytest.raises(ValueError):
        pyramid_train.warp_fuse(x, x[:, :2], mt, mt, fl, fl, oc, oc)
    # a flow or a mask that requires grad is refused before the device is looked at, with a pointer to the differentiable splat
    for which in range(4):
        ts = [fl.clone(), fl.clone(), oc.clone(), oc.clone()]
        ts[which].requires_grad_(True)
        with pytest.raises(ValueError, match="softsplat.softsplat"):
            pyramid_train.warp_fuse(x, x, mt, mt, *ts)
        with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU path"):
            pyramid_train.warp_fuse(x, x, mt, mt, *ts)
    with pytest.raises(ValueError, match="softsplat.softsplat"):
        m(torch.zeros(1, 6, 64, 64), torch.zeros(1, 4, 64, 64, requires_grad=True))
