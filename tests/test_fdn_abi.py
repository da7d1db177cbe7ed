"""CPU: what is specific to the FDN family (include/diffcodec_fdn_hip.h, lib.FDN_SIGNATURES; tests/test_abi.py holds the pair to its
header and to the built library): its name set (no size query: there is no workspace); every launcher has a literal lib.call in
tests/test_gpu_fdn_grad.py or in diffcodec_amd/fdn_train.py; null pointers, C % 32 != 0 and bad sizes and strides are refused before
any launch; and the module surface of diffcodec_amd.fdn_train."""
import pytest
import torch

import abi_check as A

NAMES = ("dc_fdn_f32", "dc_fdn_grad_f32")


@pytest.fixture(scope="module")
def lib():
    return A.built_lib()


def test_fdn_names():
    from diffcodec_amd import lib
    assert sorted(lib.FDN_SIGNATURES) == sorted(NAMES) == A.header_symbols("diffcodec_fdn_hip.h")
    assert all(n.startswith("dc_fdn_") for n in NAMES) and not [n for n in NAMES if n.endswith("_ws_bytes")]
    assert ("diffcodec_fdn_hip.h", lib.FDN_SIGNATURES) in lib.ABI and len(lib.ABI) == 7
    assert not set(NAMES) & set(lib.SIGNATURES)                          # the inference FDN (dc_fdn_modulate_nhwc_bf16) stays where it is
    src = open(A.os.path.join(A.ROOT, "include", "diffcodec_fdn_hip.h")).read()
    assert src.count("control_utils.py:28-34") >= 3                      # the file and each entry cite the reference


def census(signatures):
    from diffcodec_amd import fdn_train
    return A.family_census(signatures, (), A.module_source("test_gpu_fdn_grad"), open(fdn_train.__file__).read())


def test_every_launcher_is_called_by_the_gpu_tests_or_by_the_product():
    from diffcodec_amd import lib, fdn_train
    assert census(lib.FDN_SIGNATURES) == ([], [])
    assert census(dict(lib.FDN_SIGNATURES, dc_fdn_imaginary=[]))[0] == ["dc_fdn_imaginary"]
    assert set(NAMES) <= A.lib_calls(open(fdn_train.__file__).read())                      # the product launches both
    assert set(NAMES) <= A.lib_calls(A.module_source("test_gpu_fdn_grad"))                 # and the GPU tests call each by hand


BAD_SHAPES = [(0, 32, 4, 4), (65536, 32, 4, 4), (2, 0, 4, 4), (2, 48, 4, 4), (2, 31, 4, 4), (2, 33, 4, 4), (2, 65536, 4, 4), (2, 32, 0, 4),
              (2, 32, 4, 0), (2, 32, 16385, 4), (2, 32, 4, 16385), (1, 32, 16384, 16385), (1, 256, 16384, 16384), (-1, 32, 4, 4),
              (2, -32, 4, 4), (2, 32, -4, 4)]


def test_launchers_refuse_null_pointers_bad_shapes_and_strides(lib):
    l = lib.load()
    P = 256                                                          # a non-null pointer nothing reads: the argument is refused first
    good = (2, 64, 4, 4)
    chw = 64 * 4 * 4
    fwd = lambda a, shape=good, gs=chw, bs=chw, eps=1e-5: l.dc_fdn_f32(a[0], a[1], gs, a[2], bs, a[3], a[4], a[5], *shape, eps, None)
    bwd = lambda a, shape=good, gs=chw, ggs=chw: l.dc_fdn_grad_f32(a[0], a[1], a[2], gs, a[3], a[4], a[5], a[6], ggs, *shape, None)
    for bad in BAD_SHAPES:
        assert fwd([P] * 6, bad) == -1 and bwd([P] * 7, bad) == -1, bad
    for i in range(6):                                               # x, gamma, beta, y, mean, rstd
        args = [P] * 6
        args[i] = None
        assert fwd(args) == -1, i
    assert fwd([P] * 6, gs=-1) == -1 and fwd([P] * 6, bs=-1) == -1
    assert fwd([P] * 6, eps=0.0) == -1 and fwd([P] * 6, eps=-1e-5) == -1 and fwd([P] * 6, eps=float("nan")) == -1 and fwd([P] * 6, eps=float("inf")) == -1
    for i in (0, 1, 3, 4):                                           # g, x, mean, rstd
        args = [P] * 7
        args[i] = None
        assert bwd(args) == -1, i
    args = [P] * 7
    args[5] = args[6] = None                                         # no output
    assert bwd(args) == -1
    args = [P] * 7
    args[2] = None                                                   # gamma is read when g_x is wanted
    assert bwd(args) == -1
    assert bwd([P] * 7, gs=-1) == -1 and bwd([P] * 7, ggs=chw - 1) == -1 and bwd([P] * 7, ggs=0) == -1


# ------------------------------------------------------------------------------------------ module surface
def test_module_keys_are_the_reference_checkpoints():
    from diffcodec_amd import fdn_train, weights
    m = fdn_train.FDN(64, 96)
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert got == {"conv_gamma.weight": (64, 96, 3, 3), "conv_gamma.bias": (64,), "conv_beta.weight": (64, 96, 3, 3), "conv_beta.bias": (64,)}
    assert m.conv_gamma.stride == 1 and not m.conv_gamma.silu and m.conv_gamma.weight.any() and all(p.requires_grad for p in m.parameters())
    bound = 1.0 / (96 * 9) ** 0.5                                    # nn.Conv2d's initialisation
    top = float(m.conv_beta.weight.detach().abs().max())
    assert 0.9 * bound < top <= bound
    with pytest.raises(ValueError):
        fdn_train.FDN(48, 48)
    layers = fdn_train.DualFlowControlLayers((64, 64, 128, 128))
    assert [n for n, _ in layers.named_children()] == ["feature_extractor", "fdn64", "fdn32", "fdn16", "fdn08"]
    # a full ControlNet state dict: exactly the feature_extractor.* and fdn* slices load, nothing of the module's own is missing
    spec = weights.controlnet_spec()
    own = {k for k in spec if k.startswith(("feature_extractor.", "fdn"))}
    assert 0 < len(own) < len(spec)
    full = fdn_train.DualFlowControlLayers()
    assert {k: tuple(v.shape) for k, v in full.state_dict().items()} == {k: tuple(spec[k][1]) for k in own}


def test_refusals_on_the_cpu():
    from diffcodec_amd import fdn_train
    x = torch.zeros(1, 32, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        fdn_train.fdn(x, x, x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        fdn_train.FDN(32, 32)(x, x)
    with pytest.raises(ValueError, match="multiple of 32"):
        fdn_train.fdn(torch.zeros(1, 48, 4, 4), torch.zeros(1, 48, 4, 4), torch.zeros(1, 48, 4, 4))
    with pytest.raises(ValueError, match="gamma"):
        fdn_train.fdn(x, torch.zeros(1, 32, 4, 5), x)                # control_utils.py:30
    with pytest.raises(ValueError, match="beta"):
        fdn_train.fdn(x, x, torch.zeros(1, 32, 2, 2))
    with pytest.raises(ValueError):
        fdn_train.fdn(x[0], x[0], x[0])
    with pytest.raises(ValueError, match="eps"):
        fdn_train.fdn(x, x, x, eps=0.0)                              # a constant group would have rstd = inf
    with pytest.raises(ValueError, match="spatial"):
        fdn_train.FDN(32, 32)(x, torch.zeros(1, 32, 8, 8))
    layers = fdn_train.DualFlowControlLayers((32, 32, 32, 32))
    with pytest.raises(TypeError):
        layers.inject(0, x)                                          # no hidden state: the levels are an argument
    with pytest.raises(ValueError):
        layers.inject(5, x, [x] * 4)
    with pytest.raises(ValueError, match="levels"):
        layers.inject(0, x, [x] * 3)
    assert not [k for k in vars(layers) if "level" in k]
