"""GPU: full SD-1.5-width decodes (synthetic weights) with every HIP launch checked against its fp64 reference
(tests/launch_shadow.py, oracle/launch_ref.py) at the model batches the benchmark measures, plus the launch-level regression
of the folded LayerNorm's scratch decision."""
import json
import os
import time

import pytest
import torch

from launch_shadow import LaunchShadow
from oracle import launch_ref as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
# (route, epilogue mode, split-K > 1) of the GEMM / conv launches the 16- and 44-frame decodes (model batches 32 and 88) exercised on
# the first hardware run of this test: a dispatcher change that drops one of them fails here; new ones are only reported
ROUTES_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shadow_routes.json")


@pytest.fixture(scope="module")
def sd15():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from diffcodec_amd import weights as W
    from diffcodec_amd.controlnet import HipDualFlowControlNet
    from diffcodec_amd.pipeline import StableDiffusionDualFlowControlNetPipeline
    from diffcodec_amd.scheduler import DDIMScheduler
    from diffcodec_amd.unet import HipUNet2DConditionModel
    from diffcodec_amd.vae import HipAutoencoderKL
    usd, csd, vsd = W.synthesize(W.unet_spec(), 0), W.synthesize(W.controlnet_spec(), 1), W.synthesize(W.vae_spec(), 2)
    pipe = StableDiffusionDualFlowControlNetPipeline(vae=HipAutoencoderKL(vsd), text_encoder=None, tokenizer=None,
                                                     unet=HipUNet2DConditionModel(usd), controlnet=HipDualFlowControlNet(csd),
                                                     scheduler=DDIMScheduler(), safety_checker=None, feature_extractor=None)
    pipe.enable_hip_graphs(False)
    pipe.enable_dual_stream(False)
    return pipe


def _call(frames):
    from diffcodec_amd.synthetic import synth_controls, synth_latents, synth_text
    cond, flow = synth_controls(frames, 512)
    pe, npe = synth_text(frames)
    lat = synth_latents(frames, 512)
    return dict(prompt_embeds=pe, negative_prompt_embeds=npe, controlnet_cond=cond, flow_cond=flow, latents=lat,
                num_inference_steps=2, guidance_scale=4.5, controlnet_conditioning_scale=1.7)


def _shadowed(record, tag, fn):
    t0 = time.time()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    with LaunchShadow(record=record, prefix=f"shadow_{tag}") as sh:
        out = fn()
    torch.cuda.synchronize()
    record(f"shadow_{tag}_seconds", round(time.time() - t0, 1))
    record(f"shadow_{tag}_peak_gb", round(torch.cuda.max_memory_allocated() / 2 ** 30, 2))
    return sh, out


@pytest.mark.parametrize("frames", [1, 11, 16, 44])
def test_every_launch_of_a_decode_matches_fp64(sd15, record, frames):
    """Two DDIM steps (model batch 2 * frames: 2, 22, 32, 88 — the single-frame, GOP-12, default and C3 legs of the benchmark; the
    eager fused loop issues the launches the graphs capture) and the VAE decode of every frame in one call (at 44 frames its last
    up-block holds 5.8 GB, so the sampled rows include the blocks past byte 2^31 and 2^32), each launch against its fp64 reference."""
    sh, out = _shadowed(record, f"f{frames}", lambda: sd15(output_type="pt", **_call(frames)).images)
    if frames in (16, 44):
        record(f"shadow_routes_b{2 * frames}", json.dumps(sorted(list(k) for k in sh.routes() if len(k) == 3)))
    sh.raise_on_failure()
    assert out.shape == (frames, 3, 512, 512) and torch.isfinite(out).all()
    routes = {k[0] for k in sh.stats}
    assert {"gemm_dma", "conv3x3_tile", "igemm", "attention", "group_norm_ab", "conv3x3_nchw_f32"} <= routes, routes
    # the control stage and the loop's entry / exit: flows and reference frames -> control pyramid, latents -> model input, image out
    assert {"splat_soft", "occlusion_mask", "flow_resize_normalize", "fuse_warped", "nchw_f32_to_nhwc_bf16", "latents_to_model_input",
            "postprocess_image"} <= routes, routes
    assert sh.band and all(share <= 0.005 for _, share in sh.band.values()), sh.band
    if frames in (16, 44):                              # model batches 32 and 88: the production 1x1 kernels, coverage pinned
        assert {"gemm_rowpanel", "gemm_wide", "gemm_p8"} <= routes, routes
        seen = sorted(list(k) for k in sh.routes() if len(k) == 3)
        want = json.load(open(ROUTES_GOLDEN))[str(2 * frames)]
        missing = [k for k in want if k not in seen]
        assert not missing, f"model batch {2 * frames}: dispatcher routes no longer exercised: {missing}"
        new = [k for k in seen if k not in want]
        if new:
            record(f"shadow_routes_b{2 * frames}_new", json.dumps(new))


def test_validation_config_unipc_freeu(sd15, record):
    """The validation configuration (UniPC multistep + FreeU s1=0.9, s2=0.2, b1=1.2, b2=1.4) at 16 frames, every launch checked."""
    from diffcodec_amd.scheduler import DDIMScheduler, UniPCMultistepScheduler
    sd15.scheduler = UniPCMultistepScheduler()
    sd15.enable_freeu(s1=0.9, s2=0.2, b1=1.2, b2=1.4)
    try:
        sh, out = _shadowed(record, "unipc_freeu_f16", lambda: sd15(output_type="latent", **_call(16)).images)
    finally:
        sd15.disable_freeu()
        sd15.scheduler = DDIMScheduler()
    sh.raise_on_failure()
    assert torch.isfinite(out).all()
    assert {"freeu_lowfreq", "freeu_backbone"} <= {k[0] for k in sh.stats}


def test_vae_encode(sd15, record):
    """AutoencoderKL.encode of 16 frames at 512x512, every launch checked."""
    x = torch.rand(16, 3, 512, 512, generator=torch.Generator().manual_seed(5)) * 2 - 1
    sh, m = _shadowed(record, "vae_encode_f16", lambda: sd15.vae.encode(x).latent_dist.moments_nhwc)
    sh.raise_on_failure()
    assert m.shape == (16, 64, 64, 8) and torch.isfinite(m.float()).all()
    assert {"igemm", "conv3x3_tile", "small_cin"} <= {k[0] for k in sh.stats}


def test_config4_dual_controlnet(record):
    """The C4 configuration: DualFlowControlNet + ResControlNet (warp_cond) on the two 512x512 windows of a 960x512 frame
    (2 units, model batch 4), every launch checked — including the ResControlNet's fp32 extractor convs."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from diffcodec_amd import weights as W
    from diffcodec_amd.controlnet import HipDualFlowControlNet
    from diffcodec_amd.pipeline import StableDiffusionDualFlowControlNetPipeline
    from diffcodec_amd.rescontrolnet import HipResControlNet
    from diffcodec_amd.scheduler import DDIMScheduler
    from diffcodec_amd.unet import HipUNet2DConditionModel
    from diffcodec_amd.vae import HipAutoencoderKL
    cfg, vcfg = W.SD15_UNET_CONFIG, W.SD15_VAE_CONFIG
    pipe = StableDiffusionDualFlowControlNetPipeline(
        vae=HipAutoencoderKL(W.synthesize(W.vae_spec(vcfg), 2), vcfg, DEV), text_encoder=None, tokenizer=None,
        unet=HipUNet2DConditionModel(W.synthesize(W.unet_spec(cfg), 0), cfg, DEV),
        controlnet=[HipDualFlowControlNet(W.synthesize(W.controlnet_spec(cfg), 1), cfg, DEV),
                    HipResControlNet(W.synthesize(W.rescontrolnet_spec(cfg), 3), cfg, DEV)],
        scheduler=DDIMScheduler(), safety_checker=None, feature_extractor=None)
    pipe.enable_hip_graphs(False)
    pipe.enable_dual_stream(False)
    call = _call(2)
    call["controlnet_conditioning_scale"] = [1.7, 1.0]
    call["warp_cond"] = torch.rand(2, 3, 512, 512, generator=torch.Generator().manual_seed(9))
    sh, img = _shadowed(record, "c4_dual_u2", lambda: pipe(output_type="pt", **call).images)
    sh.raise_on_failure()
    assert img.shape == (2, 3, 512, 512) and torch.isfinite(img).all()
    assert {"conv3x3_nchw_f32", "flow_resize_divide", "add_f32", "splat_soft", "occlusion_mask", "fuse_warped"} <= {k[0] for k in sh.stats}


def test_shadow_does_not_change_results(sd15):
    call = _call(1)
    plain = sd15(output_type="latent", **call).images
    with LaunchShadow() as sh:
        shadowed = sd15(output_type="latent", **call).images
    assert sh.calls > 100
    assert torch.equal(plain, shadowed)


@pytest.mark.parametrize("extra", ["residual", "stats_out", "row_add", "act"])
def test_folded_layernorm_partials_with_a_generic_epilogue(extra):
    """K = 320, M = 65,536 with raw LayerNorm partials and an epilogue the row-panel kernel does not specialise: the dispatcher
    finalizes first into ln_scratch, which ops.conv must allocate (it asks the library's route, not a Python restatement)."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from diffcodec_amd import ops
    m, k, n = 65536, 320, 320
    g = torch.Generator().manual_seed(77)
    x = (torch.randn(1, 1, m, k, generator=g) + 0.5).to(DEV, torch.bfloat16)
    w, b = torch.randn(n, k, generator=g) / 18, torch.randn(n, generator=g) * 0.1
    gamma, beta = 1 + 0.1 * torch.randn(k, generator=g), 0.1 * torch.randn(k, generator=g)
    pc = ops.PackedConv(w, b, DEV, ln=(gamma, beta, 1e-5))
    kw = {}
    if extra == "residual":
        kw["residual"] = torch.randn(1, 1, m, n, generator=g).to(DEV, torch.bfloat16)
    elif extra == "stats_out":
        kw["stats_out"] = torch.empty((m, ops.row_stats_parts(n), 2), device=DEV)
    elif extra == "row_add":
        kw["row_add"] = torch.randn(1, n, generator=g).to(DEV)
    else:
        kw["act"] = 1
    y = ops.linear(x, pc, ln_partials=(ops.row_stats(x), 1e-5), **kw)
    torch.cuda.synchronize()
    rows = L.sample_rows(m)
    r, s = L.conv_ref(x, pc, rows, residual=kw.get("residual"), row_add=kw.get("row_add"), act=kw.get("act", 0))
    v = L.check(y.reshape(m, n)[rows.to(DEV)], r, s, torch.bfloat16)
    assert v["ok"], v
