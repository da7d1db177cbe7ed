"""GPU: the sampling loop of pipeline.py (`__call__`, `_denoise_fused`, `_denoise_generic`) against tests/loop_ref.py.

Per case the device's own control pyramid (`compute_pyramid`) is handed to the fp64 reference and to the bf16 emulation on the CPU;
final latents and image, and every step's latents of the generic loop, sit under 4 x the emulation's own figure (rel_l2 and
max|d| / max|ref|, no element excluded), for the eager fused loop, graphs with one and two steps per graph, two streams and the
generic loop.  What such bars cannot see is held exactly: the fused loop's latents are the bits of the same decode driven by hand
from the package's public step pieces with the step index, keep value and scales of loop_ref's schedule; the timestep and the
coefficient row of every step are loop_ref's as integers and bits; the UniPC table runs the corrector at loop_ref's orders.
Last, the caches (graphs, text context, control pyramid and FDN gamma / beta, scheduler tables, buffer epoch): on one pipeline
with graphs on, a call B after a call A that differs in one thing gives the bits of B on a freshly built pipeline.
No fault is injected on the device: what the bars reject is shown on the CPU (tests/test_loop_ref.py)."""
import pytest
import torch

import block_ref as B
import loop_ref as L
import test_loop_ref as TL

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64 = torch.float64
MODES = ("fused", "graphs1", "graphs2", "dual_stream", "generic")
_RIG = {}


# ------------------------------------------------------------------------------------------ pipelines and inputs
def build_pipe(two_nets=False, csd=None):
    from diffcodec_amd.controlnet import HipDualFlowControlNet
    from diffcodec_amd.pipeline import StableDiffusionDualFlowControlNetPipeline
    from diffcodec_amd.rescontrolnet import HipResControlNet
    from diffcodec_amd.scheduler import DDIMScheduler
    from diffcodec_amd.unet import HipUNet2DConditionModel
    from diffcodec_amd.vae import HipAutoencoderKL
    raw = TL.raw_weights()
    ucfg = raw["unet_cfg"]
    cn = HipDualFlowControlNet(raw["cn"][0] if csd is None else csd, ucfg, DEV)
    nets = [cn, HipResControlNet(raw["cn"][1], ucfg, DEV)] if two_nets else cn
    return StableDiffusionDualFlowControlNetPipeline(
        vae=HipAutoencoderKL(raw["vae"], raw["vae_cfg"], DEV), text_encoder=None, tokenizer=None,
        unet=HipUNet2DConditionModel(raw["unet"], ucfg, DEV), controlnet=nets, scheduler=DDIMScheduler(), safety_checker=None,
        feature_extractor=None)


def pipe_for(case):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    two = len(case.opts["scales"]) == 2
    if two not in _RIG:
        _RIG[two] = build_pipe(two)
    return _RIG[two]


def nets_of(pipe):
    return list(pipe.controlnet) if isinstance(pipe.controlnet, (list, tuple)) else [pipe.controlnet]


def call_kw(case, ci):
    """the keywords of `pipe(...)` for a case; the tensors live on the device and are the same objects on every call"""
    o = case.opts
    kw = dict(prompt_embeds=ci["pe"], negative_prompt_embeds=ci["npe"], controlnet_cond=ci["cond"], flow_cond=ci["flow"],
              latents=ci["latents"], num_inference_steps=o["steps"], guidance_scale=o["g"],
              controlnet_conditioning_scale=list(o["scales"]) if len(o["scales"]) > 1 else o["scales"][0],
              control_guidance_start=o["window"][0], control_guidance_end=o["window"][1])
    if ci["warp"] is not None:
        kw["warp_cond"] = ci["warp"]
    return kw


class configured:
    """the scheduler and FreeU state of a case on a pipeline, restored on exit"""

    def __init__(self, pipe, case):
        self.pipe, self.o = pipe, case.opts

    def __enter__(self):
        from diffcodec_amd.scheduler import UniPCMultistepScheduler
        self.saved = self.pipe.scheduler
        if self.o["sched"] == "unipc":
            self.pipe.scheduler = UniPCMultistepScheduler()
        if self.o["freeu"]:
            self.pipe.enable_freeu(**self.o["freeu"])
        return self.pipe

    def __exit__(self, *exc):
        if self.o["freeu"]:
            self.pipe.disable_freeu()
        self.pipe.scheduler = self.saved
        self.pipe.enable_hip_graphs(False)
        self.pipe.enable_dual_stream(False)


def device_setup(case):
    """-> (pipe, device call inputs, loop_ref weights, loop_ref inputs on the DEVICE's pyramids); once per case"""
    k = ("setup", case.name)
    if k not in _RIG:
        pipe = pipe_for(case)
        ci = TL.call_inputs(case)
        dev = {n: (v.to(DEV) if torch.is_tensor(v) else v) for n, v in ci.items()}
        pyrs = [net.compute_pyramid(dev["cond"], dev["flow"], dev["warp"]) for net in nets_of(pipe)]
        torch.cuda.synchronize()
        _RIG[k] = (pipe, dev, TL.loop_weights(len(case.opts["scales"])), TL.loop_inputs(ci, pyrs))
    return _RIG[k]


def run_mode(pipe, case, kw, mode, output_type, trail=None):
    o = case.opts
    extra = {}
    if mode == "generic" or "fused" not in L.loops_of(case):
        def cb(p, i, t, d):
            if trail is not None:
                trail.append((i, int(t), d["latents"].detach().to("cpu", F64)))
            return d
        extra["callback_on_step_end"] = cb
    if o["eta"]:
        extra.update(eta=o["eta"], generator=torch.Generator().manual_seed(TL.ETA_SEED))
    if o["guess"]:
        extra["guess_mode"] = True
    pipe.enable_hip_graphs(mode in ("graphs1", "graphs2", "dual_stream"), steps_per_graph=2 if mode == "graphs2" else 1)
    pipe.enable_dual_stream(mode == "dual_stream")
    return pipe(**kw, **extra, output_type=output_type).images


CASE_MODES = [(c, m) for c in L.LOOP_CASES for m in (MODES if "fused" in L.loops_of(c) else ("generic",))]


# ------------------------------------------------------------------------------------------ the bars
@pytest.mark.parametrize("case,mode", CASE_MODES, ids=[f"{c.name}-{m}" for c, m in CASE_MODES])
def test_loop_against_fp64_under_four_times_the_bf16_emulation(case, mode, record):
    pipe, dev, W, inp = device_setup(case)
    loop = "generic" if mode == "generic" else "fused"
    assert loop in L.loops_of(case)
    rb = L.reference_and_bars(case, W, inp, loop, key="device pyramid")
    kw = call_kw(case, dev)
    trail = []
    with configured(pipe, case):
        lat = run_mode(pipe, case, kw, mode, "latent", trail)
        img = run_mode(pipe, case, kw, mode, "pt")
    outs = dict(latents=lat.detach().to("cpu", F64), image=img.detach().to("cpu", F64))
    if loop == "generic":                                    # every step's latents, through callback_on_step_end
        sched = L.schedule(case.opts)
        assert [(i, t) for i, t, _ in trail] == [(st.index, st.t) for st in sched]
        for i, _, x in trail:
            outs[f"step{i}"] = x
    worst = 0.0
    for name, out in outs.items():
        ref = rb["ref"]["steps"][int(name[4:])] if name.startswith("step") else rb["ref"][name]
        assert out.shape == ref.shape and bool(torch.isfinite(out).all())
        for fig, f, e, bar in zip(("rel_l2", "max_rel"), B.figures(out, ref), rb["emu_figs"][name], rb["bars"][name]):
            print(f"loop/{case.name}/{mode}/{name}/{fig}\tdevice {f:.3e}\temulation {e:.3e}\tbar {bar:.3e}")
            record(f"loop/{case.name}/{mode}/{name}/{fig}", f"{f:.4e}\t{e:.4e}")
            worst = max(worst, f / bar)
    assert worst <= 1.0, worst


# ------------------------------------------------------------------------------------------ exact: the hand-driven chain
def hand_chain(pipe, case, dev):
    """The decode of `_denoise_fused`, driven from the package's public step pieces; which row a step reads, whether each
    ControlNet runs and at what scale come from loop_ref.schedule, not from the pipeline."""
    from diffcodec_amd import ops
    o = case.opts
    unet, nets, sched = pipe.unet, nets_of(pipe), pipe.scheduler
    do_cfg = o["g"] > 1.0
    ctx = (torch.cat([dev["npe"], dev["pe"]], 0) if do_cfg else dev["pe"]).to(device=DEV, dtype=torch.bfloat16).contiguous()
    unet.set_context(ctx)
    for cn in nets:
        cn.set_context(ctx)
        cn.prepare_controls(dev["cond"], dev["flow"], dev["warp"])
    sched.set_timesteps(o["steps"])
    coef, ttab = sched.device_tables(DEV)
    lat = (dev["latents"].to(DEV, torch.float32) * sched.init_noise_sigma).contiguous().clone()
    x_in = ops.latents_to_model_input(lat, 1.0, 2 if do_cfg else 1)
    state = [torch.zeros_like(lat) for _ in range(3)]
    step = torch.zeros(1, device=DEV, dtype=torch.int32)
    fed = []
    for st in L.schedule(o):
        step.fill_(st.index)
        fed.append(ttab[st.index].item())
        control = []
        for cn, sc in zip(nets, st.scales):
            if sc != 0.0:
                feats, midf = cn.forward_nhwc(x_in, ttab, sc, step_dev=step, cfg_shared=do_cfg, features_only=True)
                control.append((feats, midf, cn.zero, cn.zero_mid, sc))
        eps = unet.forward_nhwc(x_in, ttab, step_dev=step, cfg_shared=do_cfg, control=control or None)
        if o["sched"] == "unipc":
            ops.cfg_unipc_step(eps, lat, state[0], state[1], state[2], x_in, coef, step, o["g"] if do_cfg else 1.0, do_cfg)
        else:
            ops.cfg_ddim_step(eps, lat, x_in, coef, step, o["g"] if do_cfg else 1.0, do_cfg)
    torch.cuda.synchronize()
    return lat, fed


FUSED_CASES = [c for c in L.LOOP_CASES if "fused" in L.loops_of(c)]


@pytest.mark.parametrize("case", FUSED_CASES, ids=[c.name for c in FUSED_CASES])
def test_fused_loop_equals_the_hand_driven_chain(case):
    pipe, dev, _, _ = device_setup(case)
    kw = call_kw(case, dev)
    with configured(pipe, case):
        want, fed = hand_chain(pipe, case, dev)
        sched = L.schedule(case.opts)
        assert [float(t) == float(st.t_net) and int(t) == st.t_net for t, st in zip(fed, sched)] == [True] * len(sched), (fed, sched)
        for mode in ("fused", "graphs1", "graphs2", "dual_stream"):
            got = run_mode(pipe, case, kw, mode, "latent")
            assert torch.equal(got, want), (mode, float((got - want).abs().max()))
            if mode != "fused":                              # a second call is pure replay
                assert torch.equal(run_mode(pipe, case, kw, mode, "latent"), want), mode


@pytest.mark.parametrize("case", L.LOOP_CASES, ids=[c.name for c in L.LOOP_CASES])
def test_schedule_rows_and_timesteps_are_loop_ref_s(case):
    """the timestep table as integers and, for DDIM, the coefficient row of every step as bits; the generic loop's callback
    reports the same timesteps (test_loop_against_fp64...)"""
    pipe, dev, _, _ = device_setup(case)
    o = case.opts
    with configured(pipe, case):
        sched = pipe.scheduler
        sched.set_timesteps(o["steps"])
        coef, ttab = sched.device_tables(DEV)
        want = L.schedule(o)
        assert sched.timesteps.tolist() == [st.t for st in want]
        assert ttab.dtype == torch.float32 and ttab.cpu().tolist() == [float(st.t) for st in want]
        assert coef.shape[0] == len(want)
        if o["sched"] == "ddim":
            rows = L.ddim_rows(o)
            assert rows.dtype == coef.dtype == torch.float32 and torch.equal(coef.cpu(), rows)
            assert [st.t for st in L.schedule(o, "steps_offset_dropped")] != [st.t for st in want]


def test_unipc_table_runs_the_corrector_at_loop_ref_s_orders():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from diffcodec_amd.scheduler import UniPCMultistepScheduler
    for steps in (2, 3, 4, 7):
        o = dict(L.CASES["unipc_freeu"].opts, steps=steps)
        s = UniPCMultistepScheduler()
        s.set_timesteps(steps)
        coef = s.device_tables(DEV)[0].cpu()
        assert coef.shape == (steps, s.UNIPC_ROW)
        flags = [int(v) for v in coef[:, 2].tolist()]
        assert flags == L.unipc_flags(o), (steps, flags)
        for i, f in enumerate(flags):
            corr, pred = coef[i, 3:7], coef[i, 7:10]
            assert bool(torch.isfinite(coef[i]).all())
            assert bool((corr[:3] != 0).all()) == bool(f & 1) and bool(corr[3] != 0) == bool(f & 2), (steps, i, corr)
            assert bool(pred[1] != 0) and bool(pred[2] != 0) == bool(f & 4), (steps, i, pred)


# ------------------------------------------------------------------------------------------ call-order independence of the caches
BASE = L.Case("cache_base", dict(L._DEFAULT, steps=3))


class Seq:
    """One transition: a list of (keywords, prepare) calls.  `prepare(pipe)` sets absolute pipeline state (scheduler, FreeU) ahead
    of its call.  Every call after the first is compared with the same call on a freshly built pipeline."""

    def __init__(self):
        ci = TL.call_inputs(BASE)
        self.dev = {n: (v.to(DEV).clone() if torch.is_tensor(v) else v) for n, v in ci.items()}
        self.two = TL.call_inputs(L.Case("cache_b2", dict(BASE.opts, b=2)))
        self.two = {n: (v.to(DEV) if torch.is_tensor(v) else v) for n, v in self.two.items()}

    def kw(self, src=None, **over):
        return dict(call_kw(BASE, src or self.dev), **over)


def _ddim(p):
    from diffcodec_amd.scheduler import DDIMScheduler
    p.scheduler = DDIMScheduler()


def _unipc(p):
    from diffcodec_amd.scheduler import UniPCMultistepScheduler
    p.scheduler = UniPCMultistepScheduler()


def _other(t, seed):
    return torch.randn(t.shape, generator=torch.Generator().manual_seed(seed)).to(t.device, t.dtype)


def transitions():
    def guidance(s):
        return [(s.kw(), None), (s.kw(guidance_scale=3.0), None)]

    def conditioning_scale(s):
        return [(s.kw(), None), (s.kw(controlnet_conditioning_scale=0.9), None)]

    def window(s):
        return [(s.kw(), None), (s.kw(control_guidance_start=0.3, control_guidance_end=0.7), None)]

    def step_count(s):
        return [(s.kw(), None), (s.kw(num_inference_steps=2), None), (s.kw(), None)]

    def batch(s):
        return [(s.kw(), None), (s.kw(s.two), None), (s.kw(), None)]

    def cfg_on_off_on(s):
        return [(s.kw(), None), (s.kw(guidance_scale=1.0), None), (s.kw(), None)]

    def prompt_replaced(s):
        return [(s.kw(), None), (s.kw(prompt_embeds=_other(s.dev["pe"], 5)), None)]

    def prompt_in_place(s):
        return [(s.kw(), None), (s.kw(), lambda p: s.dev["pe"].copy_(_other(s.dev["pe"], 6)))]

    def controls_replaced(s):
        cond, flow = s.dev["cond"].flip(-1).contiguous(), (s.dev["flow"] * 0.5).contiguous()
        return [(s.kw(), None), (s.kw(controlnet_cond=cond, flow_cond=flow), None)]

    def controls_in_place(s):
        def mutate(p):
            s.dev["cond"].copy_(s.dev["cond"].flip(-2).contiguous())
            s.dev["flow"].mul_(0.5)
        return [(s.kw(), None), (s.kw(), mutate)]

    def scheduler_swapped(s):
        return [(s.kw(), _ddim), (s.kw(), _unipc), (s.kw(), _ddim)]

    def freeu_through_pipe(s):
        return [(s.kw(), lambda p: p.disable_freeu()), (s.kw(), lambda p: p.enable_freeu(**L.FREEU)), (s.kw(), lambda p: p.disable_freeu())]

    def freeu_through_unet(s):
        return [(s.kw(), lambda p: p.unet.disable_freeu()), (s.kw(), lambda p: p.unet.enable_freeu(**L.FREEU)),
                (s.kw(), lambda p: p.unet.disable_freeu())]

    return {f.__name__: f for f in (guidance, conditioning_scale, window, step_count, batch, cfg_on_off_on, prompt_replaced,
                                    prompt_in_place, controls_replaced, controls_in_place, scheduler_swapped, freeu_through_pipe,
                                    freeu_through_unet)}


def latents_of(pipe, kw):
    return pipe(**kw, output_type="latent").images.clone()


@pytest.mark.parametrize("name", sorted(transitions()))
def test_call_b_after_call_a_gives_the_bits_of_a_fresh_pipeline(name):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    seq = Seq()
    calls = transitions()[name](seq)
    used = build_pipe()
    used.enable_hip_graphs(True)
    got = []
    for kw, prepare in calls:
        if prepare is not None:
            prepare(used)
        got.append(latents_of(used, kw))
    moved = False
    for i in range(1, len(calls)):
        kw, prepare = calls[i]
        fresh = build_pipe()
        fresh.enable_hip_graphs(True)
        if prepare is not None and name not in ("prompt_in_place", "controls_in_place"):   # (a mutation has happened already)
            prepare(fresh)
        want = latents_of(fresh, kw)
        assert bool(torch.isfinite(want).all())
        assert torch.equal(got[i], want), (name, i, float((got[i] - want).abs().max()))
        moved = moved or not (got[i].shape == got[i - 1].shape and torch.equal(got[i], got[i - 1]))
    assert moved, "the transition changes nothing: it tests no cache"


def extractor_state(fe):
    """the state-dict entries of a live controlnet.BiDirFeatureExtractor (names of controlnet.py:31-34)"""
    out = {}
    for side in ("first", "last"):
        for i, pc in zip((0, 2, 4, 6, 8), fe.pre[side]):
            out[f"{side}_pre_extractor.{i}"] = pc
        for i, pc in enumerate(fe.ext[side]):
            out[f"extractors_{side}.{i}.0"] = pc
    for i, (a, b) in enumerate(fe.metric):
        out[f"wrapper.{i}.metric_net.0"], out[f"wrapper.{i}.metric_net.2"] = a, b
    for i, pc in enumerate(fe.zero):
        out[f"zero_convs.{i}"] = pc
    return out


def test_a_training_step_on_the_control_pyramid_reaches_the_next_decode():
    """an SGD step through pyramid_train on the live extractor's own tensors, then the same call with the same control tensors:
    the bits of a pipeline freshly built from the updated weights"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from diffcodec_amd import pyramid_train
    seq = Seq()
    kw = seq.kw()
    used = build_pipe()
    used.enable_hip_graphs(True)
    before = latents_of(used, kw)
    fe = used.controlnet.feature_extractor
    model = pyramid_train.BiDirFeatureExtractor.from_inference(fe)
    params = [p for p in model.parameters() if p.requires_grad]
    opt = torch.optim.SGD(params, lr=0.02)
    with torch.enable_grad():
        loss = sum(lv.square().mean() for lv in model(seq.dev["cond"], seq.dev["flow"]))
        loss.backward()
    for p in params:                                         # every tensor moves by up to the learning rate
        if p.grad is not None:
            p.grad.div_(p.grad.abs().max().clamp_min(1e-30))
    opt.step()
    torch.cuda.synchronize()
    got = latents_of(used, kw)
    raw = TL.raw_weights()
    csd = dict(raw["cn"][0])
    for k, pc in extractor_state(fe).items():
        assert csd["feature_extractor." + k + ".weight"].shape == pc.w.shape
        csd["feature_extractor." + k + ".weight"] = pc.w.detach().cpu().clone()
        csd["feature_extractor." + k + ".bias"] = pc.bias.detach().cpu().clone()
    assert any(not torch.equal(csd[k], raw["cn"][0][k]) for k in csd), "the step moved no weight"
    fresh = build_pipe(csd=csd)
    fresh.enable_hip_graphs(True)
    want = latents_of(fresh, kw)
    assert not torch.equal(want, before), "the step does not reach the latents: it tests no cache"
    assert torch.equal(got, want), float((got - want).abs().max())
