"""CPU: tests/loop_ref.py is (1) the oracle — its fp64 restatement of the sampling loop equals oracle/pipeline_ref.decode_frame run in
fp64 on the same pyramid, to 1e-9, on every case; (2) sharp — every named wiring fault of the loop misses some case's bar (4 x the
bf16 emulation's own error, on final latents or image) by a factor of at least 2, or is listed in loop_ref.EXACT_ONLY with the exact
check of tests/test_gpu_loop.py that holds it; (3) not weakened silently — removing the sole case that rejects a fault names the
fault; (4) fair — the oracle's own fp32 run passes every bar."""
import contextlib

import pytest
import torch

import block_ref as B
import loop_ref as L
import test_block_ref  # noqa: F401  (hands block_ref the synthesized weights)
from oracle import control_ref as C
from oracle import pipeline_ref as R
from oracle import sd15_ref as M

F64 = torch.float64
_MEMO = {}


def f64(sd):
    return {k: v.to(F64) for k, v in sd.items()}


def raw_weights():
    """fp32 state dicts of selftest's reduced-width models: (unet, flow ControlNet, residual ControlNet, vae) and the two configs"""
    if "raw" not in _MEMO:
        from diffcodec_amd import selftest as T
        from diffcodec_amd import weights as W
        usd, csd, vsd = T.small_state_dicts()
        _MEMO["raw"] = dict(unet=usd, cn=[csd, W.synthesize(W.rescontrolnet_spec(T.SMALL_UNET), 5)], vae=vsd, unet_cfg=T.SMALL_UNET,
                            vae_cfg=T.SMALL_VAE)
    return _MEMO["raw"]


def loop_weights(n_nets):
    raw = raw_weights()
    if "w64" not in _MEMO:
        _MEMO["w64"] = dict(unet=f64(raw["unet"]), cn=[f64(s) for s in raw["cn"]], vae=f64(raw["vae"]))
    w = _MEMO["w64"]
    return dict(unet=w["unet"], cn=w["cn"][:n_nets], vae=w["vae"], unet_cfg=raw["unet_cfg"], vae_cfg=raw["vae_cfg"])


def call_inputs(case):
    """the tensors a pipeline call of this case receives (fp32, CPU), and the variance noise of each step where eta > 0"""
    from diffcodec_amd.synthetic import synth_controls, synth_latents, synth_text
    o = case.opts
    b = o["b"]
    cond, flow = synth_controls(b, L.SIZE)
    pe, npe = synth_text(b, dim=raw_weights()["unet_cfg"]["cross_attention_dim"])
    out = dict(cond=cond, flow=flow, pe=pe, npe=npe, latents=synth_latents(b, L.SIZE), warp=None, noise=None)
    if len(o["scales"]) == 2:
        out["warp"] = torch.rand(b, 3, L.SIZE, L.SIZE, generator=torch.Generator().manual_seed(9))
    if o["eta"]:
        # diffusers draws the variance noise with the caller's generator in the model's dtype (bf16 here), one draw per step
        g = torch.Generator().manual_seed(ETA_SEED)
        out["noise"] = [torch.randn((b, 4, L.LAT, L.LAT), generator=g, dtype=torch.bfloat16).to(F64) for _ in range(o["steps"])]
    return out


ETA_SEED = 31


def oracle_pyramids(case, ci):
    """the control pyramids of the oracle's fp32 control stage (on the GPU the device's own pyramids take their place)"""
    raw = raw_weights()
    pyrs = [C.bi_dir_feature_extractor(raw["cn"][0], "feature_extractor.", ci["cond"], ci["flow"])]
    if len(case.opts["scales"]) == 2:
        rp = C.bi_dir_residue_extractor(raw["cn"][1], "feature_extractor.", ci["cond"][:, :3], ci["cond"][:, 3:], ci["flow"][:, :2],
                                        ci["flow"][:, 2:])
        rw = C.warp_extractor(raw["cn"][1], "warp_extractor.", ci["warp"])
        pyrs.append([a + b for a, b in zip(rp, rw)])
    return pyrs


def loop_inputs(ci, pyrs):
    return dict(latents=ci["latents"].to(F64), pe=ci["pe"].to(F64), npe=ci["npe"].to(F64), noise=ci["noise"],
                pyr=[[lv.detach().to("cpu", F64) for lv in p] for p in pyrs])


def cpu_setup(case):
    """-> (weights, loop_ref inputs, call inputs) of a case on the oracle's pyramid; built once"""
    if case.name not in _MEMO:
        ci = call_inputs(case)
        _MEMO[case.name] = (loop_weights(len(case.opts["scales"])), loop_inputs(ci, oracle_pyramids(case, ci)), ci)
    return _MEMO[case.name]


def cpu_bars(case, loop=None):
    W, inp, _ = cpu_setup(case)
    return L.reference_and_bars(case, W, inp, loop or L.loops_of(case)[0], key="oracle pyramid")


# ------------------------------------------------------------------------------------------ pinned to the oracle
@contextlib.contextmanager
def given_pyramids(pyrs):
    """oracle/pipeline_ref.decode_frame on given pyramids: its control stage returns them"""
    saved = C.bi_dir_feature_extractor, C.bi_dir_residue_extractor, C.warp_extractor
    C.bi_dir_feature_extractor = lambda *a, **k: pyrs[0]
    C.bi_dir_residue_extractor = lambda *a, **k: pyrs[1]
    C.warp_extractor = lambda *a, **k: [torch.zeros_like(p) for p in pyrs[1]]
    try:
        yield
    finally:
        C.bi_dir_feature_extractor, C.bi_dir_residue_extractor, C.warp_extractor = saved


@contextlib.contextmanager
def oracle_widened():
    """The oracle's `.float()` casts (latents, UniPC's return, FreeU's filter, the variance noise) become `.double()`; its fp32
    timestep sinusoid keeps its arithmetic and is widened, as in tests/test_block_ref.py."""
    real, sinus = torch.Tensor.float, M.timestep_embedding

    def widen(t):
        return t.double()

    def sinus64(t, dim):
        torch.Tensor.float = real
        try:
            return sinus(t, dim).double()
        finally:
            torch.Tensor.float = widen

    torch.Tensor.float, M.timestep_embedding = widen, sinus64
    try:
        yield
    finally:
        torch.Tensor.float, M.timestep_embedding = real, sinus


def run_oracle(case, sds, pyrs, ci):
    o = case.opts
    two = len(o["scales"]) == 2
    with given_pyramids(pyrs):
        return R.decode_frame(
            sds["unet"], sds["cn"][0], sds["vae"], sds["unet_cfg"], sds["vae_cfg"], ci["cond"], ci["flow"], ci["pe"], ci["npe"],
            ci["latents"], num_inference_steps=o["steps"], guidance_scale=o["g"], controlnet_conditioning_scale=o["scales"][0],
            return_latents=True, control_guidance_start=o["window"][0], control_guidance_end=o["window"][1], eta=o["eta"],
            generator=torch.Generator().manual_seed(ETA_SEED) if o["eta"] else None, noise_dtype=torch.bfloat16,
            res_cn_sd=sds["cn"][1] if two else None, warp_cond=ci["warp"], res_conditioning_scale=o["scales"][1] if two else None,
            scheduler=o["sched"], freeu=o["freeu"], guess_mode=o["guess"])


@pytest.mark.parametrize("case", L.LOOP_CASES, ids=[c.name for c in L.LOOP_CASES])
def test_identity_restatement_is_the_oracle(case):
    W, inp, ci = cpu_setup(case)
    with oracle_widened():
        img, lat = run_oracle(case, W, inp["pyr"], {k: (v.to(F64) if torch.is_tensor(v) else v) for k, v in ci.items()})
    assert img.dtype == F64 and lat.dtype == F64
    for loop in ("fused", "generic"):                        # under `ident` the two loops are the same arithmetic
        if loop == "fused" and case.opts["guess"]:
            continue                                         # guess_mode exists in the generic loop only
        ref = cpu_bars(case)["ref"] if loop == L.loops_of(case)[0] else L.decode(W, inp, case.opts, B.ident, None, loop)
        for name, mine, theirs in (("latents", ref["latents"], lat), ("image", ref["image"], img)):
            figs = B.figures(mine, theirs)
            assert mine.shape == theirs.shape and max(figs) <= 1e-9, (loop, name, figs)
    # the emulation rounds: it differs from the reference, by no more than the few percent of some hundred bf16 launches per step
    for name, (e0, e1) in cpu_bars(case)["emu_figs"].items():
        assert 0 < e0 < 0.1 and 0 < e1 < 0.1, (name, e0, e1)


@pytest.mark.parametrize("case", L.LOOP_CASES, ids=[c.name for c in L.LOOP_CASES])
def test_the_oracle_s_fp32_run_passes_every_bar(case):
    _, inp, ci = cpu_setup(case)
    img, lat = run_oracle(case, raw_weights(), [[lv.float() for lv in p] for p in inp["pyr"]], ci)
    assert img.dtype == torch.float32
    rb = cpu_bars(case)
    f = L.factor(dict(latents=lat, image=img), rb)
    print(f"{case.name}\tfp32 oracle at {f:.2e} of the bar")
    assert f <= 1.0, f


# ------------------------------------------------------------------------------------------ sharpness
def factors_of(fault):
    """{case name: figure / bar of the faulted fp64 restatement}, over the cases the fault applies to; computed once"""
    k = ("fault", fault)
    if k not in _MEMO:
        out = {}
        for case in L.LOOP_CASES:
            if L.fault_applies(fault, case):
                W, inp, _ = cpu_setup(case)
                loop = L.loops_of(case)[0]
                out[case.name] = L.factor(L.decode(W, inp, case.opts, B.ident, fault, loop), cpu_bars(case, loop))
        _MEMO[k] = out
    return _MEMO[k]


def unrejected(cases):
    """the faults outside EXACT_ONLY that none of `cases` rejects at twice its bar"""
    names = {c.name for c in cases}
    return sorted(f for f in L.FAULTS if f not in L.EXACT_ONLY
                  and not any(v >= 2.0 for n, v in factors_of(f).items() if n in names))


@pytest.mark.parametrize("fault", sorted(L.FAULTS))
def test_every_fault_misses_a_bar_by_a_factor_of_two_or_is_held_exactly(fault):
    fs = factors_of(fault)
    assert fs, "no case takes this fault"
    name = max(fs, key=fs.get)
    if fault in L.EXACT_ONLY:
        import test_gpu_loop
        print(f"{fault}\tEXACT_ONLY: best {fs[name]:.2f} x the bar on {name}; held by test_gpu_loop.{L.EXACT_ONLY[fault]}")
        assert fs[name] < 2.0, "a case rejects it: it does not belong in EXACT_ONLY"
        assert callable(getattr(test_gpu_loop, L.EXACT_ONLY[fault], None)), L.EXACT_ONLY[fault]
        return
    print(f"{fault}\trejected by {fs[name]:.1f} x the bar on {name}")
    assert fs[name] >= 2.0, (fault, fs)


def test_exact_only_names_known_faults():
    assert set(L.EXACT_ONLY) <= set(L.FAULTS)


def test_removing_the_sole_case_that_rejects_a_fault_names_it():
    assert unrejected(L.LOOP_CASES) == []
    sole = 0
    for i, c in enumerate(L.LOOP_CASES):
        mine = sorted(f for f in L.FAULTS if f not in L.EXACT_ONLY
                      and [n for n, v in factors_of(f).items() if v >= 2.0] == [c.name])
        if mine:
            sole += 1
            assert unrejected(L.LOOP_CASES[:i] + L.LOOP_CASES[i + 1:]) == mine
    assert sole > 0


def test_a_fault_is_refused_where_it_cannot_show():
    assert not L.fault_applies("second_net_dropped", L.CASES["full_window_b2"])
    assert not L.fault_applies("keep_ignored", L.CASES["full_window_b2"])
    assert L.fault_applies("keep_ignored", L.CASES["window_scale16_g1.5"])


def test_schedule_is_the_reference_s():
    """pipeline.py:292-295,338 by hand for the window case: steps 0 and 3 are outside 0.25..0.75"""
    o = L.CASES["window_scale16_g1.5"].opts
    s = L.schedule(o)
    assert [st.t for st in s] == [751, 501, 251, 1] and [st.t_net for st in s] == [751, 501, 251, 1]
    assert [st.keep for st in s] == [0.0, 1.0, 1.0, 0.0] and [st.scales for st in s] == [(0.0,), (16.0,), (16.0,), (0.0,)]
    assert [st.keep for st in L.schedule(o, "keep_window_late_by_one")] == [0.0, 0.0, 1.0, 1.0]
    assert [st.t_net for st in L.schedule(o, "timestep_lags_one_step")] == [751, 751, 501, 251]
    assert [st.t for st in L.schedule(o, "steps_offset_dropped")] == [750, 500, 250, 0]
    assert [st.t for st in L.schedule(L.CASES["unipc_freeu"].opts)] == [801, 601, 401, 201]
    # UniPC's warm-up: first order, then second; the last step's predictor falls back to first order (lower_order_final)
    assert L.unipc_flags(L.CASES["unipc_freeu"].opts) == [0, 1 | 4, 1 | 2 | 4, 1 | 2]
