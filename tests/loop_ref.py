"""CPU restatement of the sampling loop the device runs in Python (pipeline.py `__call__`, `_denoise_fused`, `_denoise_generic`):
which timestep row a step reads, whether the ControlNets run and at what scale, how the two classifier-free-guidance halves
combine, what the sampler does with the prediction and what the VAE is handed.  Written from the reference's pipeline.py:144-404 and
oracle/pipeline_ref.py over tests/block_ref.py's blocks; nothing here imports the package.  tests/test_loop_ref.py (CPU) and
tests/test_gpu_loop.py (GPU) share the cases, the faults and the schedule.

    q      the rounding function of block_ref.  `ident` (fp64) is the REFERENCE: tests/test_loop_ref.py pins it to
           oracle/pipeline_ref.decode_frame run in fp64 on the same pyramid, to 1e-9.  `bf16` is the EMULATION of the device.
    fault  None or one name of FAULTS: a wiring mistake of this restatement, used only to show what the bars reject.
    loop   "fused" (zero-convs applied with the skip as the GEMM's residual operand, the ControlNet skipped at scale 0) or
           "generic" (module calls: scaled residuals stored, combined and added by dc_add_bf16).  The same values under `ident`.

The control pyramid is an INPUT (one list of four fp32 levels per ControlNet, at the frame batch): its extractors decide discretely
(occlusion threshold, splat order), so the device's own pyramid is handed to both sides, as DESIGN.md §18 does for the blocks.

Rounding points the loop adds over block_ref's R1-R11, each with the device code that rounds there:
  L1  the model input is the fp32 latents rounded to bf16, once per step, the same bits for both guidance halves
      (csrc/elementwise.hip latents_to_model_input_kernel:99 before the first step, cfg_ddim_kernel:85 / cfg_unipc_kernel:226 after
      each; the generic loop: unet.to_nhwc_bf16 -> ops.nchw_f32_to_nhwc_bf16)
  L2  the text context cat(negative, prompt) is stored bf16 (pipeline.py:365; unet.py:84 / controlnet.py:110 in the generic loop)
  L3  each pyramid level is stored bf16 ahead of the FDN gamma / beta convolutions (controlnet.py:134; block_ref.fdn rounds it)
  L4  the VAE input is bf16(latents * (1 / scaling_factor)), the product in fp32 (pipeline.py:271, latents_to_model_input_kernel:99)
  L5  FreeU: the scaled backbone half and the filtered skip are each rounded once (csrc/elementwise.hip:154,167)
  L6  generic loop only: every ControlNet's scaled residuals are stored bf16 (controlnet.py:171-172), two nets' residuals add
      with one rounding (rescontrolnet.combine_residuals) and the UNet adds them with one more (unet.py:113,119); the fused loop
      forms zero_conv(f) * scale + skip in one epilogue (unet.py:110,117)
Kept in fp32 on the device and NOT rounded here: the noise prediction `eps` (conv_out with out_f32, unet.py:132), the guidance
combine, the sampler state (latents, UniPC's two x0 predictions and last sample) and the decoded image with its postprocess.
The emulation carries all of these in fp64: fp32's 2^-24 is 2^-16 of a bf16 rounding, far under what the bars resolve.  The
samplers are oracle/pipeline_ref's DDIMRef and UniPCRef (their coefficient tables are fp32 values, as the device's are).
Where every scale of a step is 0 the fused loop skips the ControlNets (pipeline.py:399-402); so does this restatement in "fused",
under `ident` too: the reference multiplies finite residuals by 0.
"""
import collections

import torch

import block_ref as B
from oracle import pipeline_ref as R

F64 = torch.float64
SIZE = 128                     # the smallest frame the control stage accepts: its coarsest level (SIZE / 64) must be 2 pixels wide
LAT = SIZE // 8
FREEU = dict(s1=0.9, s2=0.2, b1=1.2, b2=1.4)                               # validation.py:106

Case = collections.namedtuple("LoopCase", "name opts")
_DEFAULT = dict(b=1, steps=4, g=4.5, scales=(1.7,), window=(0.0, 1.0), sched="ddim", freeu=None, eta=0.0, guess=False)


def _case(name, **kw):
    assert set(kw) <= set(_DEFAULT), kw
    return Case(name, dict(_DEFAULT, **kw))


LOOP_CASES = [
    _case("full_window_b2", b=2, steps=3),
    _case("window_scale16_g1.5", g=1.5, scales=(16.0,), window=(0.25, 0.75)),
    _case("two_steps_g1.5", steps=2, g=1.5),
    _case("guidance_off", steps=3, g=1.0),
    _case("two_nets", steps=3, scales=(1.7, 3.0)),
    _case("unipc_freeu", sched="unipc", freeu=FREEU, g=3.5, scales=(1.35,)),
    _case("eta_generic", steps=3, eta=0.6),
    _case("guess_mode_generic", steps=2, guess=True),
]
CASES = {c.name: c for c in LOOP_CASES}


def loops_of(case):
    """the device loops a case can run on: eta > 0 and guess_mode force the generic loop (pipeline.py:257-259)"""
    o = case.opts
    return ("generic",) if (o["eta"] or o["guess"]) else ("fused", "generic")


# fault -> the predicate of the options under which it can show at all
FAULTS = {
    "cfg_halves_swapped": lambda o: o["g"] > 1.0,
    "cfg_weight_g_minus_1": lambda o: o["g"] > 1.0,
    "scaling_factor_dropped": lambda o: True,
    "keep_ignored": lambda o: o["window"] != (0.0, 1.0),
    "keep_window_late_by_one": lambda o: o["window"] != (0.0, 1.0),
    "steps_offset_dropped": lambda o: o["sched"] == "ddim",
    "timestep_lags_one_step": lambda o: True,
    "second_net_dropped": lambda o: len(o["scales"]) == 2,
    "postprocess_no_clamp": lambda o: True,
    "unipc_corrector_dropped": lambda o: o["sched"] == "unipc",
    "unipc_first_order_last_step_dropped": lambda o: o["sched"] == "unipc",
    "freeu_on_every_up_block": lambda o: o["freeu"] is not None,
    "freeu_b_s_exchanged": lambda o: o["freeu"] is not None,
    "guess_mode_uncond_not_zeroed": lambda o: o["guess"] and o["g"] > 1.0,
}
# `vae_input_not_rescaled_for_latent_init` is not here: latents initialised from an encoded frame are scaled by the caller before
# `__call__` (sample * scaling_factor * init_noise_sigma), so no case of the loop reaches it.

# Faults that no designed case rejects at twice its bar (tests/test_loop_ref.py prints their best factor) -> the exact check of
# tests/test_gpu_loop.py that holds them instead.
EXACT_ONLY = {
    "steps_offset_dropped": "test_schedule_rows_and_timesteps_are_loop_ref_s",
    "timestep_lags_one_step": "test_fused_loop_equals_the_hand_driven_chain",
    "unipc_corrector_dropped": "test_unipc_table_runs_the_corrector_at_loop_ref_s_orders",
}


def fault_applies(fault, case):
    return bool(FAULTS[fault](case.opts))


# ------------------------------------------------------------------------------------------ schedule
class UniPC(R.UniPCRef):
    """oracle/pipeline_ref.UniPCRef kept in fp64 (the oracle hands fp32 latents back), with the two sampler faults."""

    def __init__(self, fault=None):
        super().__init__()
        self.fault = fault

    def step(self, eps, t, x):
        i, n = self.step_index, len(self.timesteps)
        if self.fault == "unipc_corrector_dropped":
            self.last_sample = None                          # the corrector needs it (UniPCRef.step); the predictor does not
        if self.fault == "unipc_first_order_last_step_dropped" and i + 1 == n and n > 1:
            # lower_order_final ignored: the last step runs the second-order predictor towards sigma = 0, where its step ratio is 0
            a_i, s_i = self._as(self.sigmas[i])
            m_t = (x.double() - s_i * eps.double()) / a_i
            return self._update(x.double(), m_t, [self.model_outputs[-1]], self.sigmas[i + 1], self.sigmas[i], [self.sigmas[i - 1]], 2)
        a_i, s_i = self._as(self.sigmas[i])
        m_t = (x.double() - s_i * eps.double()) / a_i
        super().step(eps, t, x)
        # the value before the oracle's cast to fp32: the last step returns the x0 prediction, the others the predictor's output,
        # which UniPCRef recomputes from this state on its next call; redo the predictor here in fp64
        if i + 1 == n:
            return m_t
        o = self.this_order
        return self._update(self.last_sample, m_t, [self.model_outputs[-2]] if o == 2 else [], self.sigmas[i + 1], self.sigmas[i],
                            [self.sigmas[i - 1]] if o == 2 else [], o)


def make_scheduler(o, fault=None):
    if o["sched"] == "unipc":
        s = UniPC(fault)
    else:
        s = R.DDIMRef(steps_offset=0 if fault == "steps_offset_dropped" else 1)
    s.set_timesteps(o["steps"])
    return s


def keep_of(i, nt, window, fault=None):
    """pipeline.py:292-295"""
    if fault == "keep_ignored":
        return 1.0
    if fault == "keep_window_late_by_one":
        i -= 1
    return 1.0 - float(i / nt < window[0] or (i + 1) / nt > window[1])


Step = collections.namedtuple("Step", "index t t_net keep scales")


def schedule(o, fault=None):
    """-> [Step]: per step the table row, the scheduler's timestep, the timestep the nets are fed, the keep value and each net's
    conditioning scale (base scale x keep, pipeline.py:338)."""
    ts = [int(t) for t in make_scheduler(o, fault).timesteps]
    out = []
    for i, t in enumerate(ts):
        keep = keep_of(i, len(ts), o["window"], fault)
        t_net = ts[max(i - 1, 0)] if fault == "timestep_lags_one_step" else t
        out.append(Step(i, t, t_net, keep, tuple(float(s * keep) for s in o["scales"])))
    return out


def ddim_rows(o):
    """the device's DDIM table (scheduler.DDIMScheduler.coefficients): per step sqrt(1 - a_t), sqrt(a_t), sqrt(a_prev),
    sqrt(1 - a_prev) formed in fp32 from DDIMRef's fp32 alphas_cumprod -> fp32 [steps, 4]"""
    s = make_scheduler(o)
    rows = []
    for t in s.timesteps.tolist():
        prev = t - s.T // s.n
        a_t = s.alphas_cumprod[t]
        a_p = s.alphas_cumprod[prev] if prev >= 0 else s.final_alpha_cumprod
        rows.append(torch.stack([(1 - a_t) ** 0.5, a_t ** 0.5, a_p ** 0.5, (1 - a_p) ** 0.5]))
    return torch.stack(rows)


def unipc_flags(o):
    """the flag word of each row of the device's UniPC table (csrc/elementwise.hip cfg_unipc_kernel: 1 the corrector runs, 2 it
    uses the older x0 prediction, 4 the predictor does), read off UniPCRef's own warm-up state machine on a dummy decode"""
    s = make_scheduler(o)
    z = torch.zeros(1, dtype=F64)
    flags = []
    for i, t in enumerate(s.timesteps.tolist()):
        corr = i > 0 and s.last_sample is not None
        corr_order = s.this_order
        s.step(z, t, z)
        flags.append((1 if corr else 0) | (2 if corr and corr_order == 2 else 0) | (4 if s.this_order == 2 else 0))
    return flags


# ------------------------------------------------------------------------------------------ the loop
def decode(W, inp, o, q=B.ident, fault=None, loop="fused", upto=None):
    """W: dict(unet, cn: [state dict per ControlNet], vae: fp64 state dicts; unet_cfg, vae_cfg).
    inp: dict(latents [b, 4, h, w], pe, npe [b, 77, D]: fp32 values widened; pyr: [per net: four levels at batch b];
    noise: [per step: the variance noise] when eta > 0).
    -> dict(latents, image, steps: the latents after every step)."""
    assert loop in ("fused", "generic") and (fault is None or fault in FAULTS)
    ucfg, b = W["unet_cfg"], inp["latents"].shape[0]
    do_cfg = o["g"] is not None and o["g"] > 1.0                                        # pipeline.py:202
    ctx = q(torch.cat([inp["npe"], inp["pe"]], 0) if do_cfg else inp["pe"])             # :234-236, L2
    sched = make_scheduler(o, fault)
    latents = inp["latents"] * sched.init_noise_sigma
    nets = list(zip(W["cn"], inp["pyr"]))
    assert len(nets) == len(o["scales"])
    if fault == "second_net_dropped":
        nets = nets[:1]
    guess = o["guess"] and do_cfg
    freeu_fault = fault if fault in ("freeu_on_every_up_block", "freeu_b_s_exchanged") else None
    trail = []
    for st in schedule(o, fault):
        if upto is not None and st.index >= upto:
            break
        x1 = q(latents)                                                                 # L1
        x_in = torch.cat([x1, x1], 0) if do_cfg else x1                                 # :313-320
        if guess:                                                                       # :323-327: the conditional half alone
            c_in, c_ctx, rep = x1, ctx[b:], 1
        else:
            c_in, c_ctx, rep = x_in, ctx, 2 if do_cfg else 1
        live = [(csd, [torch.cat([lv] * rep, 0) for lv in pyr], sc) for (csd, pyr), sc in zip(nets, st.scales)]
        kw = dict(freeu=o["freeu"], fault=freeu_fault)
        if loop == "fused":
            controls = []
            for csd, pyr, sc in live:
                if sc == 0.0:
                    continue
                feats, midf = B.controlnet(csd, ucfg, c_in, st.t_net, c_ctx, pyr, sc, q, features_only=True)
                controls.append((feats, midf, csd, sc))
            eps = B.unet(W["unet"], ucfg, x_in, st.t_net, ctx, q, controls=controls, **kw)
        else:
            down = mid = None
            for csd, pyr, sc in live:
                d_, m_ = B.controlnet(csd, ucfg, c_in, st.t_net, c_ctx, pyr, sc, q)     # :341-350, L6
                down, mid = (d_, m_) if down is None else B.combine_residuals((down, mid), (d_, m_), q)
            down, mid = [d.v for d in down], mid.v
            if guess:                                                                   # :353-355
                first = (lambda d: d) if fault == "guess_mode_uncond_not_zeroed" else torch.zeros_like
                down, mid = [torch.cat([first(d), d], 0) for d in down], torch.cat([first(mid), mid], 0)
            eps = B.unet(W["unet"], ucfg, x_in, st.t_net, ctx, q, down_res=down, mid_res=mid, **kw)   # :358-367
        eps = eps.v
        if do_cfg:                                                                      # :370-372
            eu, et = eps[:b], eps[b:]
            if fault == "cfg_halves_swapped":
                eu, et = et, eu
            eps = eu + ((o["g"] - 1.0) if fault == "cfg_weight_g_minus_1" else o["g"]) * (et - eu)
        if o["sched"] == "unipc":                                                       # :375
            latents = sched.step(eps, st.t, latents)
        else:
            latents = sched.step(eps, st.t, latents, o["eta"], inp["noise"][st.index] if o["eta"] else None)
        trail.append(latents)
    if upto is not None:
        return dict(latents=latents, steps=trail)
    vcfg = W["vae_cfg"]
    z = latents if fault == "scaling_factor_dropped" else latents / vcfg["scaling_factor"]   # :391
    img = B.vae_decode(W["vae"], vcfg, q(z), q).v                                       # L4
    img = img / 2 + 0.5                                                                 # :397-398
    if fault != "postprocess_no_clamp":
        img = img.clamp(0, 1)
    return dict(latents=latents, image=img, steps=trail)


# ------------------------------------------------------------------------------------------ references, shared and unchanged
_CACHE = {}


def reference_and_bars(case, W, inp, loop="fused", key=None):
    """-> dict(ref, emu: decode() results; emu_figs, bars: {output: (rel_l2, max_rel)} for `latents`, `image` and every step);
    computed once per process, case, loop and `key` (what the pyramid came from), never changed.  The reference is one per case:
    under `ident` the two loops are the same arithmetic (tests/test_loop_ref.py holds both to the oracle); the emulation is the
    loop's own."""
    k, kr = (case.name, loop, key), (case.name, key)
    if kr not in _CACHE:
        _CACHE[kr] = decode(W, inp, case.opts, B.ident, None, loops_of(case)[0])
    if k not in _CACHE:
        ref = _CACHE[kr]
        emu = decode(W, inp, case.opts, B.bf16, None, loop)
        figs = {n: B.figures(emu[n], ref[n]) for n in ("latents", "image")}
        for i, (e, r) in enumerate(zip(emu["steps"], ref["steps"])):
            figs[f"step{i}"] = B.figures(e, r)
        _CACHE[k] = dict(ref=ref, emu=emu, emu_figs=figs, bars={n: (B.MARGIN * f[0], B.MARGIN * f[1]) for n, f in figs.items()})
    return _CACHE[k]


def factor(out, rb):
    """the largest figure / bar of a decode() result over final latents and image (inf where it is not finite)"""
    worst = 0.0
    for n in ("latents", "image"):
        if not bool(torch.isfinite(out[n]).all()):
            return float("inf")
        worst = max(worst, max(f / bar for f, bar in zip(B.figures(out[n], rb["ref"][n]), rb["bars"][n])))
    return worst
