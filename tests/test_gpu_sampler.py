"""GPU: the two fused loop kernels (dc_cfg_ddim_step, dc_cfg_unipc_step) run from the first step of a 20-step schedule to the
last — CFG combine, multistep rotation, device step counter — against the exact probability-flow ODE of a Gaussian prior
(tests/sampler_ref.py), eagerly and as one captured graph, on fresh and on used multistep buffers; and the
fused pipeline loop held to the prompt it is given when the caller refills an embedding buffer in place.

Two bars, neither fitted to the device.  `run64` / `run32` are the numpy loops of sampler_ref on the device's own fp32 table in
fp64 / fp32 arithmetic:  (a) max|device - run64| <= 4 max|run32 - run64| (the margin DESIGN.md gives a device over the
reference arithmetic in fp32, sections 10 and 13);  (b) max|device - ODE| <= max|run64 - ODE| + bar (a)."""
import numpy as np
import pytest
import torch

import edge_cases as E
import sampler_ref as S

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
N_STEPS = 20
SD = 0.5
SHAPES = [E.STATE_SHAPES[0], (2, 4, 16, 24)]
KINDS = ["ddim", "unipc1", "unipc2"]
G32 = float(np.float32(E.STATE_GUIDANCE))            # the guidance the kernels see


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from diffcodec_amd import ops as o
    return o


def _bits(a, b):
    it = torch.int16 if a.dtype == BF else torch.int32
    return a.shape == b.shape and torch.equal(a.contiguous().view(it), b.contiguous().view(it))


# ------------------------------------------------------------------------------------------ the problem and its references
class Problem:
    """One loop variant on one state shape: the scheduler's fp32 table, (alpha, sigma) per step, x_T, the per-row means, and the
    numpy references, computed once and shared by the tests (never modified)."""
    _cache = {}

    @classmethod
    def get(cls, kind, cfg, shape, sd, seed=0):
        key = (kind, cfg, shape, sd, seed)
        if key not in cls._cache:
            cls._cache[key] = cls(kind, cfg, shape, sd, seed)
        return cls._cache[key]

    def __init__(self, kind, cfg, shape, sd, seed):
        from diffcodec_amd.scheduler import DDIMScheduler, UniPCMultistepScheduler
        self.kind, self.cfg, self.shape, self.sd = kind, cfg, shape, sd
        self.ddim = kind == "ddim"
        self.sched = DDIMScheduler() if self.ddim else UniPCMultistepScheduler(solver_order=int(kind[-1]))
        self.sched.set_timesteps(N_STEPS)
        self.coef = self.sched.coefficients()
        rows = self.coef.double().numpy()
        if self.ddim:
            self.alpha, self.sigma = rows[:, 1], rows[:, 0]
            self.end = (rows[-1, 2], rows[-1, 3])
        else:
            self.alpha, self.sigma = S.alpha_sigma(self.sched.sigmas[:-1])
            self.end = S.alpha_sigma(self.sched.sigmas[-1])
        b = shape[0]
        gen = torch.Generator().manual_seed(9700 + 31 * seed + KINDS.index(kind) + 7 * int(cfg) + 13 * shape[3])
        self.x_T = torch.randn(shape, generator=gen)
        mu_u = (0.9 * torch.randn(b, 1, 1, 1, generator=gen)).float()
        mu_t = (0.9 * torch.randn(b, 1, 1, 1, generator=gen)).float()
        self.mus = [mu_u, mu_t] if cfg else [mu_t]
        mu_g = mu_u.double() + G32 * (mu_t.double() - mu_u.double()) if cfg else mu_t.double()
        x64 = self.x_T.double().numpy()
        self.flow = S.gaussian_flow(x64, self.alpha[0], self.sigma[0], *self.end, mu_g.numpy(), sd)
        if self.ddim:
            self.run64 = S.run_ddim_table(rows, x64, self._model(np.float64))
            self.run32 = S.run_ddim_table(rows, x64, self._model(np.float32), np.float32).astype(np.float64)
            self.state64 = self.state32 = None
        else:
            plans = S.unipc_table_plans(rows)
            self.run64, *self.state64 = S.run_plans(plans, x64, self._model(np.float64), state=True)
            r32 = S.run_plans(plans, x64, self._model(np.float32), dtype=np.float32, state=True)
            self.run32, *self.state32 = (v.astype(np.float64) for v in r32)
        self.e32 = float(np.max(np.abs(self.run32 - self.run64)))
        self.trunc = float(np.max(np.abs(self.run64 - self.flow)))

    def k(self, i):
        a, sg = float(self.alpha[i]), float(self.sigma[i])
        return a, sg / (a * a * self.sd * self.sd + sg * sg)

    def _model(self, f):
        """guided noise prediction in dtype f, the operations of `device_eps` and of the kernel's CFG combine in their order"""
        mus = [m.numpy().astype(f) for m in self.mus]

        def model(x, i):
            a, k = self.k(i)
            es = [(x - m * f(a)) * f(k) for m in mus]
            if not self.cfg:
                return es[0]
            eu, et = es
            g = f(G32)
            return eu + g * (et - eu) if self.ddim else (f(1.0) - g) * eu + g * et
        return model


class Loop:
    """The device state of one fused loop and its 20 steps.  eps is computed from the fp32 latents with torch ops on the device,
    uncond rows first, NHWC fp32 as the kernels read it."""

    def __init__(self, ops, p, ms_fill=0.0):
        self.ops, self.p = ops, p
        b, c, h, w = p.shape
        self.lat = torch.empty(p.shape, device=DEV)
        self.ms = [torch.full(p.shape, ms_fill, device=DEV) for _ in range(3)]
        self.x_in = torch.zeros(((2 if p.cfg else 1) * b, h, w, c), device=DEV, dtype=BF)
        self.step = torch.zeros(1, device=DEV, dtype=torch.int32)
        self.coef = p.coef.to(DEV)
        self.mus = [m.to(DEV) for m in p.mus]
        self.x_src = p.x_T.to(DEV)

    def reset(self, x_src=None, zero_ms=True):
        self.lat.copy_(self.x_src if x_src is None else x_src)
        self.step.zero_()
        if zero_ms:
            for m in self.ms:
                m.zero_()

    def device_eps(self, i):
        a, k = self.p.k(i)
        es = [(self.lat - m * a) * k for m in self.mus]
        e = torch.cat(es, 0) if self.p.cfg else es[0]
        return e.permute(0, 2, 3, 1).contiguous()

    def run(self):
        g = E.STATE_GUIDANCE if self.p.cfg else 1.0
        for i in range(N_STEPS):
            eps = self.device_eps(i)
            if self.p.ddim:
                self.ops.cfg_ddim_step(eps, self.lat, self.x_in, self.coef, self.step, g, self.p.cfg)
            else:
                self.ops.cfg_unipc_step(eps, self.lat, self.ms[0], self.ms[1], self.ms[2], self.x_in, self.coef, self.step, g, self.p.cfg)

    def snapshot(self):
        torch.cuda.synchronize()
        return [t.clone() for t in [self.lat, self.x_in, self.step] + self.ms]


def _np(t):
    return t.double().cpu().numpy()


def _check_model_in(loop, what):
    b = loop.p.shape[0]
    want = loop.lat.permute(0, 2, 3, 1).to(BF)
    assert _bits(loop.x_in[:b], want), f"{what}: model_in is not bf16(new latents) in NHWC"
    if loop.p.cfg:
        assert _bits(loop.x_in[b:], want), f"{what}: the CFG half of model_in differs"


_CASES = [(k, c, s) for k in KINDS for c in (True, False) for s in SHAPES]
_IDS = [f"{k}-{'cfg' if c else 'nocfg'}-{'x'.join(map(str, s))}" for k, c, s in _CASES]


# ------------------------------------------------------------------------------------------ 1. whole loops against the ODE
@pytest.mark.parametrize("kind,cfg,shape", _CASES, ids=_IDS)
def test_whole_loop_against_the_ode(ops, record, kind, cfg, shape):
    """20 steps from step counter 0, the device counter advancing on its own.  Bars (a) and (b) of the module docstring on the final
    latents; model_in is the bf16 rounding of them; for UniPC the three multistep buffers hold what the fp32 numpy loop holds, to
    bar (a) of each buffer."""
    p = Problem.get(kind, cfg, shape, SD)
    what = f"{kind} cfg={int(cfg)} {shape}"
    loop = Loop(ops, p)
    loop.reset()
    loop.run()
    torch.cuda.synchronize()
    assert int(loop.step.item()) == N_STEPS
    dev = _np(loop.lat)
    assert np.isfinite(dev).all()
    err = float(np.max(np.abs(dev - p.run64)))
    ode = float(np.max(np.abs(dev - p.flow)))
    print(f"{what}: device-run64 {err:.3e}  run32-run64 {p.e32:.3e}  ratio {err / p.e32:.3f}  device-ODE {ode:.3e}  run64-ODE {p.trunc:.3e}")
    record(f"sampler[{_IDS[_CASES.index((kind, cfg, shape))]}]", f"device_over_fp32cpu={err / p.e32:.3f} trunc={p.trunc:.3e}")
    assert p.e32 > 0
    assert err <= 4 * p.e32, f"{what}: |device - fp64 loop| {err:.3e} above 4 x |fp32 loop - fp64 loop| = {4 * p.e32:.3e}"
    assert ode <= p.trunc + 4 * p.e32, f"{what}: |device - ODE| {ode:.3e}, truncation {p.trunc:.3e}, 4 x fp32 {4 * p.e32:.3e}"
    _check_model_in(loop, what)
    if not p.ddim:
        for name, buf, r64, r32 in zip(("m0", "m1", "last"), loop.ms, p.state64, p.state32):
            e32 = float(np.max(np.abs(r32 - r64)))
            e = float(np.max(np.abs(_np(buf) - r64)))
            print(f"{what} {name}: device-run64 {e:.3e}  run32-run64 {e32:.3e}")
            assert e <= 4 * e32, f"{what}: buffer {name} {e:.3e} above 4 x {e32:.3e}"


# ------------------------------------------------------------------------------------------ 2. point mass
@pytest.mark.parametrize("kind,cfg,shape", _CASES, ids=_IDS)
def test_point_mass_on_the_device(ops, record, kind, cfg, shape):
    """s = 0: no solver error remains, so every loop variant ends on the closed form — the guided mean itself for UniPC (the schedule
    ends at sigma 0), alpha mu + (x_T - alpha_T mu) sigma / sigma_T at final_alpha_cumprod for DDIM — within bar (a)."""
    p = Problem.get(kind, cfg, shape, 0.0)
    what = f"point mass {kind} cfg={int(cfg)} {shape}"
    loop = Loop(ops, p)
    loop.reset()
    loop.run()
    torch.cuda.synchronize()
    dev = _np(loop.lat)
    err = float(np.max(np.abs(dev - p.flow)))
    print(f"{what}: device-closed form {err:.3e}  run32-run64 {p.e32:.3e}  run64-closed form {p.trunc:.3e}")
    record(f"sampler_point[{_IDS[_CASES.index((kind, cfg, shape))]}]", f"device_err_over_fp32cpu={err / p.e32:.3f}")
    assert np.isfinite(dev).all() and p.e32 > 0
    assert err <= 4 * p.e32, f"{what}: {err:.3e} above 4 x {p.e32:.3e}"
    _check_model_in(loop, what)


# ------------------------------------------------------------------------------------------ 3. replay
@pytest.mark.parametrize("kind,cfg", [(k, c) for k in KINDS for c in (True, False)], ids=lambda v: v if isinstance(v, str) else ("cfg" if v else "nocfg"))
def test_captured_loop_replays_the_eager_bits(ops, kind, cfg):
    """The same 20 steps, eps computation included, captured once on one stream and replayed twice with the latents, the multistep
    buffers and the step counter restored in between: every state tensor has the eager run's bits both times."""
    p = Problem.get(kind, cfg, SHAPES[0], SD)
    loop = Loop(ops, p)
    loop.reset()
    loop.run()
    eager = loop.snapshot()
    loop.reset()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        loop.run()
    for rep in range(2):
        loop.reset()
        g.replay()
        for name, a, b in zip(("latents", "model_in", "step", "m0", "m1", "last"), loop.snapshot(), eager):
            assert _bits(a, b), f"{kind} cfg={int(cfg)} replay {rep}: {name} differs from the eager run"
    assert int(loop.step.item()) == N_STEPS


# ------------------------------------------------------------------------------------------ 4. a second clip on used buffers
@pytest.mark.parametrize("cfg", [True, False], ids=["cfg", "nocfg"])
@pytest.mark.parametrize("kind", ["unipc1", "unipc2"])
def test_second_clip_on_the_same_buffers_equals_a_fresh_run(ops, kind, cfg):
    """`_denoise_fused` resets the latents and the step counter between clips and nothing else: the multistep buffers still hold
    the previous clip's x0-predictions and start sample.  The table's flags keep steps 0 and 1 from reading them."""
    p = Problem.get(kind, cfg, SHAPES[0], SD)
    x2 = Problem.get(kind, cfg, SHAPES[0], SD, seed=1).x_T.to(DEV)
    used = Loop(ops, p)
    used.reset()
    used.run()
    stale = used.snapshot()[3:]
    assert all(float(m.abs().max()) > 0 for m in stale)
    used.reset(x2, zero_ms=False)
    assert all(_bits(a, b) for a, b in zip(used.ms, stale))
    used.run()
    fresh = Loop(ops, p)
    fresh.reset(x2)
    fresh.run()
    for name, a, b in zip(("latents", "model_in", "step", "m0", "m1", "last"), used.snapshot(), fresh.snapshot()):
        assert _bits(a, b), f"{kind} cfg={int(cfg)}: {name} of the second clip depends on the first"


# ------------------------------------------------------------------------------------------ 5. the fused loop follows its prompt
@pytest.fixture(scope="module")
def small():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from diffcodec_amd import selftest as T
    from diffcodec_amd.synthetic import synth_controls, synth_latents
    pipe, _ = T.build_small_pipeline()
    cond, flow = synth_controls(1, 256)
    return T, pipe, dict(controlnet_cond=cond, flow_cond=flow, latents=synth_latents(1, 256), num_inference_steps=2,
                         guidance_scale=4.5, controlnet_conditioning_scale=1.7, output_type="latent")


@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "graphs"])
@pytest.mark.parametrize("which", ["prompt_embeds", "negative_prompt_embeds"])
def test_fused_loop_follows_an_embedding_refilled_in_place(small, which, graphs):
    """A caller that reuses one embedding buffer and refills it with `copy_` passes the same tensor object with another prompt in it.
    The decode has to be the one of that prompt: bitwise the result of a call with a fresh clone (same control tensors, so the
    control cache hits and the decode is deterministic), and not the previous prompt's (PSNR below 40 dB)."""
    T, pipe, kw = small
    from diffcodec_amd.synthetic import synth_text
    dim = T.SMALL_UNET["cross_attention_dim"]
    emb = dict(zip(("prompt_embeds", "negative_prompt_embeds"), synth_text(1, dim=dim)))
    other = synth_text(1, seed=78, dim=dim)[0]
    pipe.enable_hip_graphs(graphs)
    try:
        first = pipe(**emb, **kw).images.float().cpu()
        emb[which].copy_(other)
        second = pipe(**emb, **kw).images.float().cpu()
        fresh = pipe(**dict(emb, **{which: other.clone()}), **kw).images.float().cpu()
    finally:
        pipe.enable_hip_graphs(False)
    assert torch.isfinite(second).all()
    stale, same = T.psnr(second, first), torch.equal(second, fresh)
    assert stale < 40.0, f"{which} refilled in place: the decode is still the previous prompt's ({stale:.1f} dB against it)"
    assert same, f"{which} refilled in place: PSNR against a fresh tensor of the same prompt {T.psnr(second, fresh):.1f} dB"
