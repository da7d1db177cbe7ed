"""CPU: tests/block_ref.py is (1) the oracle — its fp64 restatement equals oracle/sd15_ref.py cast to fp64 on every case; (2) sharp —
every named wiring fault misses some case's bar (4 x the bf16 emulation's own error) by a factor of at least 2; (3) complete over
the branches it lists — every branch has a case, removing a sole case names the branch, and the shape predicates that select a
branch agree with what each case declares and with the package's own constants and routes."""
import pytest
import torch
import torch.nn.functional as F

import abi_check as A
import block_ref as B
from oracle import sd15_ref as M

F64 = torch.float64
LIGHT = [c for c in B.BLOCK_CASES if c.name not in B.HEAVY]


def model_weights():
    """selftest's reduced-width configurations with weights.synthesize; a second ControlNet from another seed"""
    from diffcodec_amd import selftest as T
    from diffcodec_amd import weights as W
    usd, csd, vsd = T.small_state_dicts()
    return dict(unet=usd, cn1=csd, cn2=W.synthesize(W.controlnet_spec(T.SMALL_UNET), 11), vae=vsd, unet_cfg=T.SMALL_UNET,
                vae_cfg=T.SMALL_VAE)


B.set_model_weights(model_weights)


# ------------------------------------------------------------------------------------------ pinned to the oracle
def _oracle(case, sd, inp, monkeypatch):
    s, o = case.shape, case.opts
    x = inp["x"]
    sinus = M.timestep_embedding                            # fp32 by construction: widen its result, keep its arithmetic
    monkeypatch.setattr(M, "timestep_embedding", lambda t, dim: sinus(t, dim).to(F64))
    if case.block == "vae_decode":
        return M.vae_decode(sd["vae"], sd["vae_cfg"], x)
    if case.block == "vae_encode":
        mean, logvar = M.vae_encode_moments(sd["vae"], sd["vae_cfg"], x)
        assert float(logvar.min()) > -30 and float(logvar.max()) < 20       # the clamp is idle: the device returns raw moments
        return torch.cat([mean, logvar], 1)
    if case.block in ("controlnet", "unet"):
        cfg, ctx, t = sd["unet_cfg"], inp["ctx"], B.TIMESTEP

        def cn(k, p):
            return M.dualflow_controlnet_forward(sd[k], cfg, x, t, ctx, None, None, o["scale"], pyramid=inp[p])

        if case.block == "controlnet":
            down, mid = cn("cn1", "pyr1")
            return down + [mid]
        mode = o["mode"]
        if mode == "plain":
            return M.unet_forward(sd["unet"], cfg, x, t, ctx)
        if mode == "residuals":
            return M.unet_forward(sd["unet"], cfg, x, t, ctx, inp["down_res"], inp["mid_res"])
        down, mid = cn("cn1", "pyr1")
        if mode in ("control2", "combined2"):                # the package's rule for two ControlNets: their residuals add
            d2, m2 = cn("cn2", "pyr2")
            down, mid = [a + b for a, b in zip(down, d2)], mid + m2
        return M.unet_forward(sd["unet"], cfg, x, t, ctx, down, mid)
    if case.block == "resnet":
        temb = None
        if o.get("temb"):
            temb = M.time_embed(sd, B.TIMESTEP, s["n"], 64)
        xin = x if "x2" not in inp else torch.cat([x, inp["x2"]], 1)
        return M.resnet(sd, B.P_RES, xin, temb, B.GROUPS, o.get("eps", 1e-5))
    if case.block == "transformer":                          # one sample at a time: the 64x64 case's scores are 1 GiB per sample
        return torch.cat([M.transformer(sd, B.P_TR, x[i:i + 1], inp["ctx"][i:i + 1], B.HEADS, B.GROUPS) for i in range(x.shape[0])], 0)
    if case.block == "down":
        return M._conv(sd, "s.conv", x, stride=2)
    if case.block == "up":
        return M._conv(sd, "s.conv", F.interpolate(x, scale_factor=2.0, mode="nearest"))
    if case.block == "vae_attention":
        return M._vae_attn(sd, "a.", x, B.GROUPS)
    if case.block == "vae_mid":
        return M._vae_mid(sd, "m.", x, B.GROUPS)
    if case.block == "vae_up":                               # the loop body of M.vae_decode
        for j in range(3):
            x = M.resnet(sd, f"u.resnets.{j}.", x, None, B.GROUPS, 1e-6)
        return M._conv(sd, "u.upsamplers.0.conv", F.interpolate(x, scale_factor=2.0, mode="nearest"))
    if case.block == "vae_down":                             # the loop body of M.vae_encode_moments
        for j in range(2):
            x = M.resnet(sd, f"d.resnets.{j}.", x, None, B.GROUPS, 1e-6)
        return M._conv(sd, "d.downsamplers.0.conv", F.pad(x, (0, 1, 0, 1)), stride=2, padding=0)
    raise KeyError(case.block)


@pytest.mark.parametrize("case", B.BLOCK_CASES, ids=[c.name for c in B.BLOCK_CASES])
def test_identity_restatement_is_the_oracle(case, monkeypatch):
    rb = B.reference_and_bars(case)
    ora = _oracle(case, rb["sd"], rb["inp"], monkeypatch)
    ora = ora if isinstance(ora, list) else [ora]
    assert len(ora) == len(rb["ref"])
    for o_, r_ in zip(ora, rb["ref"]):
        assert o_.dtype == F64 and o_.shape == r_.shape
        rel_l2, max_rel = B.figures(r_, o_)
        assert rel_l2 <= 1e-12 and max_rel <= 1e-12, (rel_l2, max_rel)
    # the emulation differs from the reference (it rounds), by a few bf16 roundings per output of a block and by no more than
    # a few percent after the some sixty launches of a whole model
    lim = (0.08, 0.08) if case.block in B.MODEL_BLOCKS else (2.0 ** -5, 2.0 ** -4)
    for e0, e1 in rb["emu_figs"]:
        assert 0 < e0 < lim[0] and 0 < e1 < lim[1], rb["emu_figs"]


# ------------------------------------------------------------------------------------------ sharpness
def rejection_factor(fault):
    """(factor, case name): the largest figure / bar of the faulted fp64 restatement over the cases the fault applies to."""
    best = (0.0, None)
    for case in LIGHT:
        if not B.fault_applies(fault, case):
            continue
        rb = B.reference_and_bars(case)
        outs = B.run_case(case, rb["sd"], rb["inp"], B.ident, fault)
        factor = max(max(f / bar for f, bar in zip(B.figures(y, r), bars)) for y, r, bars in zip(outs, rb["ref"], rb["bars"]))
        if factor > best[0]:
            best = (factor, case.name)
    return best


@pytest.mark.parametrize("fault", sorted(B.FAULTS))
def test_every_fault_misses_a_bar_by_a_factor_of_two(fault):
    factor, name = rejection_factor(fault)
    print(f"{fault}\trejected by {factor:.1f} x the bar on {name}")
    assert name is not None, "no case takes this fault"
    assert factor >= 2.0, (fault, factor, name)


def test_a_fault_is_refused_where_it_cannot_show():
    case = B.CASES["down_128_b2_12x12"]
    rb = B.reference_and_bars(case)
    with pytest.raises(ValueError):
        B.run_case(case, rb["sd"], rb["inp"], B.ident, "no_temb")


# ------------------------------------------------------------------------------------------ coverage
def uncovered(cases):
    have = set().union(*(c.branches for c in cases)) if cases else set()
    return sorted(set(B.BRANCHES) - have)


def test_every_branch_has_a_case_and_every_case_a_listed_branch():
    assert uncovered(B.BLOCK_CASES) == []
    for c in B.BLOCK_CASES:
        assert c.branches and c.branches <= set(B.BRANCHES), c.name
    assert not set(B.UNREACHABLE) & set(B.BRANCHES)
    assert len(B.CASES) == len(B.BLOCK_CASES)                # names are unique


def test_removing_the_sole_case_of_a_branch_names_it():
    count = {}
    for c in B.BLOCK_CASES:
        for br in c.branches:
            count[br] = count.get(br, 0) + 1
    sole = 0
    for i, c in enumerate(B.BLOCK_CASES):
        mine = sorted(br for br in c.branches if count[br] == 1)
        if mine:
            sole += 1
            assert uncovered(B.BLOCK_CASES[:i] + B.BLOCK_CASES[i + 1:]) == mine
    assert sole > 0


@pytest.mark.parametrize("case", B.BLOCK_CASES, ids=[c.name for c in B.BLOCK_CASES])
def test_shape_predicates_select_the_declared_branches(case):
    assert B.predicted_branches(case) == set(case.branches)


def test_the_unreachable_branch_is_unreachable():
    from diffcodec_amd import blocks
    assert blocks.PROJ_IN_FUSE_MIN_ROWS >= 1 << 62 and blocks.PROJ_IN_GN_ON_LOAD and blocks.LN_FOLD


def test_restated_predicates_are_the_package_s():
    from diffcodec_amd import ops
    assert (B.FUSE_GN_MAX_COUT, B.FUSE_GN_SMALL_BATCH, B.GN_DIRECT_MAX_PIXELS) == \
        (ops.FUSE_GN_MAX_COUT, ops.FUSE_GN_SMALL_BATCH, ops.GN_DIRECT_MAX_PIXELS)
    for rows_per_sample in (64, 240, 256, 1024, 4096):
        for n in (1, 2, 16, 32, 64, 256):
            for cin, cout in ((320, 320), (320, 960), (320, 2560), (64, 64), (640, 640), (320, 160)):
                a = (n * rows_per_sample, rows_per_sample, cin, cout)
                assert B.rowpanel_takes(*a) == ops.rowpanel_takes(*a), a


def test_attention_form_mirror_agrees_with_the_route():
    """R7 depends on the SHORT form: the mirror B.attn_short is held to the library's route on every attention shape of the table"""
    lib = A.built_lib()
    from diffcodec_amd import ops
    assert lib is not None
    for case in B.BLOCK_CASES:
        if case.block != "transformer":
            continue
        s = case.shape
        n, hw, d = s["n"] * s.get("tile", 1), s["h"] * s["w"], s["c"] // B.HEADS
        if case.opts.get("cfg_shared"):
            shapes = [(n // 2, hw, hw), (n // 2, hw, B.CTX_LEN)]            # each half is a launch of its own
        else:
            shapes = [(n, hw, hw), (n, hw, B.CTX_LEN)]
        for b, nq, nk in shapes:
            assert B.attn_short(b, B.HEADS, nq, nk, d) == ops.attention_route(b, B.HEADS, nq, nk, d).short, (case.name, b, nq, nk, d)
