"""GPU: every block of tests/block_ref.BLOCK_CASES, built from the package's own classes, against the fp64 restatement of the same
block.  Two figures per case (rel_l2, max|d| / max|ref|, no element excluded), each under 4 x the bf16 emulation's own error
(block_ref.MARGIN); the launches are recorded and the branch each case declares must be the one that ran; two runs give the same
bits; the classifier-free-guidance shared prefix equals the duplicated batch bit for bit.  No fault is injected on the device:
what the bars reject is shown on the CPU (tests/test_block_ref.py)."""
import pytest
import torch

import block_ref as B
from test_block_ref import model_weights

B.set_model_weights(model_weights)
pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16


def nhwc(x):
    """fp64 NCHW values that bf16 holds exactly -> the device's NHWC bf16 tensor"""
    return x.permute(0, 2, 3, 1).contiguous().to(torch.float32).to(BF16).to(DEV)


def nchw64(y):
    return y.detach().to("cpu", torch.float64).permute(0, 3, 1, 2)


class Recorder:
    """lib.call, recorded: the launch names in order and, for each dc_conv_igemm_bf16, the fields of its descriptor and the
    kernel the dispatcher routes it to."""

    def __init__(self, monkeypatch):
        from diffcodec_amd import lib, ops
        self.names, self.convs = [], []
        real = lib.call

        def call(name, *a, **k):
            self.names.append(name)
            if name == "dc_conv_igemm_bf16":
                d = a[0]
                self.convs.append(dict(kernel=ops.conv_instance(d)["kernel"], ksize=d.ksize, stride=d.stride, pad=d.pad,
                                       upsample=d.upsample, C2=d.C2, gn_ab=bool(d.gn_ab), gn_silu=bool(d.gn_silu),
                                       row_add=bool(d.row_add), out_f32=bool(d.out_f32), rows=d.N * d.Ho * d.Wo,
                                       scale=float(d.out_scale), residual=bool(d.residual)))
            return real(name, *a, **k)

        monkeypatch.setattr(lib, "call", call)

    def clear(self):
        del self.names[:], self.convs[:]

    def count(self, name):
        return self.names.count(name)


def f32_sd(sd):
    return {k: v.to(torch.float32) for k, v in sd.items()}


def build_runner(case, sd, inp, monkeypatch):
    """-> run(): the package's block on the case's inputs -> device NHWC output (with its .gn_part, if any)."""
    from diffcodec_amd import blocks, ops, vae
    s, o = case.shape, case.opts
    x = nhwc(inp["x"])
    if case.block in B.MODEL_BLOCKS:
        return build_model_runner(case, sd, inp, x)
    sd = f32_sd(sd)
    if case.block == "resnet":
        rb = blocks.ResnetBlock(sd, B.P_RES, DEV, B.GROUPS, o.get("eps", 1e-5))
        x2 = nhwc(inp["x2"]) if "x2" in inp else None
        if not o.get("temb"):
            return lambda: rb(x, None, x2=x2)
        te = blocks.TimeEmbedding(sd, DEV, 64, [B.P_RES, B.P_NEXT])
        t_dev = torch.tensor([B.TIMESTEP], device=DEV, dtype=torch.float32)
        return lambda: rb(x, te(t_dev, s["n"]), x2=x2)
    if case.block == "transformer":
        monkeypatch.setattr(blocks, "LN_FOLD", o.get("fold", True))
        tb = blocks.TransformerBlock(sd, B.P_TR, DEV, B.HEADS, B.GROUPS)
        tile = s.get("tile", 1)
        ctx = inp["ctx"].to(torch.float32).to(BF16).to(DEV).repeat(tile, 1, 1).contiguous()
        xx = x.repeat(tile, 1, 1, 1).contiguous()
        tb.set_context(ctx)
        if o.get("cfg_shared"):
            half = xx[: xx.shape[0] // 2].contiguous()
            return lambda: tb(half, cfg_shared=True)
        return lambda: tb(xx)
    if case.block in ("down", "up"):
        pc = ops.PackedConv(sd["s.conv.weight"], sd["s.conv.bias"], DEV)
        if case.block == "down":
            return lambda: ops.conv(x, pc, stride=2, gn_part=True)                 # blocks.py EncoderHalf.run_down
        return lambda: ops.conv(x, pc, upsample=True, gn_part=True)                # unet.py / vae.py decode_nhwc
    if case.block == "vae_attention":
        va = vae.VaeAttention(sd, "a.", DEV, B.GROUPS)
        return lambda: va(x)
    if case.block == "vae_mid":
        mid = (blocks.ResnetBlock(sd, "m.resnets.0.", DEV, B.GROUPS, 1e-6), vae.VaeAttention(sd, "m.attentions.0.", DEV, B.GROUPS),
               blocks.ResnetBlock(sd, "m.resnets.1.", DEV, B.GROUPS, 1e-6))
        return lambda: mid[2](mid[1](mid[0](x)))
    if case.block == "vae_up":
        res = [blocks.ResnetBlock(sd, f"u.resnets.{j}.", DEV, B.GROUPS, 1e-6) for j in range(3)]
        pc = ops.PackedConv(sd["u.upsamplers.0.conv.weight"], sd["u.upsamplers.0.conv.bias"], DEV)

        def run():
            y = x
            for r in res:
                y = r(y)
            return ops.conv(y, pc, upsample=True, gn_part=True)
        return run
    if case.block == "vae_down":
        res = [blocks.ResnetBlock(sd, f"d.resnets.{j}.", DEV, B.GROUPS, 1e-6) for j in range(2)]
        pc = ops.PackedConv(sd["d.downsamplers.0.conv.weight"], sd["d.downsamplers.0.conv.bias"], DEV)

        def run():
            y = x
            for r in res:
                y = r(y)
            return ops.conv(y, pc, stride=2, pad=0)
        return run
    raise KeyError(case.block)


def build_model_runner(case, sd, inp, x):
    from diffcodec_amd import vae
    from diffcodec_amd.controlnet import HipDualFlowControlNet
    from diffcodec_amd.rescontrolnet import combine_residuals
    from diffcodec_amd.unet import HipUNet2DConditionModel, as_nchw
    o = case.opts
    if case.block == "vae_decode":
        v = vae.HipAutoencoderKL(f32_sd(sd["vae"]), sd["vae_cfg"], DEV)
        return lambda: v.decode_nhwc(x)
    if case.block == "vae_encode":
        v = vae.HipAutoencoderKL(f32_sd(sd["vae"]), sd["vae_cfg"], DEV)
        return lambda: v.encode_moments_nhwc(x)
    cfg = sd["unet_cfg"]
    ctx = inp["ctx"].to(torch.float32).to(BF16).to(DEV)
    t_dev = torch.tensor([B.TIMESTEP], device=DEV, dtype=torch.float32)
    dummy = torch.zeros(1, device=DEV)

    def make_cn(k, p):
        cn = HipDualFlowControlNet(f32_sd(sd[k]), cfg, DEV)
        pyr = [t.to(torch.float32).to(DEV).contiguous() for t in inp[p]]
        cn.compute_pyramid = lambda *a, **kw: pyr             # the pyramid is an input of the case
        cn.set_context(ctx)
        cn.prepare_controls(dummy, dummy)
        return cn

    if case.block == "controlnet":
        cn = make_cn("cn1", "pyr1")

        def run_cn():
            down, mid = cn.forward_nhwc(x, t_dev, o["scale"])
            return list(down) + [mid]
        return run_cn
    un = HipUNet2DConditionModel(f32_sd(sd["unet"]), cfg, DEV)
    un.set_context(ctx)
    mode = o["mode"]
    if mode == "plain":
        return lambda: un.forward_nhwc(x, t_dev, cfg_shared=bool(o.get("cfg_shared")))
    if mode == "residuals":
        down, mid = [nhwc(d) for d in inp["down_res"]], nhwc(inp["mid_res"])
        return lambda: un.forward_nhwc(x, t_dev, down_res=down, mid_res=mid)
    cns = [make_cn("cn1", "pyr1")] + ([make_cn("cn2", "pyr2")] if mode in ("control2", "combined2") else [])
    if mode == "combined2":
        def run_combined():
            outs = [cn.forward_nhwc(x, t_dev, o["scale"]) for cn in cns]
            outs = [([as_nchw(d) for d in down], as_nchw(mid)) for down, mid in outs]
            down, mid = combine_residuals(outs[0], outs[1])
            return un.forward_nhwc(x, t_dev, down_res=[d.permute(0, 2, 3, 1) for d in down], mid_res=mid.permute(0, 2, 3, 1))
        return run_combined

    def run_control():
        tuples = []
        for cn in cns:
            feats, midf = cn.forward_nhwc(x, t_dev, features_only=True)
            tuples.append((feats, midf, cn.zero, cn.zero_mid, o["scale"]))
        return un.forward_nhwc(x, t_dev, control=tuples[0] if len(tuples) == 1 else tuples)
    return run_control


def check_branches(case, rec):
    """the launches `rec` holds are those of the branches the case declares"""
    s, br = case.shape, case.branches
    n3 = [c for c in rec.convs if c["ksize"] == 3]
    n1 = [c for c in rec.convs if c["ksize"] == 1]
    if case.block == "resnet":
        assert len(n3) == 2 and rec.count("dc_attention_bf16") == 0
        assert n3[0]["row_add"] == ("resnet.temb" in br) and not n3[1]["row_add"]
        assert rec.count("dc_timestep_embedding_f32") == (1 if "temb.batched_slices" in br else 0)
        assert sum(c["out_f32"] for c in rec.convs) == (1 if "temb.batched_slices" in br else 0)       # the one batched time_emb_proj GEMM
        shortcut = [c for c in n1 if c["rows"] == s["n"] * s["h"] * s["w"]]
        assert len(shortcut) == (1 if "resnet.shortcut_conv" in br else 0)
        assert any(c["C2"] > 0 for c in rec.convs) == ("resnet.x2_concat" in br)
        if "resnet.x2_concat" in br:
            assert n3[0]["C2"] == s["c2"] or "conv_gn_silu.standalone_gn_apply" in br       # (the standalone pass resolves the concat)
        if "conv_gn_silu.standalone_gn_apply" in br:
            assert rec.count("dc_gn_apply_nhwc_bf16") == 2 and not any(c["gn_ab"] for c in n3)
        else:
            assert "conv_gn_silu.fused_on_load" in br
            assert rec.count("dc_gn_apply_nhwc_bf16") == 0 and all(c["gn_ab"] and c["gn_silu"] for c in n3)
    if case.block == "transformer":
        first = rec.convs[0]
        if "transformer.proj_in.rowpanel_gn_on_load" in br:
            assert first["kernel"] == "gemm_rowpanel" and first["gn_ab"] and not first["gn_silu"]
            assert rec.count("dc_gn_apply_nhwc_bf16") == 0
        else:
            assert "transformer.proj_in.gn_apply_then_gemm" in br
            assert rec.count("dc_gn_apply_nhwc_bf16") == 1 and not any(c["gn_ab"] for c in rec.convs)
        assert rec.count("dc_layernorm_bf16") == (0 if "transformer.ln_fold" in br else 3)
        assert ("transformer.ln_fold" in br) != ("transformer.ln_standalone" in br)
        assert rec.count("dc_attention_bf16") == (3 if "transformer.cfg_shared" in br else 2)
        assert ("transformer.cfg_shared" in br) != ("transformer.unshared" in br)
    if "gn_ab.direct" in br:
        assert rec.count("dc_gn_direct_nhwc_bf16") >= 1
    if "gn_ab.stats_pass" in br:
        assert rec.count("dc_gn_stats_nhwc_bf16") >= 1 and rec.count("dc_gn_direct_nhwc_bf16") == 0
    if case.block == "down":
        assert [(c["stride"], c["pad"], c["upsample"]) for c in rec.convs] == [(2, 1, 0)]
    if case.block in ("up", "vae_up"):
        assert (rec.convs[-1]["stride"], rec.convs[-1]["upsample"], rec.convs[-1]["ksize"]) == (1, 1, 3)
    if case.block == "vae_down":
        assert (rec.convs[-1]["stride"], rec.convs[-1]["pad"], rec.convs[-1]["ksize"]) == (2, 0, 3)
    if "vae.attention" in br:
        assert rec.count("dc_softmax_rows_f32_to_bf16") == s["n"] and rec.count("dc_transpose_bf16") == 1
    if case.block == "vae_mid":
        assert len(n3) == 4
    if case.block == "vae_up":
        assert len(n3) == 7
    if case.block in B.MODEL_BLOCKS:
        check_model_branches(case, rec)


def check_model_branches(case, rec):
    br, o = case.branches, case.opts
    down2 = [c for c in rec.convs if c["ksize"] == 3 and c["stride"] == 2]
    ups = [c for c in rec.convs if c["upsample"]]
    scaled = [c for c in rec.convs if c["ksize"] == 1 and abs(c["scale"] - o.get("scale", 0.0)) < 1e-6]
    nets = 2 if o.get("mode") in ("control2", "combined2") else (0 if o.get("mode") in ("plain", "residuals") else 1)
    if case.block == "vae_decode":
        assert len(ups) == 3 and not down2 and rec.convs[-1]["out_f32"] and rec.convs[-1]["gn_ab"] and rec.convs[-1]["kernel"] != "igemm"
        assert rec.count("dc_conv_small_cin_bf16") == 2 and rec.count("dc_conv_small_cout_bf16") == 0
        return
    if case.block == "vae_encode":
        assert [c["pad"] for c in down2] == [0, 0, 0] and not ups
        assert rec.count("dc_conv_small_cin_bf16") == 2 and rec.count("dc_conv_small_cout_bf16") == 1
        return
    assert rec.count("dc_fdn_modulate_nhwc_bf16") == 5 * nets                    # fdn64 and the four hooks (fdn08 twice) per ControlNet
    assert rec.count("dc_timestep_embedding_f32") == nets + (case.block == "unet")
    if case.block == "controlnet":
        assert len(down2) == 3 and not ups and len(scaled) == 13 and not any(c["residual"] for c in scaled)
        assert rec.count("dc_attention_bf16") == 14
        return
    assert len(down2) == 3 * (1 + nets) and len(ups) == 3 and all(c["pad"] == 1 for c in down2)
    assert rec.count("dc_attention_bf16") == 14 * nets + 32 + (1 if "run_down.cfg_shared" in br else 0)
    assert ("run_down.cfg_shared" in br) != ("run_down.unshared" in br)
    adds = rec.count("dc_add_bf16")
    if "unet.plain" in br:
        assert adds == 0 and not scaled
    if "unet.residuals_added" in br:
        combined = "rescontrolnet.combine_residuals" in br
        assert adds == (26 if combined else 13)
        assert len(scaled) == (26 if combined else 0) and not any(c["residual"] for c in scaled)
    if "unet.control_one" in br or "unet.control_two" in br:
        assert adds == 0 and len(scaled) == 13 * nets and all(c["residual"] for c in scaled)
    assert any(c["C2"] > 0 for c in rec.convs) and rec.convs[-1]["out_f32"] and rec.convs[-1]["gn_ab"]


def same_bits(a, b):
    if isinstance(a, list):
        return len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))
    if not (a.shape == b.shape and torch.equal(a, b)):
        return False
    pa, pb = getattr(a, "gn_part", None), getattr(b, "gn_part", None)
    return (pa is None) == (pb is None) and (pa is None or (pa.shape == pb.shape and torch.equal(pa, pb)))


@pytest.mark.parametrize("case", B.BLOCK_CASES, ids=[c.name for c in B.BLOCK_CASES])
def test_block_against_fp64_under_four_times_the_bf16_emulation(case, monkeypatch, record):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    rb = B.reference_and_bars(case)
    run = build_runner(case, rb["sd"], rb["inp"], monkeypatch)
    rec = Recorder(monkeypatch)
    y = run()
    torch.cuda.synchronize()
    check_branches(case, rec)
    # two runs, same bits
    y2 = run()
    assert same_bits(y, y2)
    ys = y if isinstance(y, list) else [y]
    outs = [nchw64(t) for t in ys]
    n = case.shape["n"]
    if case.shape.get("tile", 1) > 1:                        # every copy of a sample carries the bits of the first
        for i in range(n, ys[0].shape[0]):
            assert torch.equal(ys[0][i], ys[0][i % n]), i
        outs = [outs[0][:n]]
    assert len(outs) == len(rb["ref"])
    worst = 0.0
    for k, (out, ref, emu, bars) in enumerate(zip(outs, rb["ref"], rb["emu_figs"], rb["bars"])):
        assert out.shape == ref.shape
        figs = B.figures(out, ref)
        tag = f"blocks/{case.name}" + (f"/{k}" if len(outs) > 1 else "")
        for name, f, e, bar in zip(("rel_l2", "max_rel"), figs, emu, bars):
            print(f"{tag}/{name}\tdevice {f:.3e}\temulation {e:.3e}\tbar {bar:.3e}")
            record(f"{tag}/{name}", f"{f:.4e}\t{e:.4e}")
            worst = max(worst, f / bar)
    assert worst <= 1.0, worst
    if case.opts.get("cfg_shared"):                          # the shared prefix equals the duplicated batch, partials included
        assert same_bits(y, build_runner(case._replace(opts=dict(case.opts, cfg_shared=False)), rb["sd"], rb["inp"], monkeypatch)())
