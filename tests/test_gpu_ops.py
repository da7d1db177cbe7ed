"""GPU parity: every C-ABI launcher against the CPU oracle / a plain torch fp32 reference of the same op, on the
same seeded inputs.  bf16 kernels: inputs are bf16-rounded first so the fp32 reference sees identical operands;
tolerance then covers fp32-accumulation order + one bf16 rounding of the output (rel 2^-8)."""
import math

import pytest
import torch
import torch.nn.functional as F

from launch_shadow import capture_routes
from oracle import launch_ref as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from diffcodec_amd import ops as o
    return o


DEV = "cuda"


def bf(x):
    return x.to(torch.bfloat16).float()


def nhwc(x):  # NCHW fp32 cpu -> NHWC bf16 device
    return x.permute(0, 2, 3, 1).contiguous().to(DEV, torch.bfloat16)


def from_nhwc(y):
    return y.float().cpu().permute(0, 3, 1, 2)


def close(a, b, rtol=2e-2, atol=2e-2):
    torch.testing.assert_close(a, b, rtol=rtol, atol=atol)


# ------------------------------------------------------------------------------------------- splat stage
def test_splat_soft_matches_oracle(ops):
    from oracle import splat as S
    g = torch.Generator().manual_seed(0)
    for (n, c, h, w) in [(1, 3, 9, 11), (2, 21, 32, 32), (2, 161, 64, 64)]:
        x = torch.randn(n, c, h, w, generator=g)
        flow = torch.randn(n, 2, h, w, generator=g) * 3
        flow[0, 0, 0, 0] = float("inf")
        flow[-1, 1, 1, 2] = float("nan")
        m = torch.randn(n, 1, h, w, generator=g) * 0.5
        mask = (torch.rand(n, 1, h, w, generator=g) > 0.5).float()
        ref = S.softsplat(x, flow, m, "soft") * (1 - mask)
        out = ops.splat_soft(x.to(DEV), flow.to(DEV), m.to(DEV), mask.to(DEV)).cpu()
        close(out, ref, rtol=1e-4, atol=1e-5)      # fp32; same summation order, device expf vs libm expf
        v = L.check(out.to(DEV), *L.splat_soft_ref(x.to(DEV), flow.to(DEV), m.to(DEV), mask.to(DEV))[:2], torch.float32)
        assert v["ok"], v                          # ... and the derived fp32 bound against the fp64 reference
        assert torch.equal(out, ops.splat_soft(x.to(DEV), flow.to(DEV), m.to(DEV), mask.to(DEV)).cpu())   # run-to-run bit-identical
        ref_sum = S.splat_sum(x, flow)
        # 'sum' mode has no transcendental: the gather adds every target's sources in ascending raster order with un-contracted
        # fp32 operations, i.e. exactly the sequential oracle's arithmetic -> bit-exact
        assert torch.equal(ops.splat_sum(x.to(DEV), flow.to(DEV)).cpu(), ref_sum)


def test_splat_pathological_flows(ops):
    """Every source landing in one cell (a k-way collision: the rank pass and the 4-way merge see long segments), everything
    leaving the map, landing points exactly on the map border, and a non-square map: bit-exact against the sequential oracle."""
    from oracle import splat as S
    g = torch.Generator().manual_seed(7)
    n, c, h, w = 2, 5, 24, 40
    x = torch.randn(n, c, h, w, generator=g)
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    collapse = torch.stack([7.25 - xs, 3.5 - ys])[None].repeat(n, 1, 1, 1)                 # all 960 sources -> (7.25, 3.5)
    away = torch.full((n, 2, h, w), 1.0e4)
    away[1, :, 5, 6] = torch.tensor([float(w - 1 - 6), float(h - 1 - 5)])                # one source exactly onto the last pixel
    edge = torch.stack([-1.0 - xs + (xs % 3) * 0.5, -0.5 - ys + (ys % 2)])[None].repeat(n, 1, 1, 1)   # columns -1 .. 0, rows -0.5 / 0.5
    smooth = torch.randn(n, 2, h, w, generator=g) * 1.5
    for flow in (collapse, away, edge, smooth):
        out = ops.splat_sum(x.to(DEV), flow.to(DEV)).cpu()
        assert torch.equal(out, S.splat_sum(x, flow))
        m = torch.randn(n, 1, h, w, generator=g)
        soft = ops.splat_soft(x.to(DEV), flow.to(DEV), m.to(DEV))
        close(soft.cpu(), S.softsplat(x, flow, m, "soft"), rtol=1e-4, atol=1e-5)
        v = L.check(soft, *L.splat_soft_ref(x.to(DEV), flow.to(DEV), m.to(DEV))[:2], torch.float32)
        assert v["ok"], v


def test_splat_fully_collapsed_flow_is_bounded(ops):
    """the deterministic gather ranks a cell's sources by counting (k^2 compares for a k-way collision) and one thread
    walks a target's whole source list.  Worst case: EVERY source of a full-size 512x512 map lands in one cell (k = 262,144:
    7e10 compares, four targets x C threads walking 262,144-long lists).  All lanes of a wave read the same list element, so the
    rank pass is one broadcast load per step and the job stays in the tens of milliseconds — asserted here with a wide margin
    (a slow-down to seconds would make a pathological flow look like a hang on a shared box), still bit-exact with the oracle."""
    import time
    from oracle import splat as S
    h = w = 512
    g = torch.Generator().manual_seed(3)
    x = torch.randn(1, 3, h, w, generator=g)
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    flow = torch.stack([200.25 - xs, 100.5 - ys])[None].contiguous()
    xd, fd = x.to(DEV), flow.to(DEV)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = ops.splat_sum(xd, fd)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert dt < 3.0, f"collapsed 512x512 splat took {dt:.2f} s"
    assert torch.equal(out.cpu(), S.splat_sum(x, flow))


def test_occlusion_mask_and_flow_resize(ops):
    from oracle import control_ref as C
    g = torch.Generator().manual_seed(1)
    flow = torch.randn(2, 4, 128, 128, generator=g) * 6
    for r in (16, 8, 32):
        ref = C.resize_and_normalize_flow(flow[:, :2], r, r)
        out = ops.flow_resize_normalize(flow.to(DEV)[:, :2], r, r).cpu()
        close(out, ref, rtol=1e-5, atol=1e-5)
        ref2 = C.resize_and_normalize_flow(flow[:, 2:], r, r)
        close(ops.flow_resize_normalize(flow.to(DEV)[:, 2:], r, r).cpu(), ref2, rtol=1e-5, atol=1e-5)
    fa = torch.randn(2, 2, 32, 32, generator=g) * 0.6
    fb = -fa + 0.25 * torch.randn(2, 2, 32, 32, generator=g)
    ref = C.compute_mask(fa, fb)
    out = ops.occlusion_mask(fa.to(DEV), fb.to(DEV)).cpu()
    # threshold compare: allow disagreement only where the norm is within 1e-4 of 0.3
    assert (out != ref).float().mean().item() < 2e-3
    v = L.check_occlusion_mask(out, L.occlusion_mask_ref(fa, fb))      # no disagreement outside the fp64 reference's own band
    assert v["ok"] and v["band"] <= 0.005, v
    assert 0.05 < ref.mean() < 0.95


def test_fuse_warped(ops):
    g = torch.Generator().manual_seed(2)
    n, c, h, w = 2, 7, 8, 8
    wf, wl = torch.randn(n, c, h, w, generator=g), torch.randn(n, c, h, w, generator=g)
    cf, cb = torch.randn(n, 1, h, w, generator=g), torch.randn(n, 1, h, w, generator=g)
    of, ob = (torch.rand(n, 1, h, w, generator=g) > 0.5).float(), (torch.rand(n, 1, h, w, generator=g) > 0.5).float()
    conf = torch.clamp(torch.cat([cf, cb], 1), min=0)
    wn = conf / (conf.sum(1, keepdim=True) + 1e-6)
    ref = wn[:, :1] * wf + wn[:, 1:] * wl
    ref = torch.where(((of + ob) > 1.5).expand_as(ref), 0.5 * (wf + wl), ref)
    out = ops.fuse_warped(*(t.to(DEV) for t in (wf, wl, cf, cb, of, ob))).cpu()
    close(out, ref, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("cin,cout,hw,stride,silu", [(3, 16, 40, 1, True), (16, 32, 33, 2, True), (64, 160, 16, 2, True),
                                                      (160, 64, 8, 1, True), (64, 1, 8, 1, False), (80, 160, 8, 1, False),
                                                      # larger maps: ragged tiles, Cout < 16, stride 2
                                                      (3, 16, 70, 1, True), (20, 40, 67, 2, False), (16, 1, 64, 1, False),
                                                      # the register-blocked form (>= 64 output channels, wide maps): ragged map,
                                                      # ragged channel tile, stride 2 at 34 wide with 160 channels
                                                      (32, 64, 70, 1, True), (16, 80, 64, 1, False), (24, 160, 67, 2, False)])
def test_conv3x3_nchw_f32(ops, cin, cout, hw, stride, silu):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, cin + 2, hw, hw, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(cin * 9)
    b = torch.randn(cout, generator=g) * 0.1
    xs = x[:, 1:1 + cin]                                  # channel-slice view, like cond[:, 3:]
    ref = F.conv2d(xs, w, b, stride=stride, padding=1)
    if silu:
        ref = F.silu(ref)
    pc = ops.PackedConvF32(w, b, DEV)
    out = ops.conv3x3_nchw_f32(x.to(DEV)[:, 1:1 + cin], pc, stride=stride, silu=silu).cpu()
    close(out, ref, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("cin,cout,hw,stride", [
    (16, 32, 512, 2),      # 256-wide output: 1 x 128 pixel tiles, the widest stride-2 patch (3 x 257)
    (32, 32, 256, 1),      # 1 x 128 tiles, 32-channel tile
    (32, 64, 64, 2),       # 32-wide output: 4 x 32 tiles
    (64, 64, 128, 1),
    (64, 160, 128, 2),     # Cout = 160: 32-channel tiles
    (160, 160, 64, 2),
    (160, 320, 64, 1),     # 2 x 64 tiles
    (160, 320, 32, 1),
    (160, 320, 32, 2),     # 16-wide output: 8 x 16 tiles
    (320, 640, 16, 2),     # 8x8 output: the 64-pixel tile
    (640, 1280, 8, 1),
    (640, 64, 8, 1),
    (320, 64, 16, 1),
    (24, 96, 16, 1),       # Cin not a multiple of 16 (three 8-channel chunks)
])
def test_conv3x3_nchw_f32_mfma_form(ops, cin, cout, hw, stride):
    """The extractor layers that take the exact-fp32 MFMA kernel (csrc/conv_f32_mfma.hip: Cin >= 16 in 8-channel chunks, Cout in
    32-wide tiles, whole pixel tiles) — every pyramid shape of extractors.py:215-262 at its true map size — against F.conv2d in
    fp32.  The instruction is a k-ordered fmaf chain: same 1e-4 bar as the VALU kernels, and bit-identical run to run."""
    g = torch.Generator().manual_seed(11)
    n = 2 if hw <= 256 else 1
    x = torch.randn(n, cin + 2, hw, hw, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(cin * 9)
    b = torch.randn(cout, generator=g) * 0.1
    ref = F.silu(F.conv2d(x[:, 1:1 + cin], w, b, stride=stride, padding=1))
    pc = ops.PackedConvF32(w, b, DEV)
    xd = x.to(DEV)[:, 1:1 + cin]                          # channel-slice view (batch stride != Cin*H*W), like cond[:, 3:]
    out = ops.conv3x3_nchw_f32(xd, pc, stride=stride, silu=True)
    close(out.cpu(), ref, rtol=1e-4, atol=1e-4)
    assert torch.equal(out, ops.conv3x3_nchw_f32(xd, pc, stride=stride, silu=True))
    ref_lin = F.conv2d(x[:, 1:1 + cin], w, None, stride=stride, padding=1)        # no bias, no SiLU
    close(ops.conv3x3_nchw_f32(xd, ops.PackedConvF32(w, None, DEV), stride=stride, silu=False).cpu(), ref_lin, rtol=1e-4, atol=1e-4)


# ------------------------------------------------------------------------------------------- igemm
CONV_CASES = [
    # n, h, w, c1, c2, cout, k, stride, pad, upsample
    (2, 16, 16, 64, 0, 64, 3, 1, 1, False),
    (2, 16, 16, 128, 0, 160, 3, 1, 1, False),
    (1, 13, 9, 64, 0, 48, 3, 1, 1, False),          # ragged M, Cout not a tile multiple
    (2, 16, 16, 64, 64, 128, 3, 1, 1, False),       # channel concat
    (2, 16, 16, 128, 0, 128, 3, 2, 1, False),       # stride 2
    (1, 16, 16, 64, 0, 64, 3, 2, 0, False),         # asymmetric pad (VAE encoder)
    (1, 8, 8, 64, 0, 128, 3, 1, 1, True),           # fused nearest-2x upsample
    (2, 16, 16, 320, 0, 320, 3, 1, 1, True),        # Upsample2D conv on the pipelined path: 4-row tiles (too few for 8-row ones), 160-column tiles, four-slot ring
    (20, 16, 24, 128, 0, 320, 3, 1, 1, True),       # the same with > 256 workgroups (two-slot ring), non-square map
    (3, 10, 8, 192, 0, 256, 3, 1, 1, True),         # 4-row tiles (Ho = 20), 128-column tiles
    (2, 8, 8, 320, 0, 320, 1, 1, 1, False),         # 1x1
    (2, 64, 64, 320, 0, 320, 3, 1, 1, False),       # UNet 64x64 ResBlock conv (halo-tile path, 4-row tiles; <= 256 workgroups: four-slot weight ring)
    (10, 64, 64, 128, 64, 320, 3, 1, 1, False),     # the same path with > 256 workgroups: 8-row tiles, two-slot ring, two workgroups per CU, skip concat
    (9, 32, 16, 192, 0, 256, 3, 1, 1, False),       # 128-column tiles, 4-row tiles, batch not a power of two
    (2, 8, 8, 1280, 1280, 1280, 3, 1, 1, False),    # UNet 8x8 up-block conv (split-K path)
    # weight-stationary tile order (round 4: pixel tile fastest inside an XCD where Cout * 9 > N * H * W) on grids that are not a multiple of 8
    (3, 8, 8, 640, 0, 1280, 3, 1, 1, False),        # 8x8, odd batch: 4-row tiles, 3 x 8 N tiles
    (6, 8, 8, 320, 0, 1280, 3, 1, 1, False),        # 8x8, even batch, split-K 5: too few tiles for two images per tile, 4-row tiles
    (5, 16, 16, 320, 0, 1280, 3, 1, 1, False),      # 16x16: 5 x 2 pixel tiles x 8 N tiles
    (1, 16, 16, 256, 0, 640, 3, 1, 1, True),        # fused upsample (16x16 -> 32x32) in the new order
]


# (kernel, variant) dc_conv_route reports for each case above: conv3x3_tile variant = tile rows (2: 4-row tiles, 4: 8-row tiles,
# 8: two 8x8 images per tile), igemm 24 = the 64 x 128 gather-GEMM tile, gemm_dma 25201 = its 64-row tile with the deep ring
CONV_ROUTES = [("conv3x3_tile", 2), ("conv3x3_tile", 2), ("igemm", 24), ("conv3x3_tile", 2), ("igemm", 24), ("igemm", 24),
               ("conv3x3_tile", 2), ("conv3x3_tile", 2), ("conv3x3_tile", 2), ("conv3x3_tile", 2), ("gemm_dma", 25201),
               ("conv3x3_tile", 2), ("conv3x3_tile", 4), ("conv3x3_tile", 2), ("conv3x3_tile", 2), ("conv3x3_tile", 2),
               ("conv3x3_tile", 2), ("conv3x3_tile", 2), ("conv3x3_tile", 2)]


@pytest.mark.parametrize("case", CONV_CASES)
def test_conv_igemm_plain(ops, case):
    n, h, w, c1, c2, cout, k, stride, pad, up = case
    g = torch.Generator().manual_seed(4)
    x1 = bf(torch.randn(n, c1, h, w, generator=g))
    x2 = bf(torch.randn(n, c2, h, w, generator=g)) if c2 else None
    cin = c1 + c2
    wt = bf(torch.randn(cout, cin, k, k, generator=g) / math.sqrt(cin * k * k))
    b = torch.randn(cout, generator=g) * 0.1
    xin = torch.cat([x1, x2], 1) if c2 else x1
    if up:
        xin = F.interpolate(xin, scale_factor=2.0, mode="nearest")
    if k == 3 and pad == 0:
        xin = F.pad(xin, (0, 1, 0, 1))
    ref = F.conv2d(xin, wt, b, stride=stride, padding=(1 if (k == 3 and pad) else 0))
    pc = ops.PackedConv(wt, b, DEV)
    with capture_routes() as routes:
        out = ops.conv(nhwc(x1), pc, x2=None if x2 is None else nhwc(x2), stride=stride, pad=pad, upsample=up)
    assert [(r.kernel, r.variant) for r in routes] == [CONV_ROUTES[CONV_CASES.index(case)]], routes
    close(from_nhwc(out), ref)
    _strict(out, lambda rows: L.conv_ref(nhwc(x1), pc, rows, x2=None if x2 is None else nhwc(x2), stride=stride, pad=pad, upsample=up),
            spatial=(out.shape[0], out.shape[1], out.shape[2]) if k == 3 else None)


def _strict(y, ref_fn, spatial=None):
    """the launch's output held to its fp64 reference (oracle/launch_ref.py) on the sampled rows, beside the torch comparison"""
    c = y.shape[-1]
    rows = L.sample_rows(y.numel() // c, spatial=spatial)
    r, s = ref_fn(rows)
    v = L.check(y.reshape(-1, c)[rows.to(y.device)], r, s, y.dtype)
    assert v["ok"], v


def test_conv_igemm_asymmetric_operands(ops):
    """A = identity-like weights with asymmetric data: catches a transposed / permuted fragment map."""
    n, h, w, c = 1, 8, 16, 64
    x = torch.arange(n * c * h * w, dtype=torch.float32).reshape(n, c, h, w) % 251 - 125
    wt = torch.zeros(64, c, 1, 1)
    for o in range(64):
        wt[o, (o * 7 + 3) % c, 0, 0] = 1.0 + (o % 5)
    ref = F.conv2d(x, wt)
    out = ops.conv(nhwc(x), ops.PackedConv(wt, None, DEV))
    assert torch.equal(from_nhwc(out), bf(ref))     # exact: integers below 2^8 scale


@pytest.mark.parametrize("n,h,w", [(2, 16, 16), (3, 8, 8), (2, 32, 32), (1, 12, 20)])
def test_conv_igemm_fused_epilogues(ops, n, h, w):
    g = torch.Generator().manual_seed(5)
    cin, cout = 128, 160
    x = bf(torch.randn(n, cin, h, w, generator=g))
    wt = bf(torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(cin * 9))
    b = torch.randn(cout, generator=g) * 0.1
    temb = torch.randn(n, cout, generator=g)
    res = bf(torch.randn(n, cout, h, w, generator=g))
    gamma, beta = 1 + 0.1 * torch.randn(cin, generator=g), 0.1 * torch.randn(cin, generator=g)
    # reference: GN -> SiLU -> (bf16 operand) -> conv -> +bias +temb -> *scale -> +res
    y = F.silu(F.group_norm(x, 32, gamma, beta, 1e-5))
    ref = (F.conv2d(bf(y), wt, b, padding=1) + temb[:, :, None, None]) * 0.75 + res
    xd = nhwc(x)
    ab = ops.group_norm_ab(xd, gamma.to(DEV), beta.to(DEV), 32, 1e-5)
    out = ops.conv(xd, ops.PackedConv(wt, b, DEV), gn_ab=ab, gn_silu=True, row_add=temb.to(DEV), residual=nhwc(res), out_scale=0.75)
    close(from_nhwc(out), ref, rtol=3e-2, atol=3e-2)
    out32 = ops.conv(xd, ops.PackedConv(wt, b, DEV), gn_ab=ab, gn_silu=True, row_add=temb.to(DEV), residual=nhwc(res),
                     out_scale=0.75, out_f32=True)
    close(out32.cpu().permute(0, 3, 1, 2), ref, rtol=2e-2, atol=2e-2)
    # forced split-K gives the same answer
    outk = ops.conv(xd, ops.PackedConv(wt, b, DEV), gn_ab=ab, gn_silu=True, row_add=temb.to(DEV), residual=nhwc(res),
                    out_scale=0.75, splitk=3)
    close(from_nhwc(outk), ref, rtol=3e-2, atol=3e-2)


def test_linear_and_geglu(ops):
    g = torch.Generator().manual_seed(6)
    m, c = 300, 320
    x = bf(torch.randn(2, m, c, generator=g))
    w1 = bf(torch.randn(8 * c, c, generator=g) / math.sqrt(c))
    b1 = torch.randn(8 * c, generator=g) * 0.1
    hg = F.linear(x, w1, b1)
    hid, gate = hg.chunk(2, -1)
    ref = hid * F.gelu(gate)
    out = ops.linear(x.to(DEV, torch.bfloat16), ops.PackedConv(w1, b1, DEV, geglu=True))
    assert out.shape == (2, m, 4 * c)
    close(out.float().cpu(), ref)
    w2 = bf(torch.randn(c, 4 * c, generator=g) / math.sqrt(4 * c))
    res = bf(torch.randn(2, m, c, generator=g))
    ref2 = F.linear(bf(ref), w2) + res
    out2 = ops.linear(out, ops.PackedConv(w2, None, DEV), residual=res.to(DEV, torch.bfloat16))
    close(out2.float().cpu(), ref2, rtol=3e-2, atol=3e-2)


def test_small_channel_convs(ops):
    g = torch.Generator().manual_seed(7)
    x = bf(torch.randn(2, 4, 16, 16, generator=g))
    w = bf(torch.randn(64, 4, 3, 3, generator=g) / 6)
    b = torch.randn(64, generator=g) * 0.1
    out = ops.conv(nhwc(x), ops.PackedConv(w, b, DEV))
    close(from_nhwc(out), F.conv2d(x, w, b, padding=1))
    # conv_in 4 -> 320 at 64x64 (4-pixel-strip kernel), without bias, and a width that is not a multiple of 4 (generic kernel)
    xin = bf(torch.randn(3, 4, 64, 64, generator=g))
    win = bf(torch.randn(320, 4, 3, 3, generator=g) / 6)
    close(from_nhwc(ops.conv(nhwc(xin), ops.PackedConv(win, None, DEV))), F.conv2d(xin, win, None, padding=1))
    xw = bf(torch.randn(1, 4, 10, 18, generator=g))
    close(from_nhwc(ops.conv(nhwc(xw), ops.PackedConv(w, b, DEV))), F.conv2d(xw, w, b, padding=1))
    x3 = bf(torch.randn(1, 3, 20, 12, generator=g))
    w3 = bf(torch.randn(32, 3, 3, 3, generator=g) / 5)
    close(from_nhwc(ops.conv(nhwc(x3), ops.PackedConv(w3, None, DEV))), F.conv2d(x3, w3, None, padding=1))
    w1 = bf(torch.randn(4, 4, 1, 1, generator=g) / 2)
    close(from_nhwc(ops.conv(nhwc(x), ops.PackedConv(w1, b[:4], DEV))), F.conv2d(x, w1, b[:4]))
    # small cout with fused GN+SiLU and fp32 output (UNet conv_out)
    xc = bf(torch.randn(2, 64, 16, 16, generator=g))
    wc = bf(torch.randn(4, 64, 3, 3, generator=g) / 24)
    bc = torch.randn(4, generator=g) * 0.1
    gamma, beta = 1 + 0.1 * torch.randn(64, generator=g), 0.1 * torch.randn(64, generator=g)
    ref = F.conv2d(bf(F.silu(F.group_norm(xc, 32, gamma, beta, 1e-5))), wc, bc, padding=1)
    xd = nhwc(xc)
    ab = ops.group_norm_ab(xd, gamma.to(DEV), beta.to(DEV), 32, 1e-5)
    out = ops.conv(xd, ops.PackedConv(wc, bc, DEV), gn_ab=ab, gn_silu=True, out_f32=True)
    close(out.cpu().permute(0, 3, 1, 2), ref, rtol=2e-2, atol=2e-2)
    w8 = bf(torch.randn(3, 64, 3, 3, generator=g) / 24)
    close(from_nhwc(ops.conv(xd, ops.PackedConv(w8, None, DEV))), F.conv2d(xc, w8, None, padding=1))


# ------------------------------------------------------------------------------------------- norms
def test_group_norm_paths(ops):
    g = torch.Generator().manual_seed(8)
    for (n, c1, c2, hw, groups) in [(2, 64, 0, 16, 32), (2, 320, 0, 32, 32), (1, 1280, 640, 8, 32), (2, 128, 0, 64, 32)]:
        x1 = bf(torch.randn(n, c1, hw, hw, generator=g) * 2 + 0.5)
        x2 = bf(torch.randn(n, c2, hw, hw, generator=g)) if c2 else None
        c = c1 + c2
        gamma, beta = 1 + 0.1 * torch.randn(c, generator=g), 0.1 * torch.randn(c, generator=g)
        xin = torch.cat([x1, x2], 1) if c2 else x1
        ref = F.silu(F.group_norm(xin, groups, gamma, beta, 1e-5))
        d1, d2 = nhwc(x1), (nhwc(x2) if c2 else None)
        keep = ops.GN_DIRECT_MAX_PIXELS
        abs_ = []
        for limit in (0, 1 << 30):                           # chunk-slab + finalize pair, then the one-launch small-map kernel
            ops.GN_DIRECT_MAX_PIXELS = limit
            try:
                ab = ops.group_norm_ab(d1, gamma.to(DEV), beta.to(DEV), groups, 1e-5, x2=d2)
            finally:
                ops.GN_DIRECT_MAX_PIXELS = keep
            abs_.append(ab)
            out = ops.gn_apply(d1, ab, silu=True, x2=d2)
            close(from_nhwc(out), ref)
        for other in abs_[1:]:
            close(abs_[0].cpu(), other.cpu(), rtol=1e-4, atol=1e-5)    # same statistic, different summation order


def test_fdn_modulate(ops):
    g = torch.Generator().manual_seed(9)
    n, c, hw = 4, 64, 16
    x = bf(torch.randn(n, c, hw, hw, generator=g))
    gam = bf(torch.randn(2, c, hw, hw, generator=g) * 0.3)
    bet = bf(torch.randn(2, c, hw, hw, generator=g) * 0.3)
    ref = F.group_norm(x, 32, None, None, 1e-5) * (1 + gam.repeat(2, 1, 1, 1)) + bet.repeat(2, 1, 1, 1)
    xd = nhwc(x)
    ab = ops.group_norm_ab(xd, None, None, 32, 1e-5)
    out = ops.fdn_modulate(xd, ab, nhwc(gam), nhwc(bet))
    close(from_nhwc(out), ref)


def test_layer_norm(ops):
    g = torch.Generator().manual_seed(10)
    for c in (64, 320, 640, 1280):
        x = bf(torch.randn(3, 50, c, generator=g) * 1.5 + 0.3)
        gamma, beta = 1 + 0.1 * torch.randn(c, generator=g), 0.1 * torch.randn(c, generator=g)
        ref = F.layer_norm(x, (c,), gamma, beta, 1e-5)
        out = ops.layer_norm(x.to(DEV, torch.bfloat16), gamma.to(DEV), beta.to(DEV))
        close(out.float().cpu(), ref)


@pytest.mark.parametrize("n,h,w,cin,cout,k,up", [(2, 32, 32, 64, 320, 3, 0), (2, 16, 16, 128, 640, 3, 0), (4, 8, 8, 128, 320, 3, 0),
                                                (3, 8, 8, 128, 320, 3, 0), (1, 16, 16, 64, 128, 3, 1), (2, 16, 16, 192, 320, 1, 0),
                                                (2, 64, 64, 64, 160, 1, 0), (2, 8, 8, 128, 320, 1, 0), (3, 4, 4, 128, 320, 1, 0)])
def test_group_norm_statistics_from_the_producing_epilogue(ops, n, h, w, cin, cout, k, up):
    """dc_conv_desc.gn_part_out: the conv / GEMM epilogue that writes a tensor also writes its GroupNorm partial sums, and
    `group_norm_ab` turns them into the same per-(sample, channel) scale / shift as the read pass (gn_stats / gn_direct) over
    the stored tensor — 8-row, 4-row and two-images-per-tile conv tiles, fused upsample, the LDS-DMA GEMM with a residual;
    when the rows of one sample do not fill a GEMM row tile (4x4 map), the launch declines and the read pass stays."""
    g = torch.Generator().manual_seed(31)
    x = torch.randn(n, h, w, cin, generator=g).to(DEV, torch.bfloat16)
    pc = ops.PackedConv(torch.randn(cout, cin, k, k, generator=g) / math.sqrt(cin * k * k), 0.5 * torch.randn(cout, generator=g), DEV)
    ho = h * (2 if up else 1)
    res = torch.randn(n, ho, ho, cout, generator=g).to(DEV, torch.bfloat16)
    y = ops.conv(x, pc, residual=res, upsample=bool(up), out_scale=1.3, gn_part=True)
    gamma, beta = (1 + 0.1 * torch.randn(cout, generator=g)).to(DEV), (0.1 * torch.randn(cout, generator=g)).to(DEV)
    if not hasattr(y, "gn_part"):                      # only a GEMM row tile that straddles two samples may decline
        assert k == 1 and (h * w) % 64 != 0
        return
    assert y.gn_part.shape[1:] == (n, cout, 2)
    fused = ops.group_norm_ab(y, gamma, beta, 32, 1e-5)
    plain = ops.group_norm_ab(y.clone(), gamma, beta, 32, 1e-5)          # the clone carries no partials: read pass
    # fp32 sums of the values before (epilogue) / after (read pass) the bf16 rounding of y
    torch.testing.assert_close(fused, plain, rtol=2e-3, atol=2e-3)
    y0 = ops.conv(x, pc, residual=res, upsample=bool(up), out_scale=1.3)
    assert torch.equal(y0, y)                                            # asking for statistics does not change the output


@pytest.mark.parametrize("c,mean", [(320, 0.3), (640, 2.5), (1280, -1.0)])
def test_layer_norm_folded_into_linear(ops, c, mean):
    """BasicTransformerBlock.norm1/2/3 -> to_q/k/v | to_q | ff.net.0.proj with the LayerNorm folded into the weights and the
    GEMM epilogue (dc_conv_desc.ln_stats): against F.linear(F.layer_norm(x)) in fp32 on the same bf16 operands.  The row
    statistics come (a) from dc_row_stats_bf16 and (b) from the epilogue of the producing linear (stats_out), whose partial
    sums are also checked directly.  Row offsets well away from zero (|mean| up to 2.5 sigma) exercise the mean * colsum
    cancellation.  Tolerance: one bf16 rounding of gamma*W instead of one of LN(x) — same order as the unfused path."""
    g = torch.Generator().manual_seed(20)
    m = 3 * 128 + 37                                   # ragged last M tile
    gamma, beta = 1 + 0.2 * torch.randn(c, generator=g), 0.2 * torch.randn(c, generator=g)
    # producer: t = a @ Wo^T + bo + res, emitting the row statistics of t
    a_in = bf(torch.randn(1, m, c, generator=g))
    wo = bf(torch.randn(c, c, generator=g) / math.sqrt(c))
    bo = torch.randn(c, generator=g) * 0.1 + mean
    res = bf(torch.randn(1, m, c, generator=g) * 1.5)
    parts = ops.row_stats_parts(c)
    st = torch.full((m, parts, 2), float("nan"), device=DEV)
    t = ops.linear(a_in.to(DEV, torch.bfloat16), ops.PackedConv(wo, bo, DEV), residual=res.to(DEV, torch.bfloat16), stats_out=st)
    tf = t.float().cpu()                                # the stored (bf16) tensor the LayerNorm sees
    tot = st.sum(1).cpu()
    close(tot[:, 0], tf[0].sum(-1), rtol=2e-3, atol=0.3)             # statistics of the fp32 values before the bf16 rounding
    close(tot[:, 1], (tf[0] ** 2).sum(-1), rtol=5e-3, atol=0.5)
    st1 = ops.row_stats(t)
    close(st1[:, 0, 0].cpu(), tf[0].sum(-1), rtol=1e-5, atol=1e-3)
    close(st1[:, 0, 1].cpu(), (tf[0] ** 2).sum(-1), rtol=1e-5, atol=1e-3)
    ln = F.layer_norm(tf, (c,), gamma, beta, 1e-5)
    # consumer 1: plain linear without bias (to_q/k/v)
    wq = bf(torch.randn(3 * c, c, generator=g) / math.sqrt(c))
    ref = F.linear(ln, wq)
    pc = ops.PackedConv(wq, None, DEV, ln=(gamma, beta, 1e-5))
    for stats in (st, st1):
        out = ops.linear(t, pc, ln_stats=ops.ln_finalize(stats, c, 1e-5))
        close(out.float().cpu(), ref, rtol=3e-2, atol=3e-2)
    # consumer 2: GEGLU projection with bias (ff.net.0.proj)
    w1 = bf(torch.randn(8 * c, c, generator=g) / math.sqrt(c))
    b1 = torch.randn(8 * c, generator=g) * 0.1
    hid, gate = F.linear(ln, w1, b1).chunk(2, -1)
    mr = ops.ln_finalize(st1, c, 1e-5)
    close(mr[:, 0].cpu(), tf[0].mean(-1), rtol=1e-4, atol=1e-4)
    close(mr[:, 1].cpu(), (tf[0].var(-1, unbiased=False) + 1e-5).rsqrt(), rtol=1e-3, atol=1e-4)
    out = ops.linear(t, ops.PackedConv(w1, b1, DEV, geglu=True, ln=(gamma, beta, 1e-5)), ln_stats=mr)
    close(out.float().cpu(), hid * F.gelu(gate), rtol=3e-2, atol=3e-2)
    with pytest.raises(ValueError):
        ops.linear(t, pc)                               # folded weights without statistics: refused, never silently wrong


@pytest.mark.parametrize("m,k,n", [(16384, 640, 1280), (12288, 1280, 640), (8192, 1920, 1280)])
def test_wide_gemm_long_k_shapes(ops, m, k, n):
    """Shapes the dispatcher hands to the 256-row ping-pong GEMM (gemm_wide.hip: K >= 640, whole tiles, >= 192 tiles): every
    specialised epilogue against fp32 torch on the same bf16 operands — bias; bias + scale + residual with the LayerNorm row
    statistics and the GroupNorm partials of the output; folded LayerNorm; GEGLU; folded LayerNorm + GEGLU; a channel-concat
    input (two K ranges).  Each launch twice: the ring / barrier protocol must give the same bits."""
    g = torch.Generator().manual_seed(40)
    x = bf(torch.randn(1, m, k, generator=g))
    w = bf(torch.randn(n, k, generator=g) / math.sqrt(k))
    b = torch.randn(n, generator=g) * 0.1
    xd = x.to(DEV, torch.bfloat16)
    pc = ops.PackedConv(w, b, DEV)
    ref = F.linear(x, w, b)
    with capture_routes() as routes:
        out = ops.linear(xd, pc)
    assert [r.kernel for r in routes] == ["gemm_wide"], routes
    close(out.float().cpu(), ref)
    assert torch.equal(out, ops.linear(xd, pc))
    # residual + scale + statistics (4-D call: per-sample GroupNorm partials)
    hw = 4096 if m % 4096 == 0 else 2048
    res = bf(torch.randn(1, m, n, generator=g))
    st = torch.full((m, ops.row_stats_parts(n), 2), float("nan"), device=DEV)
    with capture_routes() as routes:
        y = ops.conv(xd.reshape(m // hw, hw // 64, 64, k), pc, residual=res.to(DEV, torch.bfloat16).reshape(m // hw, hw // 64, 64, n),
                     out_scale=0.7, stats_out=st, gn_part=True)
    assert [r.kernel for r in routes] == ["gemm_wide"], routes
    ref2 = 0.7 * ref + res
    close(y.reshape(1, m, n).float().cpu(), ref2, rtol=3e-2, atol=3e-2)
    yf = y.reshape(m, n).float().cpu()
    close(st.sum(1)[:, 0].cpu(), yf.sum(-1), rtol=2e-3, atol=0.5)
    close(st.sum(1)[:, 1].cpu(), (yf ** 2).sum(-1), rtol=5e-3, atol=1.0)
    gamma, beta = (1 + 0.1 * torch.randn(n, generator=g)).to(DEV), (0.1 * torch.randn(n, generator=g)).to(DEV)
    close(ops.group_norm_ab(y, gamma, beta, 32, 1e-5), ops.group_norm_ab(y.clone(), gamma, beta, 32, 1e-5), rtol=2e-3, atol=2e-3)
    # folded LayerNorm, plain and GEGLU
    lg, lb = 1 + 0.2 * torch.randn(k, generator=g), 0.2 * torch.randn(k, generator=g)
    ln = F.layer_norm(x, (k,), lg, lb, 1e-5)
    mr = ops.ln_finalize(ops.row_stats(xd), k, 1e-5)
    close(ops.linear(xd, ops.PackedConv(w, None, DEV, ln=(lg, lb, 1e-5)), ln_stats=mr).float().cpu(), F.linear(ln, w), rtol=3e-2, atol=3e-2)
    w1 = bf(torch.randn(2 * n, k, generator=g) / math.sqrt(k))
    b1 = torch.randn(2 * n, generator=g) * 0.1
    hid, gate = F.linear(x, w1, b1).chunk(2, -1)
    o = ops.linear(xd, ops.PackedConv(w1, b1, DEV, geglu=True))
    close(o.float().cpu(), hid * F.gelu(gate), rtol=3e-2, atol=3e-2)
    assert torch.equal(o, ops.linear(xd, ops.PackedConv(w1, b1, DEV, geglu=True)))
    hid, gate = F.linear(ln, w1, b1).chunk(2, -1)
    close(ops.linear(xd, ops.PackedConv(w1, b1, DEV, geglu=True, ln=(lg, lb, 1e-5)), ln_stats=mr).float().cpu(), hid * F.gelu(gate),
          rtol=3e-2, atol=3e-2)
    # channel concat: cat[x[..., :k1], x[..., k1:]] read in place
    k1 = 320 if k > 640 else 256
    xa, xb = xd[..., :k1].contiguous().reshape(1, 1, m, k1), xd[..., k1:].contiguous().reshape(1, 1, m, k - k1)
    close(ops.conv(xa, pc, x2=xb).reshape(1, m, n).float().cpu(), ref)


@pytest.mark.parametrize("m,k,n", [(8192, 640, 3584), (7168, 1344, 4096), (14336, 640, 1920),
                                   (15104, 640, 1920)])        # 59 row tiles: a short last group of the gm = 8 tile order, half-full last column tile
def test_p8_gemm_shapes(ops, m, k, n):
    """Shapes the dispatcher hands to the 256 x 256 four-phase GEMM (gemm_p8.hip: no residual / statistics, whole 256 x 256 tiles,
    >= 448 of them, K >= 640; an even and an odd number of K tiles; a half-full last column tile): bias, folded LayerNorm, GEGLU, folded LayerNorm + GEGLU against
    fp32 torch on the same bf16 operands.  Each launch twice (the DMA / barrier protocol must give the same bits), and the first 256
    rows against a 256-row launch of the same operator, which another kernel of the family takes: the kernels accumulate in the
    same order with the same epilogue arithmetic, so the bits must agree."""
    g = torch.Generator().manual_seed(41)
    x = bf(torch.randn(1, m, k, generator=g))
    w = bf(torch.randn(n, k, generator=g) / math.sqrt(k))
    b = torch.randn(n, generator=g) * 0.1
    xd = x.to(DEV, torch.bfloat16)
    head = xd[:, :256].contiguous()
    lg, lb = 1 + 0.2 * torch.randn(k, generator=g), 0.2 * torch.randn(k, generator=g)
    ln = F.layer_norm(x, (k,), lg, lb, 1e-5)
    mr = ops.ln_finalize(ops.row_stats(xd), k, 1e-5)
    mr_head = mr[:256].contiguous()
    hid, gate = F.linear(x, w, b).chunk(2, -1)
    hid_ln, gate_ln = F.linear(ln, w, b).chunk(2, -1)
    cases = [(ops.PackedConv(w, b, DEV), None, F.linear(x, w, b)),
             (ops.PackedConv(w, b, DEV, ln=(lg, lb, 1e-5)), mr, F.linear(ln, w, b)),
             (ops.PackedConv(w, b, DEV, geglu=True), None, hid * F.gelu(gate)),
             (ops.PackedConv(w, b, DEV, geglu=True, ln=(lg, lb, 1e-5)), mr, hid_ln * F.gelu(gate_ln))]
    for pc, stats, ref in cases:
        with capture_routes() as routes:
            out = ops.linear(xd, pc, ln_stats=stats)
        assert [r.kernel for r in routes] == ["gemm_p8"], routes
        close(out.float().cpu(), ref, rtol=3e-2, atol=3e-2)
        assert torch.equal(out, ops.linear(xd, pc, ln_stats=stats))
        assert torch.equal(out[:, :256], ops.linear(head, pc, ln_stats=None if stats is None else mr_head))


# ------------------------------------------------------------------------------------------- attention
@pytest.mark.parametrize("b,heads,nq,nk,d", [(2, 8, 256, 256, 40), (1, 8, 1024, 1024, 80), (2, 8, 64, 64, 160),
                                             (2, 8, 256, 77, 40), (1, 2, 100, 77, 64), (1, 4, 70, 130, 16),
                                             (1, 2, 33, 5, 8), (1, 3, 200, 200, 32), (1, 1, 128, 192, 128),
                                             # text cross-attention at full batch: keys resident, 4 query blocks per workgroup
                                             (16, 8, 4096, 77, 40), (32, 8, 1000, 77, 80), (40, 8, 250, 100, 160),
                                             # grids that are NOT a multiple of 8 workgroups (the XCD-aware block order of round 4 has to stay a
                                             # bijection there): 3 x 5 heads, ragged query counts; long, ping-pong and short-context forms
                                             (3, 5, 700, 300, 40), (3, 5, 700, 77, 40), (37, 7, 1500, 320, 40), (5, 3, 130, 70, 80), (67, 7, 2100, 77, 40)])
def test_attention(ops, b, heads, nq, nk, d):
    g = torch.Generator().manual_seed(11)
    c = heads * d
    q = bf(torch.randn(b, nq, c, generator=g))
    k = bf(torch.randn(b, nk, c, generator=g))
    v = bf(torch.randn(b, nk, c, generator=g))
    qh, kh, vh = (t.view(b, -1, heads, d).transpose(1, 2) for t in (q, k, v))
    ref = F.scaled_dot_product_attention(qh, kh, vh).transpose(1, 2).reshape(b, nq, c)
    qd, kd, vd = (t.to(DEV, torch.bfloat16) for t in (q, k, v))
    out = ops.attention(qd, kd, vd, heads)
    close(out.float().cpu(), ref, rtol=2e-2, atol=1e-2)
    _strict(out, lambda rows: L.attention_ref(qd, kd, vd, heads, rows))


def test_attention_forced_rescale_and_strided_views(ops):
    """A key spike late in the sequence forces the online-softmax rescale branch; K/V are slices of one fused tensor."""
    g = torch.Generator().manual_seed(12)
    b, heads, n, d = 1, 2, 256, 40
    c = heads * d
    q = bf(torch.randn(b, n, c, generator=g))
    kv = bf(torch.randn(b, n, 2 * c, generator=g))
    kv[0, 200, :c] = bf(q[0, 17] * 6.0)             # row 17's max jumps at key 200 (4th tile)
    k, v = kv[..., :c], kv[..., c:]
    qh, kh, vh = (t.reshape(b, -1, heads, d).transpose(1, 2) for t in (q, k, v))
    ref = F.scaled_dot_product_attention(qh, kh, vh).transpose(1, 2).reshape(b, n, c)
    kvd = kv.to(DEV, torch.bfloat16)
    qd = q.to(DEV, torch.bfloat16)
    out = ops.attention(qd, kvd[..., :c], kvd[..., c:], heads)
    close(out.float().cpu(), ref, rtol=2e-2, atol=1e-2)
    _strict(out, lambda rows: L.attention_ref(qd, kvd[..., :c], kvd[..., c:], heads, rows))


@pytest.mark.parametrize("b,heads,nq,nk,d", [(32, 8, 4096, 4096, 40),   # the 64x64 self-attention of the decode loop at model batch 32
                                             (40, 8, 1100, 1000, 40),   # ragged: Nq not a multiple of 512, Nk not of 64
                                             (64, 8, 512, 256, 32), (36, 8, 600, 320, 16),   # d = 16: back on the ping-pong form since round 4 (the packed-FMA cause of its wrong rows)
                                             (32, 8, 1024, 1024, 80),    # the 32x32 self-attention at model batch 32 (4-wave form: its ping-pong variant measured no gain)
                                             (34, 8, 700, 330, 80), (40, 4, 512, 256, 64)])
def test_attention_ping_pong_form(ops, b, heads, nq, nk, d):
    """Long-context shapes at decode batch sizes — d <= 48 takes the 8-wave ping-pong kernel (>= 256 workgroups of 512 queries,
    Nk >= 256), d = 64 / 80 the 4-wave form: against SDPA on a sample of the batch, and bit-identical from launch to launch."""
    g = torch.Generator().manual_seed(21)
    c = heads * d
    q = bf(torch.randn(b, nq, c, generator=g))
    k = bf(torch.randn(b, nk, c, generator=g))
    v = bf(torch.randn(b, nk, c, generator=g))
    k[1, nk - 3, :d] = bf(q[1, 5, :d] * 6.0)           # a late key spike: the offset of head 0 / sample 1 has to move
    qd, kd, vd = (t.to(DEV, torch.bfloat16) for t in (q, k, v))
    out = ops.attention(qd, kd, vd, heads)
    assert torch.equal(out, ops.attention(qd, kd, vd, heads))
    for bi in (0, 1, b - 1):
        qh, kh, vh = (t[bi:bi + 1].view(1, -1, heads, d).transpose(1, 2) for t in (q, k, v))
        ref = F.scaled_dot_product_attention(qh, kh, vh).transpose(1, 2).reshape(1, nq, c)
        close(out[bi:bi + 1].float().cpu(), ref, rtol=2e-2, atol=1e-2)
    _strict(out, lambda rows: L.attention_ref(qd, kd, vd, heads, rows))


@pytest.mark.parametrize("b,heads,nq,nk,d", [(36, 8, 1024, 512, 16), (64, 8, 512, 256, 8), (16, 8, 4096, 4096, 40), (4, 8, 4096, 4096, 40),
                                             (2, 8, 1024, 1024, 80), (32, 8, 256, 256, 160), (8, 2, 512, 512, 128),
                                             (32, 8, 4096, 77, 40), (32, 8, 1024, 77, 80), (32, 8, 256, 77, 160)])
def test_attention_launch_to_launch_bit_identity(ops, b, heads, nq, nk, d):
    """Every head dim and every form of the kernel (4-wave, two query blocks per wave, 8-wave ping-pong, keys-resident short
    context; whole and ragged key tiles): eight launches of the same inputs must be `torch.equal`, and right against SDPA.  A wrong
    build of one instantiation showed up exactly here in round 3 ("Open")."""
    g = torch.Generator().manual_seed(77)
    c = heads * d
    q, k, v = (bf(torch.randn(b, n, c, generator=g)).to(DEV, torch.bfloat16) for n in (nq, nk, nk))
    outs = [ops.attention(q, k, v, heads) for _ in range(8)]
    for o in outs[1:]:
        assert torch.equal(o, outs[0])
    qh, kh, vh = (t[:2].float().view(2, -1, heads, d).transpose(1, 2) for t in (q, k, v))
    ref = F.scaled_dot_product_attention(qh, kh, vh).transpose(1, 2).reshape(2, nq, c)
    close(outs[0][:2].float(), ref, rtol=2e-2, atol=1e-2)


def test_softmax_rows(ops):
    g = torch.Generator().manual_seed(13)
    s = torch.randn(37, 4096, generator=g) * 4
    ref = torch.softmax(s * 0.25, -1)
    close(ops.softmax_rows(s.to(DEV), 0.25).float().cpu(), ref, rtol=1e-2, atol=1e-5)


# ------------------------------------------------------------------------------------------- misc
def test_layout_and_timestep_embedding(ops):
    from oracle.sd15_ref import timestep_embedding
    g = torch.Generator().manual_seed(14)
    x = torch.randn(2, 5, 6, 7, generator=g)
    y = ops.nchw_f32_to_nhwc_bf16(x.to(DEV))
    assert torch.equal(from_nhwc(y), bf(x))
    assert torch.equal(ops.nhwc_bf16_to_nchw_f32(y).cpu(), bf(x))
    t = torch.tensor([951.0])
    ref = timestep_embedding(t.expand(3), 320)
    out = ops.timestep_embedding(t.to(DEV), 3, 320).cpu()
    close(out, ref, rtol=1e-4, atol=2e-4)


def test_conv_tile_two_images_per_tile(ops):
    """8x8 maps, even batch, enough tiles: the 8-row tile shape carries two whole images (wave row = image)."""
    g = torch.Generator().manual_seed(15)
    n, cin, cout = 16, 640, 1280
    x = bf(torch.randn(n, cin, 8, 8, generator=g))
    wt = bf(torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(cin * 9))
    b = torch.randn(cout, generator=g) * 0.1
    temb = torch.randn(n, cout, generator=g)
    ref = F.conv2d(x, wt, b, padding=1) + temb[:, :, None, None]
    out = ops.conv(nhwc(x), ops.PackedConv(wt, b, DEV), row_add=temb.to(DEV), splitk=10)     # (16/2) * 8 N-tiles * 10 splits = 640 workgroups >= 512
    close(from_nhwc(out), ref)


# the smallest shapes at which each arm of the split-K rule picks above 1: (n, h, w, cin, cout, k, stride), the kernel the library
# routes the launch to and the split it picks (csrc/igemm.hip: splitk_pick; tests/splitk_rule_ref.py is the frozen statement)
AUTO_SPLIT_CASES = [
    ((1, 8, 8, 2560, 1280, 1, 1), "gemm_dma", 5),              # 1x1, 64 rows: K steps split, target 256 workgroups
    ((1, 8, 8, 1280, 1280, 3, 1), "conv3x3_tile", 20),         # the halo-tile kernel splits 64-channel chunks
    ((2, 32, 32, 640, 640, 3, 1), "conv3x3_tile", 2),          # ... and aims at one workgroup per CU on big maps
    ((1, 32, 32, 640, 640, 3, 2), "igemm", 10),                # the stride-2 rule (no split reaches 1024 workgroups: the largest)
    ((1, 13, 9, 1280, 128, 3, 1), "igemm", 20),                # ragged map on the gather GEMM: (tap, chunk) steps split
]


def _recording_scratch(ops, monkeypatch):
    handed, real = [], ops._scratch

    def scratch(shape, device, what):
        handed.append((what, tuple(shape)))
        return real(shape, device, what)
    monkeypatch.setattr(ops, "_scratch", scratch)
    return handed


@pytest.mark.parametrize("shape,kernel,pick", AUTO_SPLIT_CASES)
def test_conv_split_picked_by_the_library_is_the_frozen_rule_s_launch(ops, monkeypatch, shape, kernel, pick):
    """ops.conv(splitk=None) (DC_SPLITK_AUTO) against splitk = the frozen rule's value on the same operands: the same slabs are
    asked for, the outputs are the same bits, and they meet the launch's fp64 reference"""
    import splitk_rule_ref
    n, h, w, cin, cout, k, stride = shape
    g = torch.Generator().manual_seed(19)
    xd = nhwc(bf(torch.randn(n, cin, h, w, generator=g)))
    pc = ops.PackedConv(bf(torch.randn(cout, cin, k, k, generator=g) / math.sqrt(cin * k * k)), torch.randn(cout, generator=g) * 0.1, DEV)
    handed = _recording_scratch(ops, monkeypatch)
    with capture_routes() as routes:
        auto = ops.conv(xd, pc, stride=stride)
    m, rows_per_image = auto.numel() // cout, auto.shape[1] * auto.shape[2]
    assert [(r.kernel, r.splitk) for r in routes] == [(kernel, pick)], routes
    assert handed == [("splitk", (pick, m, cout))], handed
    assert splitk_rule_ref.pick(m, cin, cout, k, stride, rows_per_image, lambda: kernel == "conv3x3_tile") == pick
    del handed[:]
    with capture_routes() as routes:
        asked = ops.conv(xd, pc, stride=stride, splitk=pick)
    assert [(r.kernel, r.splitk) for r in routes] == [(kernel, pick)] and handed == [("splitk", (pick, m, cout))], (routes, handed)
    assert torch.equal(auto, asked)
    _strict(auto, lambda rows: L.conv_ref(xd, pc, rows, stride=stride), spatial=tuple(auto.shape[:3]) if k == 3 else None)


def test_unet_conv_out_of_one_small_frame_runs_unsplit(ops, monkeypatch):
    """UNet conv_out (320 -> 4 on the halo-tile kernel, GroupNorm + SiLU on load, fp32 out) on the 8x8 latents of one frame: the
    frozen rule picked split 5 there, which the library refuses for a Cout that is no multiple of 16; the library's own pick is 1"""
    g = torch.Generator().manual_seed(20)
    n, cin, cout, hw = 1, 320, 4, 8
    xd = nhwc(bf(torch.randn(n, cin, hw, hw, generator=g)))
    pc = ops.PackedConv(bf(torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(cin * 9)), torch.randn(cout, generator=g) * 0.1, DEV,
                        mfma_small_cout=True)
    gamma, beta = 1 + 0.1 * torch.randn(cin, generator=g), 0.1 * torch.randn(cin, generator=g)
    ab = ops.group_norm_ab(xd, gamma.to(DEV), beta.to(DEV), 32, 1e-5)
    handed = _recording_scratch(ops, monkeypatch)
    with capture_routes() as routes:
        auto = ops.conv(xd, pc, gn_ab=ab, gn_silu=True, out_f32=True)
    assert [(r.kernel, r.splitk) for r in routes] == [("conv3x3_tile", 1)] and not handed, (routes, handed)
    assert torch.equal(auto, ops.conv(xd, pc, gn_ab=ab, gn_silu=True, out_f32=True, splitk=1))
    _strict(auto, lambda rows: L.conv_ref(xd, pc, rows, gn_ab=ab, gn_silu=True), spatial=tuple(auto.shape[:3]))


# ------------------------------------------------------------------------------------------- input side
@pytest.mark.parametrize("hw,target", [((270, 480), (512, 512)), ((512, 512), (512, 512)), ((64, 96), (33, 1)), ((1, 7), (5, 9))])
def test_flow_hw2_resize_scale(ops, hw, target):
    """resize_flow_to (controlnet/utils.py:21-28) restated with the same torch calls on the CPU vs the device kernel.
    fp32 both sides; tolerance covers fma contraction only."""
    g = torch.Generator().manual_seed(16)
    h, w = hw
    th, tw = target
    flow = torch.randn(h, w, 2, generator=g) * 6
    ft = F.interpolate(flow.permute(2, 0, 1).unsqueeze(0), size=(th, tw), mode="bilinear", align_corners=True)
    ft[:, 0] *= (tw / max(w, 1))
    ft[:, 1] *= (th / max(h, 1))
    out = ops.flow_hw2_resize_scale(flow.to(DEV), th, tw).cpu()
    close(out, ft[0], rtol=1e-5, atol=1e-5)


def test_pack_sixch_bit_exact(ops):
    """TF.to_tensor + cat of load_pair_to_sixch (utils.py:36-39): uint8 -> x/255 is bit-exact."""
    g = torch.Generator().manual_seed(17)
    a = torch.randint(0, 256, (37, 53, 3), generator=g, dtype=torch.uint8)
    b = torch.randint(0, 256, (37, 53, 3), generator=g, dtype=torch.uint8)
    ref = torch.cat([a.permute(2, 0, 1).float().div(255.0), b.permute(2, 0, 1).float().div(255.0)], 0).unsqueeze(0)
    assert torch.equal(ops.pack_sixch(a.to(DEV), b.to(DEV)).cpu(), ref)


def test_load_controls_and_flows_device_path_equals_host_path(tmp_path):
    """utils.py:41-52: the GPU preprocessing path against the host path of the same loader on the same files."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import numpy as np
    from PIL import Image
    from diffcodec_amd import io_utils
    rng = np.random.default_rng(0)
    for name in ("a.png", "b.png"):
        Image.fromarray(rng.integers(0, 256, (300, 400, 3), dtype=np.uint8)).save(tmp_path / name)
    for name in ("f.flo", "b.flo"):
        io_utils.write_flo(str(tmp_path / name), rng.normal(0, 5, (135, 240, 2)).astype(np.float32))
    args = [str(tmp_path / n) for n in ("a.png", "b.png", "f.flo", "b.flo")]
    c_ref, f_ref = io_utils.load_controls_and_flows(*args, size=(512, 512), device="cpu")
    c_dev, f_dev = io_utils.load_controls_and_flows(*args, size=(512, 512), device=DEV)
    assert c_dev.shape == (1, 6, 512, 512) and f_dev.shape == (1, 4, 512, 512)
    assert torch.equal(c_dev.cpu(), c_ref)
    close(f_dev.cpu(), f_ref, rtol=1e-5, atol=1e-5)


def test_conv3x3_four_output_channels_on_the_tile_kernel(ops):
    """UNet conv_out (320 -> 4, GroupNorm+SiLU on load, fp32 out) through the MFMA halo-tile kernel: Cout = 4 is one
    mostly empty N-tile (clamped weight rows, guarded stores)."""
    g = torch.Generator().manual_seed(18)
    n, cin, cout, hw = 2, 320, 4, 32
    x = bf(torch.randn(n, cin, hw, hw, generator=g))
    wt = bf(torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(cin * 9))
    b = torch.randn(cout, generator=g) * 0.1
    gamma, beta = 1 + 0.1 * torch.randn(cin, generator=g), 0.1 * torch.randn(cin, generator=g)
    ref = F.conv2d(F.silu(F.group_norm(x, 32, gamma, beta, 1e-5)), wt, b, padding=1)
    pc = ops.PackedConv(wt, b, DEV, mfma_small_cout=True)
    assert pc.kind == "igemm"
    xn = nhwc(x)
    ab = ops.group_norm_ab(xn, gamma.to(DEV), beta.to(DEV), 32, 1e-5)
    out = ops.conv(xn, pc, gn_ab=ab, gn_silu=True, out_f32=True)
    assert out.dtype == torch.float32 and out.shape == (n, hw, hw, cout)
    close(out.permute(0, 3, 1, 2).cpu(), ref)
    # the direct small-Cout kernel stays the fallback for shapes the tile kernel does not take
    assert ops.PackedConv(wt[:3], b[:3], DEV, mfma_small_cout=True).kind == "small_cout"


@pytest.mark.parametrize("hw,tile,overlap", [((256, 448), 256, 64), ((540, 960), 256, 64), ((512, 512), 512, 64), ((300, 300), 128, 32)])
def test_blend_tiles_ramp_equals_host_merge(ops, hw, tile, overlap):
    """Tiled-decode blend kernel vs tiling.merge_ramp (host, numpy fp32) on the windows of plan_tiles: same weights, same
    fp32 op order -> bit-exact uint8 frame.  Covers 1x2, 3x5 (1080p/2-like), a single window, and a 3x3 plan."""
    import numpy as np
    from diffcodec_amd import tiling
    from diffcodec_amd.tiled_decode import plan_tiles
    h, w = hw
    coords = plan_tiles(h, w, tile, overlap)
    g = torch.Generator().manual_seed(19)
    tiles = torch.rand(len(coords), 3, tile, tile, generator=g)
    host = tiling.merge_ramp([np.asarray(t.permute(1, 2, 0).numpy() * 255.0, np.float32) for t in tiles], coords, (h, w),
                             order="hwc", feather=overlap)
    dev = ops.blend_tiles_ramp(tiles.to(DEV), coords, (h, w), overlap).cpu().numpy()
    assert dev.shape == host.shape == (h, w, 3) and dev.dtype == np.uint8
    assert np.array_equal(dev, host)


# ------------------------------------------------------------------------------------------- single-pass variance under outliers
@pytest.mark.parametrize("ratio", [30.0, 100.0])
@pytest.mark.parametrize("k", [1, 3])
def test_group_norm_epilogue_partials_with_outlier_channel_means(ops, ratio, k):
    """the GroupNorm partials of a conv / GEMM epilogue are (sum, sum of squares) in fp32 and the finalize forms
    E[x^2] - mean^2.  Trained SD-1.5 activations have channels whose |mean| is tens of sigma; here every group of the OUTPUT
    sits at |mean| / sigma = 30 and 100 (a large per-group bias on a unit-variance conv output).  Bar: the per-(sample, channel)
    scale / shift against a two-pass float64 reference over the SAME stored bf16 tensor: rstd within 2 % (the bf16 grid of the
    tensor itself is 0.4 % of the mean, i.e. up to 0.4 sigma at ratio 100)."""
    g = torch.Generator().manual_seed(97)
    n, h, w, cin, cout, groups = 2, 32, 32, 64, 320, 32
    x = torch.randn(n, h, w, cin, generator=g).to(DEV, torch.bfloat16)
    wgt = torch.randn(cout, cin, k, k, generator=g) / math.sqrt(cin * k * k)          # unit-variance outputs
    sign = torch.where(torch.arange(groups) % 2 == 0, 1.0, -1.0).repeat_interleave(cout // groups)
    bias = sign * ratio * (1.0 + 0.05 * torch.randn(groups, generator=g)).repeat_interleave(cout // groups)
    y = ops.conv(x, ops.PackedConv(wgt, bias, DEV), gn_part=True)
    assert hasattr(y, "gn_part")
    gamma, beta = (1 + 0.1 * torch.randn(cout, generator=g)).to(DEV), (0.1 * torch.randn(cout, generator=g)).to(DEV)
    for name, ab in (("epilogue partials", ops.group_norm_ab(y, gamma, beta, groups, 1e-5)),
                     ("read pass", ops.group_norm_ab(y.clone(), gamma, beta, groups, 1e-5))):
        yd = y.double().reshape(n, h * w, groups, cout // groups)
        mean = yd.mean(dim=(1, 3))
        var = ((yd - mean[:, None, :, None]) ** 2).mean(dim=(1, 3))
        assert 0.7 * ratio < (mean.abs() / var.sqrt()).min().item()                  # the case really is what it says
        rstd = (var + 1e-5).rsqrt().repeat_interleave(cout // groups, 1)
        a_ref = rstd * gamma.double()[None]
        b_ref = beta.double()[None] - mean.repeat_interleave(cout // groups, 1) * a_ref
        a, b = ab[..., 0].double(), ab[..., 1].double()
        rel = ((a - a_ref).abs() / a_ref.abs()).max().item()
        assert rel < 2e-2, (name, ratio, k, rel)
        # the normalised value of a typical element: (x * a + b) has O(1) magnitude, so the shift must be right to ~1e-2 absolute
        xs = mean.repeat_interleave(cout // groups, 1)
        assert ((xs * a + b) - (xs * a_ref + b_ref)).abs().max().item() < 3e-2, (name, ratio, k)


@pytest.mark.parametrize("ratio", [30.0, 100.0])
def test_layer_norm_fold_with_outlier_row_means(ops, ratio):
    """The LayerNorm fold Linear(LN(x)) = rstd * (x W'^T - mean * colsum(W')) + b' at |row mean| / sigma = 30 and 100, statistics
    from the producing GEMM's epilogue.  Those statistics are taken from the fp32 values the epilogue is about to round (DESIGN
    §3 item 9), so the single-pass E[x^2] - mean^2 is checked against a two-pass float64 reference over the UNROUNDED rows
    (a float64 GEMM of the same bf16 operands): at ratio 100 the bf16 grid of the stored rows is 0.5 = half a sigma, and the
    variance of the stored rows is 2 % larger than that of the values they were rounded from — which is not the finalize's
    doing (first GPU run of this test compared against the stored rows and read 3.5 % there).
    The fold itself is then checked against the same formula in float64 on the stored bf16 rows with the reference statistics:
    the subtraction cancels `ratio` times the result's magnitude in the fp32 accumulators — two decimal digits of seven."""
    g = torch.Generator().manual_seed(5)
    c, m = 320, 256
    a_in = bf(torch.randn(1, m, c, generator=g))
    wo = bf(torch.randn(c, c, generator=g) / math.sqrt(c))
    bo = torch.full((c,), ratio)                                          # rows: unit sigma around `ratio`
    st = torch.empty((m, ops.row_stats_parts(c), 2), device=DEV)
    t = ops.linear(a_in.to(DEV, torch.bfloat16), ops.PackedConv(wo, bo, DEV), stats_out=st)
    td = t.double().cpu()[0]                                              # the stored bf16 rows
    tu = F.linear(a_in.double()[0], wo.double(), bo.double())             # the values they were rounded from
    assert (td - tu).abs().max().item() <= 0.0045 * ratio + 0.05          # bf16 grid of a value near `ratio`
    mean, var = tu.mean(-1), tu.var(-1, unbiased=False)
    assert (mean.abs() / var.sqrt()).min().item() > 0.7 * ratio
    mr = ops.ln_finalize(st, c, 1e-5).double().cpu()
    rstd = (var + 1e-5).rsqrt()
    assert ((mr[:, 0] - mean).abs() / var.sqrt()).max().item() < 1e-3     # mean to a thousandth of a sigma
    assert ((mr[:, 1] - rstd).abs() / rstd).max().item() < 5e-3, ((mr[:, 1] - rstd).abs() / rstd).max().item()
    gamma, beta = 1 + 0.2 * torch.randn(c, generator=g), 0.2 * torch.randn(c, generator=g)
    wq = bf(torch.randn(3 * c, c, generator=g) / math.sqrt(c))
    out = ops.linear(t, ops.PackedConv(wq, None, DEV, ln=(gamma, beta, 1e-5)), ln_stats=ops.ln_finalize(st, c, 1e-5))
    ref = F.linear((td - mean[:, None]) * rstd[:, None] * gamma.double() + beta.double(), wq.double())
    err = (out.double().cpu()[0] - ref).abs()
    assert err.mean().item() < 1.5e-2 and err.max().item() < 0.12, (ratio, err.mean().item(), err.max().item())
