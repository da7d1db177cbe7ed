"""GPU parity of the K = 320 row-panel GEMM (csrc/gemm_rowpanel.hip: activation panel in registers, W streamed through an
LDS-DMA ring) — the kernel that takes the 64x64-resolution transformer linears once the row count fills the chip
(M >= 65,536, M % 256 == 0).

Two checkers per epilogue mode:
  * the SAME rows launched in chunks of 16,384 take the 128-row tile kernel (gemm_dma.hip: M too small for the row-panel rule).
    A GEMM is row-independent and both kernels accumulate k in the same order with the same epilogue expressions, so the bf16
    outputs must be `torch.equal` — the bar of VERDICT r2 item 2;
  * a float64 reference of the op on the bf16-rounded operands (rows sampled across every panel / wave / stage position).
Statistics by-products (row sums for the LayerNorm fold, GroupNorm partials) associate differently in the two kernels: compared
after their finalize passes with a tolerance, and against float64."""
import math

import pytest
import torch
import torch.nn.functional as F

from launch_shadow import capture_routes

pytestmark = pytest.mark.gpu
DEV = "cuda"
M, K, CH = 65536, 320, 16384


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from diffcodec_amd import ops as o
    return o


def bf(x):
    return x.to(torch.bfloat16).float()


def _rows(g, m, c, scale=1.0):
    return (torch.randn(1, m, c, generator=g) * scale).to(DEV, torch.bfloat16)


def _on(kernel, fn, ln_first=None):
    """fn() must issue exactly one GEMM launch, on `kernel` (dc_conv_route of its descriptor); returns fn()'s value."""
    with capture_routes() as routes:
        y = fn()
    assert [r.kernel for r in routes] == [kernel], routes
    if ln_first is not None:
        assert routes[0].ln_first == ln_first, routes
    return y


def _sample_rows():
    # every wave of a panel, first / last panels, all 16 fragment rows and both row tiles
    idx = list(range(0, 256)) + list(range(M - 256, M)) + list(range(256 * 100 + 3, M, 4099))
    return torch.tensor(sorted(set(idx)))


@pytest.mark.parametrize("n_out", [320, 960])
def test_bias_mode_equals_tile_kernel_and_fp64(ops, n_out):
    g = torch.Generator().manual_seed(1)
    x = _rows(g, M, K)
    w = bf(torch.randn(n_out, K, generator=g) / math.sqrt(K))
    b = torch.randn(n_out, generator=g)
    pc = ops.PackedConv(w, b, DEV)
    with capture_routes() as routes:
        big = ops.linear(x, pc)
        small = torch.cat([ops.linear(x[:, i:i + CH], pc) for i in range(0, M, CH)], 1)
    assert [r.kernel for r in routes] == ["gemm_rowpanel"] + ["gemm_dma"] * (M // CH), routes
    assert torch.equal(big, small)
    rows = _sample_rows()
    ref = F.linear(x[0, rows].double().cpu(), w.double(), b.double())
    torch.testing.assert_close(big[0, rows].double().cpu(), ref, rtol=1e-2, atol=1e-2)
    assert torch.equal(big, ops.linear(x, pc))                                   # run-to-run bit-identical


def test_residual_scale_and_row_statistics(ops):
    g = torch.Generator().manual_seed(2)
    n_out = 320
    x = _rows(g, M, K)
    res = _rows(g, M, n_out, 2.0)
    w = bf(torch.randn(n_out, K, generator=g) / math.sqrt(K))
    b = torch.randn(n_out, generator=g)
    pc = ops.PackedConv(w, b, DEV)
    parts = ops.row_stats_parts(n_out)
    st = torch.full((M, parts, 2), float("nan"), device=DEV)
    big = _on("gemm_rowpanel", lambda: ops.linear(x, pc, residual=res, out_scale=0.75, stats_out=st))
    sts = torch.empty((M, parts, 2), device=DEV)
    small = torch.cat([ops.linear(x[:, i:i + CH], pc, residual=res[:, i:i + CH], out_scale=0.75, stats_out=sts[i:i + CH])
                       for i in range(0, M, CH)], 1)
    assert torch.equal(big, small)
    assert torch.isfinite(st).all()                                               # every promised part is written
    mr_big, mr_small = ops.ln_finalize(st, n_out, 1e-5), ops.ln_finalize(sts, n_out, 1e-5)
    torch.testing.assert_close(mr_big, mr_small, rtol=2e-5, atol=2e-5)
    rows = _sample_rows()
    ref = (F.linear(x[0, rows].double().cpu(), w.double(), b.double()) * 0.75 + res[0, rows].double().cpu())
    torch.testing.assert_close(big[0, rows].double().cpu(), ref, rtol=1e-2, atol=2e-2)
    mean, var = ref.mean(-1), ref.var(-1, unbiased=False)
    torch.testing.assert_close(mr_big[rows.to(DEV), 0].double().cpu(), mean, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(mr_big[rows.to(DEV), 1].double().cpu(), (var + 1e-5).rsqrt(), rtol=1e-4, atol=1e-4)


def test_groupnorm_partials_from_the_epilogue(ops):
    """NHWC form (16 samples of 64x64): the proj_out shape.  The row-panel kernel emits one partial per 32-row wave panel
    (128 chunks per sample); the tile kernels chunk by their own wave rows: same (scale, shift) after the finalize."""
    g = torch.Generator().manual_seed(3)
    n, hw, c = 16, 64, 320
    x = torch.randn(n, hw, hw, K, generator=g).to(DEV, torch.bfloat16)
    res = torch.randn(n, hw, hw, c, generator=g).to(DEV, torch.bfloat16)
    w = bf(torch.randn(c, K, 1, 1, generator=g) / math.sqrt(K))
    b = torch.randn(c, generator=g)
    pc = ops.PackedConv(w, b, DEV)
    big = _on("gemm_rowpanel", lambda: ops.conv(x, pc, residual=res, gn_part=True))
    assert hasattr(big, "gn_part") and big.gn_part.shape[0] == hw * hw // 32      # one partial per 32-row wave panel
    gamma, beta = (1 + 0.1 * torch.randn(c, generator=g)).to(DEV), (0.1 * torch.randn(c, generator=g)).to(DEV)
    ab_big = ops.group_norm_ab(big, gamma, beta, 32, 1e-5)
    smalls = [ops.conv(x[i:i + 2], pc, residual=res[i:i + 2], gn_part=True) for i in range(0, n, 2)]
    assert torch.equal(big, torch.cat(smalls, 0))
    ab_small = torch.cat([ops.group_norm_ab(s, gamma, beta, 32, 1e-5) for s in smalls], 0)
    torch.testing.assert_close(ab_big, ab_small, rtol=1e-4, atol=1e-4)
    ab_read = ops.group_norm_ab(big.clone(), gamma, beta, 32, 1e-5)               # read pass over the stored tensor
    torch.testing.assert_close(ab_big, ab_read, rtol=5e-3, atol=5e-3)


def test_folded_layernorm_qkv(ops):
    g = torch.Generator().manual_seed(4)
    n_out = 960
    x = _rows(g, M, K, 1.5)
    w = torch.randn(n_out, K, generator=g) / math.sqrt(K)
    gamma, beta = 1 + 0.2 * torch.randn(K, generator=g), 0.2 * torch.randn(K, generator=g)
    pc = ops.PackedConv(w, None, DEV, ln=(gamma, beta, 1e-5))
    mr = ops.ln_finalize(ops.row_stats(x), K, 1e-5)
    big = _on("gemm_rowpanel", lambda: ops.linear(x, pc, ln_stats=mr))
    small = torch.cat([ops.linear(x[:, i:i + CH], pc, ln_stats=mr[i:i + CH]) for i in range(0, M, CH)], 1)
    assert torch.equal(big, small)
    rows = _sample_rows()
    ref = F.linear(F.layer_norm(x[0, rows].double().cpu(), (K,), gamma.double(), beta.double(), 1e-5), w.double())
    torch.testing.assert_close(big[0, rows].double().cpu(), ref, rtol=2e-2, atol=3e-2)


@pytest.mark.parametrize("ln", [False, True])
def test_geglu_feed_forward(ops, ln):
    g = torch.Generator().manual_seed(5 + int(ln))
    n_out = 2560
    x = _rows(g, M, K, 1.5)
    w = torch.randn(n_out, K, generator=g) / math.sqrt(K)
    b = 0.1 * torch.randn(n_out, generator=g)
    lnp = (1 + 0.2 * torch.randn(K, generator=g), 0.2 * torch.randn(K, generator=g), 1e-5) if ln else None
    pc = ops.PackedConv(w, b, DEV, geglu=True, ln=lnp)
    mr = ops.ln_finalize(ops.row_stats(x), K, 1e-5) if ln else None
    kw = lambda i: dict(ln_stats=mr[i:i + CH]) if ln else {}
    big = _on("gemm_rowpanel", lambda: ops.linear(x, pc, **(dict(ln_stats=mr) if ln else {})))
    assert big.shape == (1, M, n_out // 2)
    small = torch.cat([ops.linear(x[:, i:i + CH], pc, **kw(i)) for i in range(0, M, CH)], 1)
    assert torch.equal(big, small)
    rows = _sample_rows()
    xr = x[0, rows].double().cpu()
    if ln:
        xr = F.layer_norm(xr, (K,), lnp[0].double(), lnp[1].double(), 1e-5)
        y = F.linear(xr, w.double(), b.double())
    else:
        y = F.linear(xr, bf(w).double(), b.double())
    h, gate = y.chunk(2, -1)
    torch.testing.assert_close(big[0, rows].double().cpu(), h * F.gelu(gate), rtol=2e-2, atol=3e-2)


def test_full_batch_shape_131072_rows(ops):
    """The bench shape (model batch 32 x 4096 rows): two panels per CU."""
    g = torch.Generator().manual_seed(9)
    m = 131072
    x = _rows(g, m, K)
    w = bf(torch.randn(320, K, generator=g) / math.sqrt(K))
    b = torch.randn(320, generator=g)
    pc = ops.PackedConv(w, b, DEV)
    big = _on("gemm_rowpanel", lambda: ops.linear(x, pc))
    small = torch.cat([ops.linear(x[:, i:i + CH], pc) for i in range(0, m, CH)], 1)
    assert torch.equal(big, small)


@pytest.mark.parametrize("m", [M, CH])
def test_layernorm_finalize_folded_into_the_consumer(ops, m):
    """dc_conv_desc.ln_parts: the consumer takes the producer's RAW row partials and forms (mean, rstd) itself — in its prologue
    on the row-panel kernel (m = 65,536), through the finalize pass the dispatcher launches into the caller's scratch on the tile
    kernels (m = 16,384).  One device function holds the arithmetic, so both equal `ln_stats=ln_finalize(partials)` bit for bit."""
    g = torch.Generator().manual_seed(21)
    x = _rows(g, m, K, 1.5)
    w0 = bf(torch.randn(K, K, generator=g) / math.sqrt(K))
    parts = ops.row_stats_parts(K)
    st = torch.empty((m, parts, 2), device=DEV)
    t = ops.linear(x, ops.PackedConv(w0, torch.randn(K, generator=g), DEV), residual=x, stats_out=st)   # a producer with statistics
    gamma, beta = 1 + 0.2 * torch.randn(K, generator=g), 0.2 * torch.randn(K, generator=g)
    for n_out, geglu in ((960, False), (2560, True)):
        pc = ops.PackedConv(torch.randn(n_out, K, generator=g) / math.sqrt(K), 0.1 * torch.randn(n_out, generator=g), DEV,
                            geglu=geglu, ln=(gamma, beta, 1e-5))
        a = ops.linear(t, pc, ln_stats=ops.ln_finalize(st, K, 1e-5))
        b = _on("gemm_rowpanel" if m == M else "gemm_dma", lambda: ops.linear(t, pc, ln_partials=(st, 1e-5)), ln_first=m != M)
        assert torch.equal(a, b)
    one = ops.row_stats(t)                                                       # the single-part form (row_stats)
    pc = ops.PackedConv(torch.randn(320, K, generator=g) / math.sqrt(K), None, DEV, ln=(gamma, beta, 1e-5))
    assert torch.equal(ops.linear(t, pc, ln_stats=ops.ln_finalize(one, K, 1e-5)), ops.linear(t, pc, ln_partials=(one, 1e-5)))


def test_groupnorm_affine_on_load_equals_the_standalone_pass(ops):
    """dc_conv_desc.gn_ab on the row-panel GEMM (the transformer's GroupNorm in front of proj_in at 64x64): the affine is applied to the
    register-resident activation panel with the arithmetic of dc_gn_apply_nhwc_bf16 (one shared device function), so the launch must
    equal `conv(gn_apply(x))` bit for bit — output and row statistics — and match a float64 GroupNorm + linear."""
    g = torch.Generator().manual_seed(31)
    n, hw, c = 16, 64, 320
    x = (torch.randn(n, hw, hw, c, generator=g) * 1.5 + 0.3).to(DEV, torch.bfloat16)
    gamma, beta = (1 + 0.2 * torch.randn(c, generator=g)), 0.2 * torch.randn(c, generator=g)
    w = bf(torch.randn(c, c, 1, 1, generator=g) / math.sqrt(c))
    b = torch.randn(c, generator=g)
    pc = ops.PackedConv(w, b, DEV)
    ab = ops.group_norm_ab(x, gamma.to(DEV), beta.to(DEV), 32, 1e-6)
    parts = ops.row_stats_parts(c)
    st_a = torch.full((n * hw * hw, parts, 2), float("nan"), device=DEV)
    st_b = torch.empty_like(st_a)
    fused = _on("gemm_rowpanel", lambda: ops.conv(x, pc, gn_ab=ab, gn_silu=False, stats_out=st_a))
    two_pass = ops.conv(ops.gn_apply(x, ab), pc, stats_out=st_b)
    assert torch.equal(fused, two_pass)
    assert torch.equal(st_a, st_b)
    assert torch.equal(fused, ops.conv(x, pc, gn_ab=ab, gn_silu=False))            # with or without the statistics by-product
    xs = x[:2].double().cpu()
    ref = F.group_norm(xs.permute(0, 3, 1, 2), 32, gamma.double(), beta.double(), 1e-6).permute(0, 2, 3, 1)
    ref = F.linear(ref, w.double().reshape(c, c), b.double())
    torch.testing.assert_close(fused[:2].double().cpu(), ref, rtol=2e-2, atol=4e-2)
    with pytest.raises(Exception):                                                 # SiLU on load has no statistics epilogue anywhere
        ops.conv(x, pc, gn_ab=ab, gn_silu=True, stats_out=st_a)


@pytest.mark.parametrize("m,k", [(32768, 640), (8192, 1280), (2048, 1280), (512, 640), (4096, 320)])
def test_layernorm_finalize_folded_into_the_tile_gemms(ops, m, k):
    """dc_conv_desc.ln_parts on launches the 128-row and the 256-row ping-pong GEMMs take (every transformer level below 64x64, and
    every level of a one-frame decode): the dispatcher runs dc_ln_finalize into the caller's scratch and proceeds on (mean, rstd)
    pairs — the arithmetic of the explicit finalize, so it equals `ln_stats=ln_finalize(partials)` bit for bit, with 4 / 8 / 16
    partials per row.  (Folding the finalize INTO those kernels was measured and dropped: every N tile redoes it — DESIGN.md §5.)"""
    g = torch.Generator().manual_seed(41 + k)
    x = _rows(g, m, k, 1.5)
    parts = ops.row_stats_parts(k)
    st = torch.empty((m, parts, 2), device=DEV)
    t = ops.linear(x, ops.PackedConv(bf(torch.randn(k, k, generator=g) / math.sqrt(k)), torch.randn(k, generator=g), DEV), residual=x, stats_out=st)
    gamma, beta = 1 + 0.2 * torch.randn(k, generator=g), 0.2 * torch.randn(k, generator=g)
    for n_out, geglu in ((3 * k, False), (k, False), (8 * k, True)):
        pc = ops.PackedConv(torch.randn(n_out, k, generator=g) / math.sqrt(k), 0.1 * torch.randn(n_out, generator=g), DEV,
                            geglu=geglu, ln=(gamma, beta, 1e-5))
        a = ops.linear(t, pc, ln_stats=ops.ln_finalize(st, k, 1e-5))
        with capture_routes() as routes:
            b = ops.linear(t, pc, ln_partials=(st, 1e-5))
        assert [(r.kernel in ("gemm_dma", "gemm_wide", "gemm_p8"), r.ln_first) for r in routes] == [(True, True)], routes
        assert torch.equal(a, b)
