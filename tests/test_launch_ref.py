"""CPU: the fp64 launch references of oracle/launch_ref.py equal the torch formulas, unpack every PackedConv layout, and the
checker accepts a correct bf16 result computed in another accumulation order while rejecting realistic kernel faults."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import launch_ref as L

BF = torch.bfloat16


def _packed(cin, cout, k, **kw):
    from diffcodec_amd.ops import PackedConv
    g = torch.Generator().manual_seed(cin * 7 + cout + k)
    w = torch.randn(cout, cin, k, k, generator=g) / math.sqrt(cin * k * k)
    b = torch.randn(cout, generator=g) * 0.1
    return PackedConv(w, b, "cpu", **kw), w, b


def _wq(pc):
    """checkpoint-order weights as stored (bf16-rounded) -> OIHW fp32"""
    w, b = L.unpack_weight(pc)
    k = pc.ksize
    return w.reshape(pc.cout, k, k, pc.cin).permute(0, 3, 1, 2).float(), None if b is None else b.float()


def _x(n, h, w, c, seed=0, mean=0.0):
    return (torch.randn(n, h, w, c, generator=torch.Generator().manual_seed(seed)) + mean).to(BF)


def _torch_conv(x, pc, *, x2=None, gn_ab=None, gn_silu=False, stride=1, pad=1, upsample=False):
    xx = x.float() if x2 is None else torch.cat([x.float(), x2.float()], -1)
    if gn_ab is not None:
        ab = gn_ab[torch.arange(xx.shape[0]) % gn_ab.shape[0]]
        xx = xx * ab[:, None, None, :, 0] + ab[:, None, None, :, 1]
        if gn_silu:
            xx = F.silu(xx)
    t = xx.permute(0, 3, 1, 2)
    if upsample:
        t = F.interpolate(t, scale_factor=2, mode="nearest")
    w, b = _wq(pc)
    if pc.ksize == 3 and not pad:
        t = F.pad(t, (0, 1, 0, 1))
    y = F.conv2d(t, w, b, stride=stride, padding=1 if (pc.ksize == 3 and pad) else 0)
    return y.permute(0, 2, 3, 1)


def _all_rows(y):
    return torch.arange(y.numel() // y.shape[-1])


@pytest.mark.parametrize("k,stride,pad,up", [(1, 1, 1, False), (3, 1, 1, False), (3, 2, 1, False), (3, 2, 0, False), (3, 1, 1, True)])
@pytest.mark.parametrize("cat,gn,silu", [(False, False, False), (True, True, True), (False, True, False)])
def test_conv_ref_equals_torch(k, stride, pad, up, cat, gn, silu):
    pc, _, _ = _packed(128, 32, k)
    x1 = _x(2, 6, 10, 64 if cat else 128, 1)
    x2 = _x(2, 6, 10, 64, 2) if cat else None
    ab = torch.randn(2, 128, 2, generator=torch.Generator().manual_seed(3)) if gn else None
    ref = _torch_conv(x1, pc, x2=x2, gn_ab=ab, gn_silu=silu, stride=stride, pad=pad, upsample=up)
    rows = _all_rows(ref)
    r, s = L.conv_ref(x1, pc, rows, x2=x2, gn_ab=ab, gn_silu=silu, stride=stride, pad=pad, upsample=up)
    assert torch.allclose(r.float(), ref.reshape(-1, 32), atol=1e-4, rtol=1e-4)
    assert (s >= 0).all()


def test_conv_ref_epilogue_fusions():
    pc, _, _ = _packed(64, 48, 1)
    x = _x(3, 4, 4, 64, 4)
    ra = torch.randn(3, 48, generator=torch.Generator().manual_seed(5))
    res = _x(3, 4, 4, 48, 6)
    for act, fn in ((0, lambda z: z), (1, F.silu), (2, lambda z: z * torch.sigmoid(1.702 * z))):
        z = _torch_conv(x, pc) + ra[:, None, None, :]
        ref = fn(z) * 0.7 + res.float()
        r, _ = L.conv_ref(x, pc, _all_rows(ref), row_add=ra, residual=res, out_scale=0.7, act=act)
        assert torch.allclose(r.float(), ref.reshape(-1, 48), atol=1e-4, rtol=1e-4), act


def test_geglu_and_folded_layernorm_unpack():
    from diffcodec_amd.ops import PackedConv
    g = torch.Generator().manual_seed(9)
    w, b = torch.randn(128, 64, generator=g) / 8, torch.randn(128, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(64, generator=g), 0.1 * torch.randn(64, generator=g)
    x = _x(1, 1, 40, 64, 10, mean=1.5)
    # GEGLU: packed rows interleaved 16 | 16, the reference undoes it
    pc = PackedConv(w, b, "cpu", geglu=True)
    wq, bq = _wq(pc)
    hg = F.linear(x.float().reshape(-1, 64), wq[:, :, 0, 0], bq)
    ref = hg[:, :64] * F.gelu(hg[:, 64:])
    r, _ = L.conv_ref(x, pc, torch.arange(40))
    assert torch.allclose(r.float(), ref, atol=1e-4, rtol=1e-4)
    # folded LayerNorm (+ GEGLU): Linear(LN(x)) with the stored W', b'
    pc = PackedConv(w, b, "cpu", geglu=True, ln=(gamma, beta, 1e-5))
    wq, bq = _wq(pc)
    xl = F.layer_norm(x.double().reshape(-1, 64), (64,), eps=1e-5)
    hg = xl @ wq[:, :, 0, 0].double().T + bq.double()
    ref = hg[:, :64] * F.gelu(hg[:, 64:])
    r, _ = L.conv_ref(x, pc, torch.arange(40))
    assert torch.allclose(r, ref, atol=1e-9, rtol=1e-9)
    # and W' = W diag(gamma), b' = b + W beta up to the bf16 rounding of W'
    pc = PackedConv(w, b, "cpu", ln=(gamma, beta, 1e-5))
    wq, bq = _wq(pc)
    assert torch.allclose(wq[:, :, 0, 0], w * gamma, rtol=2 ** -8, atol=1e-6)
    assert torch.allclose(bq, b + w @ beta, atol=1e-5)


@pytest.mark.parametrize("cin,cout,kw", [(4, 320, {}), (320, 4, {}), (320, 4, {"mfma_small_cout": True}), (128, 8, {})])
def test_every_packed_layout_unpacks(cin, cout, kw):
    pc, w, b = _packed(cin, cout, 3, **kw)
    assert pc.kind == {(4, 320): "small_cin", (128, 8): "small_cout"}.get((cin, cout), "small_cout" if not kw else "igemm")
    wq, bq = _wq(pc)
    assert torch.equal(wq, w.to(BF).float()) and torch.allclose(bq, b)
    x = _x(1, 5, 7, cin, 11)
    ref = _torch_conv(x, pc)
    r, _ = L.conv_ref(x, pc, _all_rows(ref))
    assert torch.allclose(r.float(), ref.reshape(-1, cout), atol=1e-4, rtol=1e-4)


def test_attention_refs_equal_explicit_softmax():
    g = torch.Generator().manual_seed(12)
    qkv = torch.randn(2, 24, 3 * 64, generator=g).to(BF)
    q, k, v = qkv[..., :64], qkv[..., 64:128], qkv[..., 128:]
    rows = torch.arange(48)
    for causal in (False, True):
        r, s = L.attention_ref(q, k, v, 4, rows, causal=causal)
        qq, kk, vv = (t.float().reshape(2, 24, 4, 16).transpose(1, 2) for t in (q, k, v))
        lg = qq @ kk.transpose(-1, -2) / 4.0
        if causal:
            lg = lg.masked_fill(torch.ones(24, 24, dtype=torch.bool).triu(1), -math.inf)
        ref = (torch.softmax(lg, -1) @ vv).transpose(1, 2).reshape(48, 64)
        assert torch.allclose(r.float(), ref, atol=1e-5)


def test_norm_refs_equal_torch():
    g = torch.Generator().manual_seed(13)
    x, x2 = _x(2, 4, 4, 64, 14, mean=0.5), _x(2, 4, 4, 32, 15)
    gamma, beta = torch.randn(96, generator=g), torch.randn(96, generator=g)
    ab, st = L.group_norm_ab_ref(x, gamma, beta, 32, 1e-6, x2=x2)
    xx = torch.cat([x.float(), x2.float()], -1).permute(0, 3, 1, 2)
    ref = F.group_norm(xx.double(), 32, gamma.double(), beta.double(), 1e-6).permute(0, 2, 3, 1)
    y = xx.double().permute(0, 2, 3, 1) * ab[:, None, None, :, 0] + ab[:, None, None, :, 1]
    assert torch.allclose(y, ref, atol=1e-9)
    assert L.check_group_norm_ab(ab.float(), ab, st)["ok"]
    bad = ab.clone()
    bad[1, 40:43, 1] += 0.02 * ab[1, 40:43, 0]                      # one group's shift off by 2 % of a standard deviation
    assert not L.check_group_norm_ab(bad.float(), ab, st)["ok"]
    rows = torch.arange(32)
    r, _ = L.gn_apply_ref(x, ab.float(), rows, silu=True, x2=x2)
    assert torch.allclose(r, F.silu(ref.reshape(32, 96)), atol=1e-6)
    gm, bt = gamma[:64], beta[:64]
    r, _ = L.layer_norm_ref(x, gm, bt, 1e-5, rows)
    assert torch.allclose(r, F.layer_norm(x.double().reshape(32, 64), (64,), gm.double(), bt.double(), 1e-5), atol=1e-9)
    fg, fb = _x(1, 4, 4, 64, 16), _x(1, 4, 4, 64, 17)
    r, _ = L.fdn_modulate_ref(x, ab[:, :64].float(), fg, fb, rows)
    ref = (x.double() * ab[:, None, None, :64, 0] + ab[:, None, None, :64, 1]) * (1 + fg.double()) + fb.double()
    assert torch.allclose(r, ref.reshape(32, 64), atol=1e-6)
    st, _ = L.row_stats_ref(x, rows)
    xr = x.double().reshape(32, 64)
    assert torch.allclose(st[:, 0], torch.stack([xr.sum(1), (xr * xr).sum(1)], 1))
    mr, _ = L.ln_finalize_ref(st.float(), 64, 1e-5, rows)
    assert torch.allclose(mr[:, 0], xr.mean(1), atol=1e-6)
    assert torch.allclose(mr[:, 1], 1 / torch.sqrt(xr.var(1, unbiased=False) + 1e-5), rtol=1e-5)


def test_elementwise_refs():
    g = torch.Generator().manual_seed(18)
    s = torch.randn(8, 40, generator=g)
    p, _ = L.softmax_rows_ref(s, 0.3, torch.arange(8))
    assert torch.allclose(p, torch.softmax(s.double() * 0.3, 1))
    x = torch.randn(3, 5, 7, generator=g).to(BF)
    t, _ = L.transpose_ref(x, torch.arange(21))
    assert torch.equal(t, x.transpose(1, 2).reshape(21, 5).double())
    x = _x(2, 8, 8, 32, 19)
    r, _ = L.freeu_backbone_ref(x, 1.4, torch.arange(128))
    assert torch.equal(r[:, 16:], x.reshape(-1, 32)[:, 16:].double()) and torch.allclose(r[:, :16], 1.4 * x.reshape(-1, 32)[:, :16].double())
    r, _ = L.freeu_lowfreq_ref(x, 0.9, torch.arange(128))
    xf = x.double().permute(0, 3, 1, 2)
    X = torch.fft.fftshift(torch.fft.fftn(xf, dim=(-2, -1)), dim=(-2, -1))
    m = torch.ones(8, 8, dtype=torch.float64)
    m[3:5, 3:5] = 0.9                                           # diffusers fourier_filter, threshold 1
    ref = torch.fft.ifftn(torch.fft.ifftshift(X * m, dim=(-2, -1)), dim=(-2, -1)).real.permute(0, 2, 3, 1).reshape(-1, 32)
    assert torch.allclose(r, ref, atol=1e-9)
    r, _ = L.timestep_embedding_ref(951.0, 2, 320)
    f = torch.exp(-math.log(10000) * torch.arange(160, dtype=torch.float64) / 160)
    assert torch.allclose(r[1], torch.cat([torch.cos(951 * f), torch.sin(951 * f)]))


# ------------------------------------------------------------------------------------------ the checker catches faults
M_T, N_T, K_T = 1024, 64, 256            # four 256-row tiles, one 64-wide N tile per 16-column fragment group, four 64-wide K chunks


def _gemm_case():
    from diffcodec_amd.ops import PackedConv
    g = torch.Generator().manual_seed(21)
    w = torch.randn(N_T, K_T, generator=g) / 16
    b = torch.randn(N_T, generator=g)
    pc = PackedConv(w, b, "cpu")
    x = torch.randn(1, 1, M_T, K_T, generator=g).to(BF)
    wq, bq = L.unpack_weight(pc)
    return pc, x, wq[:, 0].float(), bq.float()


def _verdict(y, pc, x, **kw):
    rows = L.sample_rows(M_T)
    r, s = L.conv_ref(x, pc, rows, **kw)
    return L.check(y.reshape(-1, y.shape[-1])[rows], r, s, y.dtype)


def _fp32_gemm(x, w, order=1):
    """fp32 accumulation over 64-wide K chunks, in a given chunk order (a different kernel's summation order)"""
    xs = x.float().reshape(-1, K_T)
    acc = torch.zeros(xs.shape[0], w.shape[0])
    chunks = list(range(0, K_T, 64))[::order]
    for c in chunks:
        acc = acc + xs[:, c:c + 64] @ w[:, c:c + 64].T
    return acc


def test_checker_accepts_another_accumulation_order():
    pc, x, w, b = _gemm_case()
    for order in (1, -1):
        y = (_fp32_gemm(x, w, order) + b).to(BF)
        v = _verdict(y, pc, x)
        assert v["ok"], v
        assert v["ratio"] < 0.75            # one bf16 rounding: at most half an ulp, e_out is one


FAULTS = ["k_chunk_missing", "fragment_transposed", "rows_swapped", "tile_zero", "tile_duplicate", "bias_missing_n_tile"]


@pytest.mark.parametrize("fault", FAULTS)
def test_checker_rejects_gemm_faults(fault):
    pc, x, w, b = _gemm_case()
    acc = _fp32_gemm(x, w)
    t = 2                                   # the faulty 256-row tile
    lo, hi = t * 256, (t + 1) * 256
    if fault == "k_chunk_missing":
        acc[lo:hi] -= x.float().reshape(-1, K_T)[lo:hi, 64:128] @ w[:, 64:128].T
    y = acc + b
    if fault == "fragment_transposed":
        y[lo:lo + 16, 16:32] = y[lo:lo + 16, 16:32].T.clone()
    elif fault == "rows_swapped":
        ra, rb = lo + 5, lo + 64 + 37 * t % 64          # two rows of the tile (one of them a sampled row)
        y[[ra, rb]] = y[[rb, ra]]
    elif fault == "tile_zero":
        y[lo:hi] = 0
    elif fault == "tile_duplicate":
        y[lo:hi] = y[lo - 256:lo].clone()
    elif fault == "bias_missing_n_tile":
        y[:, 32:48] -= b[32:48]
    v = _verdict(y.to(BF), pc, x)
    assert not v["ok"], (fault, v)


def test_checker_rejects_epilogue_faults():
    pc, x, w, b = _gemm_case()
    res = torch.randn(1, 1, M_T, N_T, generator=torch.Generator().manual_seed(22)).to(BF)
    z = _fp32_gemm(x, w) + b
    good = (z * 0.5 + res.reshape(-1, N_T).float()).to(BF)
    assert _verdict(good, pc, x, residual=res, out_scale=0.5)["ok"]
    twice = (z * 0.5 + 2 * res.reshape(-1, N_T).float()).to(BF)
    assert not _verdict(twice, pc, x, residual=res, out_scale=0.5)["ok"]
    scaled = ((z + res.reshape(-1, N_T).float()) * 0.5).to(BF)
    assert not _verdict(scaled, pc, x, residual=res, out_scale=0.5)["ok"]


def test_checker_rejects_geglu_halves_swapped_and_stale_layernorm_stats():
    from diffcodec_amd.ops import PackedConv
    g = torch.Generator().manual_seed(23)
    w, b = torch.randn(128, 256, generator=g) / 16, torch.randn(128, generator=g)
    x = (torch.randn(1, 1, 512, 256, generator=g) * (1 + torch.arange(512.0)[:, None] / 64) + torch.randn(512, 1, generator=g)).to(BF)
    pc = PackedConv(w, b, "cpu", geglu=True)
    wq, bq = L.unpack_weight(pc)
    hg = x.double().reshape(-1, 256) @ wq[:, 0].T + bq
    rows = L.sample_rows(512)
    r, s = L.conv_ref(x, pc, rows)
    good = (hg[:, :64] * F.gelu(hg[:, 64:])).to(BF)
    swapped = (hg[:, 64:] * F.gelu(hg[:, :64])).to(BF)
    assert L.check(good[rows], r, s, BF)["ok"]
    assert not L.check(swapped[rows], r, s, BF)["ok"]
    gamma, beta = 1 + 0.1 * torch.randn(256, generator=g), 0.1 * torch.randn(256, generator=g)
    pc = PackedConv(w[:64], b[:64], "cpu", ln=(gamma, beta, 1e-5))
    wq, bq = L.unpack_weight(pc)
    xr = x.double().reshape(-1, 256)
    mean, var = xr.mean(1, keepdim=True), xr.var(1, unbiased=False, keepdim=True)
    fold = lambda m, v: ((xr - m) / torch.sqrt(v + 1e-5)) @ wq[:, 0].T + bq
    r, s = L.conv_ref(x, pc, rows)
    assert L.check(fold(mean, var).to(BF)[rows], r, s, BF)["ok"]
    stale = fold(torch.roll(mean, 1, 0), torch.roll(var, 1, 0)).to(BF)          # every row fed the previous row's statistics
    assert not L.check(stale[rows], r, s, BF)["ok"]


def test_checker_rejects_a_skipped_key_block():
    g = torch.Generator().manual_seed(24)
    q, k, v = (torch.randn(1, 256, 64, generator=g).to(BF) for _ in range(3))
    rows = torch.arange(256)
    r, s = L.attention_ref(q, k, v, 2, rows)
    good = r.to(BF)
    assert L.check(good, r, s, BF)["ok"]
    kk = k.clone()
    sel = torch.ones(256, dtype=torch.bool)
    sel[64:128] = False                                           # head 1 skips its second 64-key block
    qq, kh, vh = q[0, :, 32:].double(), k[0, sel, 32:].double(), v[0, sel, 32:].double()
    bad = r.clone()
    bad[:, 32:] = torch.softmax(qq @ kh.T / math.sqrt(32), -1) @ vh
    assert not L.check(bad.to(BF), r, s, BF)["ok"]


# ------------------------------------------------------------------------------------------ the row sampler
def test_sampler_touches_every_tile_residue_border_and_boundary():
    M = 88 * 64 * 64
    rows = L.sample_rows(M, spatial=(88, 64, 64))
    assert rows[0] == 0 and rows[-1] == M - 1 and (rows[:256] == torch.arange(256)).all()
    assert set((rows // 256).tolist()) == set(range(M // 256))                    # every 256-row block (so every M tile)
    for tile in (64, 128, 256):
        assert set((rows // tile).tolist()) == set(range(M // tile))
    assert set((rows % 64).tolist()) == set(range(64))
    for n in range(88):
        s = set(rows[(rows // 4096) == n].tolist())
        base = n * 4096
        oy, ox = (0, 63) if n % 2 == 0 else (63, 0)
        assert all(base + oy * 64 + i in s for i in range(64)) and all(base + i * 64 + ox in s for i in range(64))
    # the VAE's last up-block of a 44-frame call: 44 x 512 x 512 rows of 256 bf16 channels (5.8 GB)
    M, rb = 44 * 512 * 512, 256 * 2
    rows = set(L.sample_rows(M, row_bytes=[rb]).tolist())
    for lim in (2 ** 31, 2 ** 32):
        r = lim // rb
        assert all(i in rows for i in range(r - 128, r + 128))


@pytest.mark.parametrize("stride,silu", [(1, True), (2, False), (2, True)])
def test_conv3x3_nchw_f32_ref_equals_torch(stride, silu):
    g = torch.Generator().manual_seed(30 + stride)
    full = torch.randn(2, 24, 9, 11, generator=g)
    x = full[:, 4:20]                                            # a channel-slice view, as the extractors pass
    w, b = torch.randn(8, 16, 3, 3, generator=g) / 12, torch.randn(8, generator=g)
    ref = F.conv2d(x.double(), w.double(), b.double(), stride=stride, padding=1)
    if silu:
        ref = F.silu(ref)
    n, co, ho, wo = ref.shape
    rows = L.sample_rows(n * ho * wo, spatial=(n, ho, wo))
    r, s = L.conv3x3_nchw_f32_ref(x, w, b, rows, stride=stride, silu=silu)
    assert torch.allclose(r, ref.permute(0, 2, 3, 1).reshape(-1, co)[rows], atol=1e-12)
    y = F.conv2d(x, w, b, stride=stride, padding=1)
    y = (F.silu(y) if silu else y).permute(0, 2, 3, 1).reshape(-1, co)[rows]
    assert L.check(y, r, s, torch.float32)["ok"]                # torch's own fp32 conv: another accumulation order
    bad = y.clone()
    bad[3, 2] *= 1 + 2 ** -12                                    # a bf16-class error is far outside an fp32 launch's bound
    assert not L.check(bad, r, s, torch.float32)["ok"]


# ------------------------------------------------------------------------------------------ loop-state kernels
def _ddim_f32(eps, lat, row, guidance, cfg, B):
    """the kernel's arithmetic restated in fp32 (torch on the CPU: every operation rounds to fp32)"""
    s1mat, sat, sap, s1map = row.to(torch.float32)
    e = eps.permute(0, 3, 1, 2)
    if cfg:
        eu, et = e[:B], e[B:]
        e = eu + torch.tensor(guidance, dtype=torch.float32) * (et - eu)
    x0 = (lat - s1mat * e) / sat
    return sap * x0 + s1map * e


@pytest.mark.parametrize("cfg", [True, False])
@pytest.mark.parametrize("t", [981, 951, 501, 1])
def test_cfg_ddim_step_ref_passes_fp32_and_rejects_faults(t, cfg):
    """cfg_ddim_step_ref on the rows t = 981, 951, 501 and 1 of the scaled-linear table: the fp32 restatement passes; a neighbouring
    coefficient row, swapped CFG halves, ignored guidance and an epsilon rounded to bf16 fail"""
    import edge_cases as E
    ts, table = E.ddim_table()
    i = ts.index(t)
    shape = E.STATE_SHAPES[0]
    B = shape[0]
    eps, lat = E.ddim_inputs(shape, cfg, 9000 + t)
    g = E.STATE_GUIDANCE if cfg else 1.0
    r, s = L.cfg_ddim_step_ref(eps, lat, table[i], g, cfg, B)
    assert r.shape == lat.shape and r.dtype == torch.float64
    v = L.check(_ddim_f32(eps, lat, table[i], g, cfg, B), r, s, torch.float32)
    assert v["ok"], v
    faults = {"next row": _ddim_f32(eps, lat, table[i + 1 if i + 1 < len(ts) else i - 1], g, cfg, B),
              "previous row": _ddim_f32(eps, lat, table[i - 1], g, cfg, B),
              "bf16 eps": _ddim_f32(eps.to(BF).float(), lat, table[i], g, cfg, B)}
    if cfg:
        faults["swapped halves"] = _ddim_f32(torch.cat([eps[B:], eps[:B]]), lat, table[i], g, cfg, B)
        faults["guidance ignored"] = _ddim_f32(eps, lat, table[i], 1.0, cfg, B)
    for name, bad in faults.items():
        assert not L.check(bad, r, s, torch.float32)["ok"], (t, cfg, name)


def _vae_f32(mom, noise, scale, lo=-30.0, hi=20.0, half=0.5, swap=False):
    c = noise.shape[1]
    mean, lv = mom[..., :c].permute(0, 3, 1, 2), mom[..., c:].permute(0, 3, 1, 2)
    if swap:
        mean, lv = lv, mean
    return (mean + torch.exp(torch.tensor(half) * lv.clamp(lo, hi)) * noise) * torch.tensor(scale, dtype=torch.float32)


def test_vae_sample_latents_ref_passes_fp32_and_rejects_faults():
    import edge_cases as E
    mom, noise = E.vae_inputs(E.STATE_SHAPES[0], 9100)
    c = noise.shape[1]
    lv = mom[..., c:]
    for v in (-45.0, -30.0, 20.0, 33.0):                          # beyond both clamps and exactly on them
        assert int((lv == v).sum()) >= 4, v
    scale = 0.18215
    r, s = L.vae_sample_latents_ref(mom, noise, scale)
    ok = L.check(_vae_f32(mom, noise, scale), r, s, torch.float32)
    assert ok["ok"], ok
    inf = float("inf")
    faults = {"no upper clamp": _vae_f32(mom, noise, scale, hi=inf), "no lower clamp": _vae_f32(mom, noise, scale, lo=-inf),
              "no scale": _vae_f32(mom, noise, 1.0), "exp(lv)": _vae_f32(mom, noise, scale, half=1.0),
              "mean and log-variance swapped": _vae_f32(mom, noise, scale, swap=True)}
    for name, bad in faults.items():
        assert not L.check(bad, r, s, torch.float32)["ok"], name
    # scale 1 (the encoder path of vae.py) is held by the same bound
    r1, s1 = L.vae_sample_latents_ref(mom, noise, 1.0)
    assert L.check(_vae_f32(mom, noise, 1.0), r1, s1, torch.float32)["ok"]


@pytest.mark.parametrize("mul,rep", [(1.0, 1), (1.0, 2), (1.0 / 0.18215, 1), (1.0 / 0.18215, 2)])
def test_latents_to_model_input_ref_passes_fp32_and_rejects_faults(mul, rep):
    g = torch.Generator().manual_seed(9200)
    lat = torch.randn(3, 4, 5, 7, generator=g)
    r, s = L.latents_to_model_input_ref(lat, mul, rep)
    assert r.shape == (3 * rep, 5, 7, 4)
    good = (lat * torch.tensor(mul, dtype=torch.float32)).to(BF).permute(0, 2, 3, 1).repeat(rep, 1, 1, 1)
    assert L.check(good, r, s, BF)["ok"]
    nchw = (lat * torch.tensor(mul, dtype=torch.float32)).to(BF).reshape(3, 5, 7, 4).repeat(rep, 1, 1, 1)      # layout not changed
    assert not L.check(nchw, r, s, BF)["ok"]
    trunc = ((lat * torch.tensor(mul, dtype=torch.float32)).view(torch.int32) & ~0xFFFF).view(torch.float32)   # truncated, not rounded
    assert not L.check(trunc.permute(0, 2, 3, 1).repeat(rep, 1, 1, 1), r, s, BF)["ok"]
    if mul != 1.0:
        assert not L.check(lat.to(BF).permute(0, 2, 3, 1).repeat(rep, 1, 1, 1), r, s, BF)["ok"]


# ------------------------------------------------------------------------------------------ control stage and plain elementwise launches
# For every table case of tests/edge_cases.py (all but the one beyond a single grid), on the case's own inputs: the project's fp32 CPU
# restatement (the C oracle, oracle/control_ref.py, plain torch fp32) passes the check the GPU edge test applies, and a seeded fault
# fails it wherever it moves the result by more than FAULT_MATERIAL — and it does so on the cases the table holds for it.
import edge_cases as E                                                # noqa: E402
from oracle import control_ref as CR                                  # noqa: E402
from oracle import splat as OS                                        # noqa: E402

F32, F64 = torch.float32, torch.float64
FAULT_MATERIAL = 1e-3
SPLAT_SMALL = [c for c in E.SPLAT_CASES if c != E.SPLAT_LARGE]
SPLAT_FAULTS = ("drop_nw", "drop_ne", "drop_sw", "drop_se", "swap_ne_sw", "drop_border", "nonfinite_zero", "no_mask", "no_eps", "pitch_h")


def _splat_variant(x, flow, metric, mask, fault=None):
    """fp64 'soft' splat with one seeded fault: drop_* one of the four corner lists dropped; swap_ne_sw the NE and SW weights
    exchanged; drop_border sources whose north-west cell has row or column -1 dropped; nonfinite_zero a non-finite flow treated as
    zero flow; no_mask; no_eps; pitch_h the gather reading cell (qy + 1) (H + 1) + qx + 1 of bins laid out with pitch W + 1."""
    n, c, h, w = x.shape
    gy, gx = torch.meshgrid(torch.arange(h, dtype=F32), torch.arange(w, dtype=F32), indexing="ij")
    fx, fy = gx[None] + flow[:, 0], gy[None] + flow[:, 1]
    fin = torch.isfinite(fx) & torch.isfinite(fy)
    if fault == "nonfinite_zero":
        fx, fy, fin = torch.where(fin, fx, gx[None].expand_as(fx)), torch.where(fin, fy, gy[None].expand_as(fy)), torch.ones_like(fin)
    fx, fy = torch.where(fin, fx, torch.zeros_like(fx)).to(F64), torch.where(fin, fy, torch.zeros_like(fy)).to(F64)
    x0, y0 = torch.floor(fx), torch.floor(fy)
    inside = fin & (x0 >= -1) & (x0 < w) & (y0 >= -1) & (y0 < h)            # the sources the bins hold
    if fault == "drop_border":
        inside = inside & (x0 >= 0) & (y0 >= 0)
    e = torch.exp(metric.to(F64))
    planes = torch.cat([x.to(F64) * e, e], 1).reshape(n, c + 1, h * w)
    out = torch.zeros(n, c + 1, h * w, dtype=F64)
    wgt = {(0, 0): (x0 + 1 - fx) * (y0 + 1 - fy), (1, 0): (fx - x0) * (y0 + 1 - fy), (0, 1): (x0 + 1 - fx) * (fy - y0),
           (1, 1): (fx - x0) * (fy - y0)}
    if fault == "swap_ne_sw":
        wgt[(1, 0)], wgt[(0, 1)] = wgt[(0, 1)], wgt[(1, 0)]
    names = {(0, 0): "drop_nw", (1, 0): "drop_ne", (0, 1): "drop_sw", (1, 1): "drop_se"}
    for (dx, dy), wk in wgt.items():
        if fault == names[(dx, dy)]:
            continue
        if fault == "pitch_h":
            cell = (y0 + 1) * (w + 1) + x0 + 1                                  # where the bins hold the source
            targets = []
            for ty in range(h):                                                # the targets whose (wrong) list index names that cell
                tx = cell - (ty - dy + 1) * (h + 1) - 1 + dx
                targets.append((tx, torch.full_like(tx, ty)))
        else:
            targets = [(x0 + dx, y0 + dy)]
        for tx, ty in targets:
            ok = inside & (tx >= 0) & (tx < w) & (ty >= 0) & (ty < h)
            idx = torch.where(ok, ty * w + tx, torch.zeros_like(tx)).long().reshape(n, 1, h * w)
            out.scatter_add_(2, idx.expand(n, c + 1, h * w), planes * torch.where(ok, wk, torch.zeros_like(wk)).reshape(n, 1, h * w))
    out = out.reshape(n, c + 1, h, w)
    r = out[:, :c] / (out[:, c:] + (0.0 if fault == "no_eps" else L.EPS_SPLAT))
    return r if (mask is None or fault == "no_mask") else r * (1 - mask.to(F64))


def _hold_fault(name, bad, r, s, label):
    """a fault that moves the result materially must fail the check; -> whether it was material here"""
    bad = torch.nan_to_num(bad, nan=1e30, posinf=1e30, neginf=-1e30)
    if float((bad - r).abs().max()) <= FAULT_MATERIAL:
        return False
    assert not L.check(bad, r, s, F32)["ok"], (label, name)
    return True


def _splat_fault_hits(i):
    """the seeded faults that are material on small splat case i (each one held to the check on the way)"""
    case = SPLAT_SMALL[i]
    x, flow, metric, mask = E.splat_inputs(case, E.splat_seed(i))
    r, s, _ = L.splat_soft_ref(x, flow, metric, mask)
    return [f for f in SPLAT_FAULTS if not (f == "pitch_h" and case[2] == case[3])
            and _hold_fault(f, _splat_variant(x, flow, metric, mask, f), r, s, E.splat_label(case))]


@pytest.fixture(scope="module")
def splat_fault_hits():
    """{fault: [case]} over every small splat case, computed here so that the table-level test stands on its own"""
    hits = {f: [] for f in SPLAT_FAULTS}
    for i, case in enumerate(SPLAT_SMALL):
        for f in _splat_fault_hits(i):
            hits[f].append(case)
    return hits


@pytest.mark.parametrize("i", range(len(SPLAT_SMALL)), ids=[E.splat_label(c) for c in SPLAT_SMALL])
def test_splat_bound_passes_the_c_oracle_and_rejects_faults(i):
    case = SPLAT_SMALL[i]
    x, flow, metric, mask = E.splat_inputs(case, E.splat_seed(i))
    label = E.splat_label(case)
    for mk in (mask, None):
        r, s, k = L.splat_soft_ref(x, flow, metric, mk)
        assert torch.isfinite(r).all() and torch.isfinite(s).all()
        assert torch.allclose(r, _splat_variant(x, flow, metric, mk), rtol=1e-12, atol=1e-300), label     # the two fp64 forms agree
        y = OS.softsplat(x, flow, metric, "soft")
        y = y if mk is None else y * (1 - mk)
        v = L.check(y, r, s, F32)
        assert v["ok"] and v["ratio"] <= 0.5, (label, v)                      # issue: the C oracle stays at err/tol <= 0.14
    _splat_fault_hits(i)                                                      # every material fault fails the check on this case
    rs, ss, _ = L.splat_sum_ref(x, flow)
    assert L.check(OS.splat_sum(x, flow), rs, ss, F32)["ok"], label
    if case[4] == "collapse":
        assert int(k.max()) == case[2] * case[3]                              # every source of the image reaches one target


def test_splat_faults_are_exposed_by_the_table(splat_fault_hits):
    """every seeded fault is material — and therefore rejected — on the flow families that are in the table for it, and on an odd batch"""
    fam = lambda f: {c[4] for c in splat_fault_hits[f]}
    for f in ("drop_nw", "drop_ne", "drop_sw", "drop_se"):
        assert {"smooth", "collapse", "nonfinite"} <= fam(f), (f, fam(f))
    assert "border" in fam("drop_nw") and "away" in fam("drop_nw")         # weights exactly 1 on the north-west corner
    assert {"smooth", "collapse"} <= fam("swap_ne_sw")
    assert {"smooth", "nonfinite"} <= fam("drop_border")                  # (exact border landings give those corners weight 0)
    assert fam("nonfinite_zero") == {"nonfinite"}
    assert fam("no_mask") == set(E.FLOW_FAMILIES)
    assert any(c[5] == "wide" for c in splat_fault_hits["no_eps"])        # (an empty target also exposes it: 0 / 0)
    assert {c[:4] for c in splat_fault_hits["pitch_h"]} >= {(2, 5, 24, 40), (3, 7, 7, 9)}      # the non-square maps
    for f in SPLAT_FAULTS:
        assert any(c[0] == 3 for c in splat_fault_hits[f]), f                # an odd batch


OCCLUSION_FAULTS = ("drop_nw", "drop_ne", "drop_sw", "drop_se", "drop_border", "swap_ne_sw")


@pytest.mark.parametrize("case", E.OCCLUSION_CASES, ids=[f"{c[0]}x{c[1]}x{c[2]}" for c in E.OCCLUSION_CASES])
def test_occlusion_band_is_narrow_and_the_check_is_sharp(case):
    fa, fb = E.occlusion_inputs(case)
    ref = L.occlusion_mask_ref(fa, fb)
    assert float(ref["delta"].max()) <= 5e-5                                   # the margin stays four orders below the threshold
    v = L.check_occlusion_mask(CR.compute_mask(fa, fb), ref)
    pixels = case[0] * case[1] * case[2]
    assert v["ok"] and v["flips"] == 0, v                                      # the fp32 restatement disagrees nowhere outside the band
    assert v["band"] <= 0.005 and (pixels >= 200 or v["band"] == 0.0), v
    assert 0.05 <= v["ones"] <= 0.95, v
    # faults: every one of them flips a pixel outside the band on every shape of the table, and must then fail the check
    ones = torch.ones_like(fb[:, :1])
    band = (ref["norm"] - L.OCC_THRESHOLD).abs() <= ref["delta"]
    exposed = set()
    for f in OCCLUSION_FAULTS:
        d = fb.to(F64) + _splat_variant(fa, fb, ones, None, f)
        bad = (torch.sqrt((d * d).sum(1, keepdim=True)) > L.OCC_THRESHOLD).to(F32)
        if bool(((bad.to(F64) != ref["mask"]) & ~band).any()):
            assert not L.check_occlusion_mask(bad, ref)["ok"], f
            exposed.add(f)
    assert exposed == set(OCCLUSION_FAULTS), (case, sorted(exposed))
    soft = ref["mask"].to(F32) * 0.999
    assert not L.check_occlusion_mask(soft, ref)["ok"] and L.check_occlusion_mask(soft, ref)["not_binary"] > 0


def _flow_cases():
    return [(c, False) for c in E.FLOW_RESIZE_CASES] + [(c, True) for c in E.FLOW_RESIZE_CASES + E.FLOW_RESIZE_DIVIDE_ONLY]


@pytest.mark.parametrize("case,divide", _flow_cases(), ids=[("divide-" if d else "normalize-") + "x".join(map(str, c)) for c, d in _flow_cases()])
def test_flow_resize_bound_passes_torch_and_rejects_faults(case, divide):
    n, hh, ww, h, w = case
    src = E.flow_resize_input(case, 0)[:, 2:4]
    dx, dy = E.FLOW_DIVISORS if divide else ((w - 1) / 2.0, (h - 1) / 2.0)
    r, s = L.flow_resize_ref(src, h, w, dx, dy)
    t = F.interpolate(src, size=(h, w), mode="bilinear", align_corners=False)
    if not divide:
        assert torch.equal(torch.stack([t[:, 0] / dx, t[:, 1] / dy], 1), CR.resize_and_normalize_flow(src, h, w))
    y = torch.stack([t[:, 0] / dx, t[:, 1] / dy], 1)
    assert torch.allclose(r, torch.stack([F.interpolate(src.double(), size=(h, w), mode="bilinear", align_corners=False)[:, 0] / dx,
                                          F.interpolate(src.double(), size=(h, w), mode="bilinear", align_corners=False)[:, 1] / dy], 1),
                          rtol=1e-12, atol=1e-14)
    v = L.check(y, r, s, F32)
    assert v["ok"], (case, v)
    label = "x".join(map(str, case))
    if dx != dy:
        assert _hold_fault("divisors_swapped", torch.stack([t[:, 0] / dy, t[:, 1] / dx], 1).double(), r, s, label)
    ta = F.interpolate(src.double(), size=(h, w), mode="bilinear", align_corners=True)
    if (hh, ww) != (1, 1):
        assert _hold_fault("align_corners", torch.stack([ta[:, 0] / dx, ta[:, 1] / dy], 1), r, s, label)
    if hh != ww:                                                              # the source read with the other pitch
        tw = F.interpolate(src.double().reshape(n, 2, ww, hh), size=(h, w), mode="bilinear", align_corners=False)
        assert _hold_fault("pitch_h", torch.stack([tw[:, 0] / dx, tw[:, 1] / dy], 1), r, s, label) or h * w == 1


@pytest.mark.parametrize("case", E.FLOW_HW2_CASES, ids=lambda c: "x".join(map(str, c)))
def test_flow_hw2_resize_scale_ref_passes_torch_and_rejects_faults(case):
    """torch's fp32 F.interpolate(align_corners=True) followed by the multiply passes L.check against L.flow_hw2_resize_scale_ref;
    the half-pixel (align_corners=False) index rule and swapped u / v multipliers fail (on every case where they change a value:
    all but the identity resize 9x9 -> 9x9)"""
    hh, ww, th, tw = case
    flow = E.flow_hw2_input(case, 0)
    r, s = L.flow_hw2_resize_scale_ref(flow, th, tw)
    nchw = flow.permute(2, 0, 1).unsqueeze(0)

    def torch_path(align, mu, mv, dtype=torch.float32):
        t = F.interpolate(nchw.to(dtype), size=(th, tw), mode="bilinear", align_corners=align)
        t[:, 0] *= mu
        t[:, 1] *= mv
        return t[0]

    v = L.check(torch_path(True, tw / ww, th / hh), r, s, F32)
    assert v["ok"], (case, v)
    ref64 = torch_path(True, float(torch.tensor(tw / ww, dtype=F32)), float(torch.tensor(th / hh, dtype=F32)), torch.float64)
    assert float((r - ref64).abs().max()) <= 1e-4 * float(r.abs().max())     # the fp32 index rule moves a weight by a few ulp of the index
    label = "x".join(map(str, case))
    if case != (9, 9, 9, 9):
        assert _hold_fault("half_pixel", torch_path(False, tw / ww, th / hh).double(), r, s, label), case
        assert tw / ww != th / hh
        assert _hold_fault("multipliers_swapped", torch_path(True, th / hh, tw / ww).double(), r, s, label), case


@pytest.mark.parametrize("occ", [True, False], ids=["holes", "noholes"])
@pytest.mark.parametrize("i", range(len(E.FUSE_CASES)))
def test_fuse_bound_passes_torch_and_rejects_faults(i, occ):
    wf, wl, cf, cb, of, ob = E.fuse_inputs(E.FUSE_CASES[i], i)
    assert bool(((cf <= 0) & (cb <= 0)).any())
    assert cf.numel() == 1 or (float(cb.max()) == 1e4 and bool(((cf < 0) & (cb > 0)).any()))
    assert {float(v) for v in (of + ob).unique()} <= {0.0, 1.0, 2.0} and float((of + ob).max()) == 2.0
    r, s = L.fuse_warped_ref(wf, wl, cf, cb, of if occ else None, ob if occ else None)

    def restated(clamp=True, thr=1.5):                                        # extractors.py:297-310 as oracle/control_ref.py writes it
        conf = torch.cat([cf, cb], 1)
        conf = torch.clamp(conf, min=0) if clamp else conf
        wn = conf / (conf.sum(1, keepdim=True) + 1e-6)
        fused = wn[:, :1] * wf + wn[:, 1:] * wl
        return torch.where(((of + ob) > thr).expand_as(fused), 0.5 * (wf + wl), fused) if occ else fused

    v = L.check(restated(), r, s, F32)
    assert v["ok"], v
    label = f"fuse{i}"
    assert _hold_fault("no_clamp", restated(clamp=False).double(), r, s, label) or (occ and of.numel() == 1)   # one pixel: a hole
    if occ and of.numel() > 1:
        assert _hold_fault("holes_at_0.5", restated(thr=0.5).double(), r, s, label)


def test_elementwise_bounds_pass_torch_fp32():
    """silu / add / lincomb / postprocess: torch's fp32 evaluation passes, a result one part in 2^18 off fails; silu stays finite at
    its special inputs"""
    for n in E.ELEMENTWISE_CASES["silu_f32"][:3]:
        x = E.elementwise_input(n, n, E.SILU_SPECIALS)
        r, s = L.silu_f32_ref(x)
        y = F.silu(x)
        assert torch.isfinite(r).all() and torch.isfinite(y).all()
        assert L.check(y, r, s, F32)["ok"]
        assert L.check(torch.zeros_like(y).where(x < -88, y), r, s, F32)["ok"]       # a flushed reciprocal passes
        assert not L.check(y * (1 + 2.0 ** -18), r, s, F32)["ok"] or n == 1 and float(y.abs().max()) == 0
        assert not L.check(x * torch.sigmoid(1.001 * x), r, s, F32)["ok"] or n == 1
    for n in E.ELEMENTWISE_CASES["add_f32"][:3]:
        a, b = E.elementwise_input(n, 1), E.elementwise_input(n, 2)
        r, s = L.add_f32_ref(a, b)
        assert L.check(a + b, r, s, F32)["ok"] and not L.check(a + b * (1 + 2.0 ** -16), r, s, F32)["ok"]
    for n, t in E.ELEMENTWISE_CASES["lincomb"]:
        if n > 257:
            continue
        terms = [(E.LINCOMB_COEFS[j], E.elementwise_input(n, 10 + j)) for j in range(t)]
        r, s = L.lincomb_ref(terms)
        y = sum(torch.tensor(c, dtype=F32) * v for c, v in terms)
        assert L.check(y, r, s, F32)["ok"]
        bad = y - terms[-1][1] * torch.tensor(terms[-1][0], dtype=F32) * 2.0 ** -16     # the last coefficient slightly off
        assert not L.check(bad, r, s, F32)["ok"]
    n, c, h, w = 2, 3, 5, 7
    for xs in (3, 4):
        x = E.postprocess_input(n, c, h, w, xs)[..., :c]
        r, s = L.postprocess_image_ref(x)
        y = (x / 2 + 0.5).clamp(0, 1).permute(0, 3, 1, 2)
        assert L.check(y, r, s, F32)["ok"] and float(r.min()) == 0.0 and float(r.max()) == 1.0
        assert not L.check((x / 2 + 0.5).permute(0, 3, 1, 2), r, s, F32)["ok"]            # no clamp


def test_exact_references_round_once():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 3, 4, 5, generator=g)
    y = L.nchw_f32_to_nhwc_bf16_ref(x)
    assert y.shape == (2, 4, 5, 3) and torch.equal(y.permute(0, 3, 1, 2), x.to(BF))
    assert torch.equal(L.nhwc_to_nchw_f32_ref(y), x.to(BF).float())
    tok, pos = torch.randn(11, 8, generator=g).to(BF), torch.randn(7, 8, generator=g).to(BF)
    ids = torch.tensor([[0, 10, 3, 3, 9], [10, 0, 1, 2, 5]])
    e = L.embed_tokens_ref(ids, tok, pos)
    assert torch.equal(e[1, 0], (tok[10].float() + pos[0].float()).to(BF)) and e.shape == (2, 5, 8)
