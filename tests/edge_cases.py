"""Edge-case tables of the conv / linear, attention and normalisation launches, their instance keys, and guarded buffers.

Plain module (imported by tests/test_edge_coverage.py on the CPU and tests/test_gpu_edges.py on the GPU, as launch_shadow.py is):

* `Guarded`: a tensor view inside a larger allocation whose guard elements (before, after, and in the gap between rows of a
  pitched view) hold a NaN with a distinctive payload.  An output view is pre-filled with the same pattern, so an element the
  kernel never writes stays non-finite (L.check treats it as infinitely wrong); `bad()` lists every guard element that no longer
  holds the pattern, compared as integers.  A uint8 buffer holds the byte 0xA5 instead: a legitimate output value, so `unwritten()`
  means nothing for it and such an output is compared in full.  float64 (the metric outputs) holds a NaN compared as int64.
* `run_on_fills`: one launcher on a guarded workspace of exactly its dc_*_ws_bytes, under three fills of the workspace (the NaN
  pattern, zeros, what a launch on other inputs left): guards, nothing unwritten, finite, bitwise equal outputs.  The GPU test of
  every launcher that takes a caller-owned workspace goes through it (tests/test_edge_coverage.py keeps the census).
  `CONV_SCRATCH_CASES`: the conv cases whose launch is handed a scratch by ops.conv (ops._scratch); which ones: `case_plan(c).scratch`.
* `conv_key` / `attention_key`: the kernel instance a launch runs, from the dispatcher's own queries (dc_conv_route and
  dc_conv_instance, dc_attention_route).  `case_plan`: ops.conv_plan of a conv case, the descriptor and scratches of its launch.
* `conv_operands`: the seeded operands of a conv case, drawn once for tests/test_gpu_edges.py, tests/test_gpu_conv_bits.py and
  tools/record_conv_bits.py.
* `f32_conv_key`: the same as `conv_key` for the fp32 extractor conv (dc_conv3x3_f32_route).
* `SPLAT_CASES`, `OCCLUSION_CASES`, `FLOW_RESIZE_CASES`, `FUSE_CASES`, `ELEMENTWISE_CASES`: the control stage (splat, occlusion
  mask, flow resize, fusion) and the plain elementwise launchers, with the generators of their inputs.
* `SSIM_CASES`, `MS_SSIM_CASES`, `PSNR_CASES`, `METRIC_REFUSALS`: dc_ssim / dc_ms_ssim / dc_psnr at the window instances, tile,
  wave and loop edges of csrc/metrics.hip, over operand forms (two stride sets) and value families, with `metric_inputs` /
  `metric_operand`; `FDN_CASES`, `FLOW_HW2_CASES`, `PACK_CASES`, `BLEND_CASES`: the input-side and blend launchers.
* `CONV_CASES`, `ATTN_CASES`, `NORM_CASES`, `F32_CONV_CASES`: the tables.  Every conv / attention case declares the instance it
  targets; tests/test_edge_coverage.py proves that every instance the dispatcher can reach has a case and that every case routes
  where it says."""
import ctypes
import math
from dataclasses import dataclass

import torch

from diffcodec_amd import ops as _ops

GUARD = 256                                   # guard elements on each side of a view
NAN_BITS = {torch.bfloat16: 0x7FA5, torch.float32: 0x7FA5A5A5, torch.uint8: 0xA5,    # uint8 has no NaN: the byte 0xA5 stands in
            torch.float64: 0x7FFA5A5AA5A5A5A5}
_INT = {torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.uint8: torch.uint8, torch.float64: torch.int64}


# ------------------------------------------------------------------------------------------ guarded buffers
class Guarded:
    """`view` = contiguous `shape` (or rows of `pitch` elements, the last dim using the first shape[-1] of them) inside one
    allocation of GUARD + rows * pitch + GUARD elements, everything filled with the NaN pattern.  `fill(t)` copies data into the
    view (operands); outputs are left holding the pattern."""

    def __init__(self, shape, dtype, device, pitch=None, guard=GUARD):
        self.shape, self.dtype = tuple(shape), dtype
        cols = self.shape[-1]
        rows = math.prod(self.shape[:-1])
        self.pitch = cols if pitch is None else pitch
        assert self.pitch >= cols
        self.guard = guard
        n = guard + rows * self.pitch + guard
        self.base = torch.empty(n, dtype=dtype, device=device)
        self.base.view(_INT[dtype]).fill_(_signed(NAN_BITS[dtype], dtype))
        # batch stride implied by the rows (a [B, N, C] view with row pitch p has batch stride N * p)
        strides = []
        acc = self.pitch
        for d in reversed(self.shape[:-1]):
            strides.append(acc)
            acc *= d
        strides = tuple(reversed(strides)) + (1,)
        self.view = torch.as_strided(self.base, self.shape, strides, guard)
        self.mask = torch.ones(n, dtype=torch.bool, device=device)             # True: a guard element
        idx = torch.as_strided(torch.arange(n, device=device), self.shape, strides, guard)
        self.mask[idx.reshape(-1)] = False

    def fill(self, t):
        self.view.copy_(t)
        return self.view

    def bad(self):
        """-> list of (where, element index) of guard elements that no longer hold the pattern: 'before', 'after' or 'gap'."""
        bits = self.base.view(_INT[self.dtype])
        wrong = (bits != _signed(NAN_BITS[self.dtype], self.dtype)) & self.mask
        out = []
        for i in torch.nonzero(wrong).reshape(-1)[:8].tolist():
            out.append(("before" if i < self.guard else "after" if i >= self.base.numel() - self.guard else "gap", i - self.guard))
        return out

    def assert_intact(self, name):
        b = self.bad()
        assert not b, f"{name}: guard elements overwritten (where, offset from the view's first element): {b}"

    def unwritten(self):
        """number of view elements that still hold the exact pattern (an output element the kernel never wrote)"""
        return int((self.view.contiguous().view(_INT[self.dtype]) == _signed(NAN_BITS[self.dtype], self.dtype)).sum())


def _signed(bits, dtype):
    if dtype == torch.uint8:
        return bits
    w = {torch.bfloat16: 16, torch.float32: 32, torch.float64: 64}[dtype]
    return bits - (1 << w) if bits >= 1 << (w - 1) else bits


# ------------------------------------------------------------------------------------------ caller-owned workspaces
WS_FILLS = ("nan", "zeros", "stale")
_STORE = {torch.int32: torch.float32, torch.int64: torch.float64}       # integer outputs live in a guarded float buffer of their width


def ws_bits(t):
    """the bits of a tensor as integers (uint8 as it is): NaN payloads compare"""
    t = t.contiguous()
    return t if not t.dtype.is_floating_point else t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def guarded_output(shape, dtype, device):
    """-> (Guarded, view of `dtype`): an output buffer holding the NaN pattern; int32 / int64 outputs are views of a guarded
    float32 / float64 buffer (the pattern read as an integer is 2141562277 / 9221788429789668773, no count or index here)"""
    g = Guarded(tuple(shape), _STORE.get(dtype, dtype), device)
    return g, (g.view.view(dtype) if dtype in _STORE else g.view)


def run_on_fills(launch, nbytes, outputs, what, operands=(), device="cuda", elem=torch.float32, finite=True, keep=False):
    """Hold one launcher to the two promises its header makes about a caller-owned workspace: it is `nbytes` (the launcher's
    dc_*_ws_bytes) long and may hold any contents.

    launch(ws, outs, prime): ws = the workspace, a 1-d `elem` view of exactly nbytes (its address: ws.data_ptr()); outs = one fresh
    tensor per (shape, dtype) of `outputs`, each inside its own Guarded holding the NaN pattern; prime = False for the launch under
    test, True for a launch of the same shape on different input values (it only dirties the workspace; its outputs are held to the
    same guards).  operands = the Guarded buffers the closure reads.  elem = float32 (its guard pattern is a NaN, which no product
    with a zero weight hides; a uint8 workspace would hold 0xA5 bytes = -2.9e-16 as floats, finite and invisible) or float64 for
    workspaces of double partials.

    The launch under test runs three times, the workspace interior holding: 'nan' the pattern as allocated; 'zeros'; 'stale' what
    a prime launch left.  After every launch (the prime one too): every guard of the workspace, the outputs and the operands is
    intact, no output element holds the pattern (uint8 outputs excepted: 0xA5 is a value), and with finite=True every floating
    output is finite.  The three sets of outputs are bitwise equal.

    keep=True: the buffer is itself a result that a later launch reads (dc_lpips_alex_keep's maps).  Every element the 'nan' run
    wrote must then hold the same bits after the other two runs, and a copy of the buffer after the 'nan' run (the pattern still
    in what nobody wrote) is appended to the outputs returned.
    -> (the outputs of the 'nan' run, the share of workspace elements still holding the pattern after it)"""
    size = torch.empty((), dtype=elem).element_size()
    assert elem in (torch.float32, torch.float64), elem
    assert nbytes > 0, f"{what}: dc_*_ws_bytes = {nbytes}"
    assert nbytes % size == 0, f"{what}: dc_*_ws_bytes = {nbytes} is no multiple of {size}"
    ws = Guarded((nbytes // size,), elem, device)
    on_gpu = ws.view.is_cuda
    if on_gpu:                                   # the alignment the cmp, guide and loss entries demand (a host allocation has 64)
        assert ws.view.data_ptr() % 256 == 0, f"{what}: the guarded workspace is not 256-byte aligned"

    def one(tag, prime):
        held = [guarded_output(shape, dtype, device) for shape, dtype in outputs]
        launch(ws.view, [v for _, v in held], prime)
        if on_gpu:
            torch.cuda.synchronize()
        ws.assert_intact(f"{what} [{tag}] workspace of {nbytes} bytes")
        for k, g in enumerate(operands):
            g.assert_intact(f"{what} [{tag}] operand {k}")
        for k, (g, v) in enumerate(held):
            g.assert_intact(f"{what} [{tag}] output {k}")
            if g.dtype != torch.uint8:
                assert g.unwritten() == 0, f"{what} [{tag}] output {k}: {g.unwritten()} of {v.numel()} elements never written"
            if finite and v.dtype.is_floating_point:
                bad = int((~torch.isfinite(v)).sum())
                assert bad == 0, f"{what} [{tag}] output {k}: {bad} of {v.numel()} elements are not finite"
        return [v for _, v in held] + ([ws.view.clone()] if keep and not prime else [])

    got = {"nan": one("nan", False)}
    share = ws.unwritten() / ws.view.numel()
    ws.view.zero_()
    got["zeros"] = one("zeros", False)
    one("prime", True)
    got["stale"] = one("stale", False)
    written = ws_bits(got["nan"][-1]) != _signed(NAN_BITS[elem], elem) if keep else None
    for tag in WS_FILLS[1:]:
        for k, (a, b) in enumerate(zip(got["nan"], got[tag])):
            diff = ws_bits(a) != ws_bits(b)
            if keep and k == len(outputs):
                diff &= written
            diff = int(diff.sum())
            assert diff == 0, (f"{what}: output {k} under the '{tag}' fill differs from the 'nan' fill in {diff} of {a.numel()} elements: "
                               "the launch reads workspace memory it never wrote")
    return got["nan"], share


# ------------------------------------------------------------------------------------------ conv / linear instances
@dataclass(frozen=True)
class ConvCase:
    """One ops.conv launch.  ln: None | 'pairs' (finalized (mean, rstd)) | number of raw partials per row (ln_partials)."""
    key: tuple
    n: int
    h: int
    w: int
    c1: int
    cout: int
    k: int = 1
    c2: int = 0
    stride: int = 1
    pad: int = 1
    up: bool = False
    gn: bool = False
    gn_silu: bool = False
    row_add: bool = False
    residual: bool = False
    act: int = 0
    out_f32: bool = False
    out_scale: float = 1.0
    geglu: bool = False
    ln: object = None
    stats_out: bool = False
    gn_part: bool = False
    splitk: int = 1
    note: str = ""

    out_hw = property(lambda s: _ops.conv_out_hw(s.h, s.w, s.k, s.stride, s.pad, s.up))
    ho = property(lambda s: s.out_hw[0])
    wo = property(lambda s: s.out_hw[1])
    m = property(lambda s: s.n * s.ho * s.wo)
    row_add_pitch = property(lambda s: s.cout + 8)      # row_add is a pitched view: its stride is part of the descriptor

    def label(self):
        f = [n for n in ("gn", "gn_silu", "row_add", "residual", "out_f32", "geglu", "stats_out", "gn_part", "up") if getattr(self, n)]
        f += [f"act={self.act}"] if self.act else []
        f += [f"ln={self.ln}"] if self.ln is not None else []
        f += [f"out_scale={self.out_scale}"] if self.out_scale != 1.0 else []
        f += [f"splitk={self.splitk}"] if self.splitk != 1 else []
        return (f"{self.n}x{self.h}x{self.w}x({self.c1}+{self.c2})->{self.cout} k{self.k}s{self.stride}p{self.pad} "
                f"M={self.m} [{','.join(f)}]")


def case_plan(c):
    """ops.conv_plan of the launch ops.conv makes for case `c` with the operands of `conv_operands` (needs the library, not a GPU)"""
    return _ops.conv_plan(c.n, c.h, c.w, c.c1, c.c2, cout=c.cout, ksize=c.k, geglu=c.geglu, ln_folded=c.ln is not None, gn_batch=c.n * c.gn,
                          gn_silu=c.gn_silu, row_add_stride=c.row_add_pitch if c.row_add else None, residual=c.residual, stride=c.stride,
                          pad=c.pad, upsample=c.up, out_scale=c.out_scale, out_f32=c.out_f32, act=c.act, splitk=c.splitk, ln=c.ln, ln_eps=1e-5,
                          stats_out=c.stats_out, gn_part=c.gn_part)


def desc_fields(d):
    """(every non-pointer field of a dc_conv_desc by name, the names of its non-null pointer fields): what a plan and a launch share"""
    fields = type(d)._fields_
    return ({n: getattr(d, n) for n, t in fields if t is not ctypes.c_void_p}, [n for n, t in fields if t is ctypes.c_void_p and getattr(d, n)])


def conv_key(d):
    """Instance key of a dc_conv_desc: (kernel, variant, epi, split-K > 1, ln_first) from dc_conv_route, then the template arguments
    of the launched instance that those five do not imply, from dc_conv_instance:
      conv3x3_tile  GN (GroupNorm on load), TN, NSTB, FAST — and the fused upsample and the narrow map (Wo < 16), which are run-time
                    paths of the FAST = 0 instances, so they come from the descriptor;
      gemm_rowpanel GN (GroupNorm partials out);
      gemm_wide     ST (statistics outputs of the epi 1 / 2 kernels) and TN (160- or 128-column tile);
      igemm         KS3 (3x3 gather), GN (GroupNorm on load)."""
    r, t = _ops.conv_route(d), _ops.conv_instance(d)
    key = (r.kernel, r.variant, r.epi, r.splitk > 1, r.ln_first)
    if r.kernel == "conv3x3_tile":
        key += (("gn", bool(t["GN"])), ("up", bool(d.upsample)), ("narrow", d.Wo < 16), ("tn", t["TN"]), ("nst", t["NSTB"]),
                ("fast", bool(t["FAST"])))
    elif r.kernel == "gemm_rowpanel":
        key += (("gn_part", bool(t["GN"])),)
    elif r.kernel == "gemm_wide":
        key += (("st", t["ST"]), ("tn", t["TN"]))
    elif r.kernel == "igemm":
        key += (("k3", bool(t["KS3"])), ("gn", bool(t["GN"])))
    return key


def key_str(key):
    return "/".join(f"{k[0]}={int(k[1]) if isinstance(k[1], bool) else k[1]}" if isinstance(k, tuple) else str(k) for k in key)


def enumerate_conv_keys():
    """Every instance key dc_conv_route yields over a descriptor grid that spans each routing flag: 1x1 shapes in the regime of
    each GEMM kernel x every epilogue / statistics / LayerNorm / split-K option, and 3x3 shapes (tile-aligned, narrow 8x8, odd,
    strided, upsampled, Cout <= 32) x GroupNorm on load, concat, epilogue and split-K options.  -> {key: example descriptor label}"""
    keys = {}

    def add(c):
        try:
            k = conv_key(case_plan(c).desc)
        except _ops.lib.HipLaunchError:
            return
        keys.setdefault(k, c.label())

    # 1x1 / linear regimes: small M (64-row deep ring), mid M (128-row tiles), the wide / p8 grids, the row-panel K = 320 panels
    shapes11 = [(1, 1, 77, 640, 640), (1, 1, 333, 320, 1280), (1, 1, 4096, 640, 640), (1, 1, 4096, 1280, 1280),
                (1, 1, 16384, 640, 1920), (1, 1, 15104, 640, 1920), (1, 1, 8192, 1280, 1280), (1, 1, 8192, 1280, 1024), (1, 1, 8192, 1280, 5120), (1, 1, 65536, 320, 320),
                (1, 1, 65536, 320, 1280), (4, 16, 16, 1280, 1280), (16, 64, 64, 320, 320), (1, 1, 64, 64, 48)]
    for (n, h, w, cin, cout) in shapes11:
        for geglu in (False, True):
            if geglu and cout % 32:
                continue
            for ln in (None, "pairs", 4, 20):
                for res, ra, act, f32, so, gp, gn, sk in _epi_grid(geglu):
                    add(ConvCase(None, n, h, w, cin, (2 * cout if geglu else cout), geglu=geglu, ln=ln, residual=res, row_add=ra,
                                 act=act, out_f32=f32, stats_out=so, gn_part=gp, gn=gn, splitk=sk))
    # 3x3 maps: 8-row / 4-row tiles, two 8x8 images per tile, narrow 8x8, odd (gather), strided, upsampled
    shapes33 = [(2, 16, 16, 64, 64), (3, 16, 32, 320, 320), (40, 12, 32, 320, 320), (40, 12, 32, 128, 144), (40, 32, 32, 320, 320),
                (80, 32, 32, 128, 128), (1, 8, 8, 320, 320), (2, 8, 8, 128, 128), (512, 8, 8, 320, 320), (1024, 8, 8, 128, 128),
                (1, 13, 9, 64, 48), (2, 16, 16, 320, 4), (2, 8, 8, 128, 16), (2, 16, 16, 128, 16), (3, 12, 32, 128, 144)]
    for (n, h, w, cin, cout) in shapes33:
        for up in (False, True):
            for stride, pad in ((1, 1), (2, 1), (2, 0)):
                if up and stride != 1:
                    continue
                for gn, silu in ((False, False), (True, False), (True, True)):
                    for res, act, f32, sk in ((False, 0, False, 1), (True, 0, False, 1), (False, 1, False, 1), (False, 0, True, 1),
                                              (False, 0, False, 2)):
                        for c2 in (0, 64):
                            add(ConvCase(None, n, h, w, cin - c2, cout, k=3, c2=c2, stride=stride, pad=pad, up=up, gn=gn,
                                         gn_silu=silu, residual=res, act=act, out_f32=f32, splitk=sk, gn_part=True))
                            add(ConvCase(None, n, h, w, cin - c2, cout, k=3, c2=c2, stride=stride, pad=pad, up=up, gn=gn,
                                         gn_silu=silu, residual=res, act=act, out_f32=f32, splitk=sk))
    return keys


def _epi_grid(geglu):
    """(residual, row_add, act, out_f32, stats_out, gn_part, gn, splitk) options of a 1x1 launch"""
    out = []
    for res in (False, True):
        for ra in (False, True):
            for act in (0, 1):
                for f32 in (False, True):
                    for so in (False, True):
                        for gp in (False, True):
                            for gn in (False, True):
                                for sk in (1, 3):
                                    out.append((res, ra, act, f32, so, gp, gn, sk))
    return out




def _k(kernel, variant, epi, split=False, ln_first=False, **extra):
    key = (kernel, variant, epi, split, ln_first)
    if kernel == "conv3x3_tile":
        key += tuple((n, extra[n]) for n in ("gn", "up", "narrow", "tn", "nst", "fast"))
    elif kernel == "gemm_rowpanel":
        key += (("gn_part", extra.get("gn_part", False)),)
    elif kernel == "gemm_wide":
        key += (("st", extra.get("st", 0)), ("tn", extra.get("tn", 5)))
    elif kernel == "igemm":
        key += (("k3", extra.get("k3", False)), ("gn", extra.get("gn", False)))
    return key


# Epilogue flag sets of the 1x1 family and the specialised epilogue mode each one declares (epi_mode in gemm_dma.hip: 1 plain,
# 2 residual, 3 folded LayerNorm, 4 GEGLU, 5 GEGLU + LayerNorm, 0 the generic run-time flags); 'lf' = the LayerNorm finalize runs
# first (raw partials on a kernel whose waves do not own whole rows), 'sk' = split-K.
_PLAIN = [(dict(), 1, {}), (dict(residual=True, out_scale=0.5), 2, {}), (dict(ln="pairs"), 3, {}), (dict(ln=4), 3, dict(lf=1)),
          (dict(out_f32=True, out_scale=0.25), 0, {}), (dict(row_add=True, act=1), 0, {}), (dict(act=2, residual=True), 0, {}),
          (dict(stats_out=True, ln=4), 0, dict(lf=1)), (dict(splitk=3), 0, dict(sk=1))]
_GEGLU = [(dict(geglu=True), 4, {}), (dict(geglu=True, ln="pairs"), 5, {}), (dict(geglu=True, ln=4), 5, dict(lf=1)),
          (dict(geglu=True, act=1), 0, {}), (dict(geglu=True, act=1, ln=20), 0, dict(lf=1))]


def _family(kernel, variant, shape, sets, skip=(), **extra):
    n, h, w, cin, cout = shape
    out = []
    for i, (flags, epi, o) in enumerate(sets):
        if i in skip:
            continue
        c_out = 2 * cout if flags.get("geglu") else cout
        out.append(ConvCase(_k(kernel, variant, epi, bool(o.get("sk")), bool(o.get("lf")), **extra), n, h, w, cin, c_out, **flags))
    return out


def _tile(variant, shape, tn, ring=2, fast=True, gn_tpl=None, split_ring=None, narrow=False, gn_opts=(False, True), up=False,
          splits=True, c2=0, **kw):
    """conv3x3_tile cases of one map shape: the plain / residual / generic epilogues, with and without GroupNorm on load, split-K.
    Declared template: (tn, ring, fast) without GroupNorm, gn_tpl (default the same) with it; split_ring = the ring of the split-K
    launch when its larger grid changes it."""
    n, h, w, cin, cout = shape
    out = []
    for gn in gn_opts:
        t_tn, t_ring, t_fast = (gn_tpl or (tn, ring, fast)) if gn else (tn, ring, fast)
        ex = dict(gn=gn, up=up, narrow=narrow, tn=t_tn, nst=t_ring, fast=t_fast)
        base = dict(k=3, up=up, gn=gn, gn_silu=gn, c2=c2, **kw)
        out.append(ConvCase(_k("conv3x3_tile", variant, 1, **ex), n, h, w, cin - c2, cout, gn_part=True, **base))
        out.append(ConvCase(_k("conv3x3_tile", variant, 2, **ex), n, h, w, cin - c2, cout, residual=True, **base))
        out.append(ConvCase(_k("conv3x3_tile", variant, 0, **ex), n, h, w, cin - c2, cout, act=1, out_scale=0.5, **base))
        if splits:
            exs = dict(ex, nst=split_ring if (split_ring is not None and t_fast and not up and not narrow) else t_ring)
            out.append(ConvCase(_k("conv3x3_tile", variant, 0, True, **exs), n, h, w, cin - c2, cout, splitk=2, **base))
    return out


CONV_CASES = (
    # ---------------------------------------------------------------- gemm_dma: the LDS-DMA GEMM's four production tiles
    # 64-row tiles, 2 stages (K = 320: too short for the deep ring), Cout 1280 = 8 x 160; M = 333: 5 full + 1 ragged row tile
    _family("gemm_dma", 25201, (1, 1, 333, 320, 1280), _PLAIN)
    # 64-row tiles, deep 4-stage ring (K = 640, one workgroup per CU): M = 77 (the text context), 4 x 160 columns
    + _family("gemm_dma", 25401, (1, 1, 77, 640, 640), _PLAIN)
    # 128-row tiles: M = 4099 (ragged last tile), N = 1280
    + _family("gemm_dma", 45201, (1, 1, 4099, 1280, 1280), _PLAIN)
    # 64-row 128-column tile (Cout not a multiple of 160): Cout = 48 (one ragged N tile), K = 64 (a single K step), M = 65
    + _family("gemm_dma", 24301, (1, 1, 65, 64, 48), _PLAIN, skip=(8,))
    + _family("gemm_dma", 24301, (1, 1, 333, 320, 1280), _GEGLU)
    + _family("gemm_dma", 24501, (1, 1, 77, 640, 640), _GEGLU)
    + _family("gemm_dma", 44201, (1, 1, 4097, 640, 640), _GEGLU)
    + [ConvCase(_k("gemm_dma", 45201, 0, True), 3, 1, 1365, 640, 640, splitk=7, note="split 7 over 10 K steps -> fixpoint 5"),
       ConvCase(_k("gemm_dma", 24301, 1), 1, 1, 65, 64, 144, note="Cout = 144: one full and one ragged 128-column tile"),
       ConvCase(_k("gemm_dma", 25401, 1), 1, 1, 77, 320, 640, c2=320, note="x2 concat"),
       ConvCase(_k("gemm_dma", 45201, 1), 3, 1, 1367, 640, 1280, c2=640, note="x2 concat, odd N")]
    # ---------------------------------------------------------------- gemm_wide: 256-row tiles, K in [640, 2560], >= 192 tiles
    + [ConvCase(_k("gemm_wide", 0, 1, st=s), 1, 1, 16384, 640, 1920, stats_out=bool(s & 1), gn_part=bool(s & 2)) for s in (1, 3)]
    + [ConvCase(_k("gemm_wide", 0, 1, st=2), 64, 16, 16, 640, 1920, gn_part=True)]
    + [ConvCase(_k("gemm_wide", 0, 2, st=s), 64, 16, 16, 640, 1920, residual=True, stats_out=bool(s & 1), gn_part=bool(s & 2))
       for s in (0, 1, 2, 3)]
    + [ConvCase(_k("gemm_wide", 0, 1, tn=4), 1, 1, 8192, 1280, 1024, note="128-column tiles"),
       ConvCase(_k("gemm_wide", 0, 2, tn=4), 1, 1, 8192, 1280, 1024, residual=True),
       ConvCase(_k("gemm_wide", 0, 3, tn=4), 1, 1, 8192, 1280, 1024, ln="pairs"),
       ConvCase(_k("gemm_wide", 0, 3, ln_first=True, tn=4), 1, 1, 8192, 1280, 1024, ln=4),
       ConvCase(_k("gemm_dma", 44201, 0, True), 1, 1, 8193, 1280, 1024, splitk=3),
       ConvCase(_k("igemm", 44, 0, True, gn=True), 1, 1, 8193, 1280, 1024, gn=True, splitk=3)]
    + [ConvCase(_k("gemm_wide", 0, e, st=st, tn=4), 32, 16, 16, 1280, 1024, residual=e == 2, stats_out=bool(st & 1),
                gn_part=bool(st & 2)) for e in (1, 2) for st in (1, 2, 3)]
    + [ConvCase(_k("gemm_wide", 0, 1), 1, 1, 8192, 1280, 1280, note="too few tiles for the 256 x 256 kernel"),
       ConvCase(_k("gemm_wide", 0, 3), 1, 1, 8192, 1280, 1280, ln="pairs"),
       ConvCase(_k("gemm_wide", 0, 3, ln_first=True), 1, 1, 8192, 1280, 1280, ln=4)]
    + [ConvCase(_k("gemm_wide", 0, 4, tn=4), 1, 1, 4096, 1280, 2 * 1280, geglu=True),
       ConvCase(_k("gemm_wide", 0, 5, tn=4), 1, 1, 4096, 1280, 2 * 1280, geglu=True, ln="pairs"),
       ConvCase(_k("gemm_wide", 0, 5, ln_first=True, tn=4), 1, 1, 4096, 1280, 2 * 1280, geglu=True, ln=20)]
    # ---------------------------------------------------------------- gemm_p8: 256 x 256 tiles; 15104 = 59 row tiles (not a
    # multiple of gm = 8) with a half-full last column tile (1920 = 7.5 x 256)
    + [ConvCase(_k("gemm_p8", 0, 1), 1, 1, 15104, 640, 1920, note="round-4 advice shape"),
       ConvCase(_k("gemm_p8", 0, 3), 1, 1, 15104, 640, 1920, ln="pairs"),
       ConvCase(_k("gemm_p8", 0, 3, ln_first=True), 1, 1, 15104, 640, 1920, ln=20),
       ConvCase(_k("gemm_p8", 0, 4), 1, 1, 15104, 640, 2 * 1920, geglu=True),
       ConvCase(_k("gemm_p8", 0, 5), 1, 1, 15104, 640, 2 * 1920, geglu=True, ln="pairs"),
       ConvCase(_k("gemm_p8", 0, 5, ln_first=True), 1, 1, 15104, 640, 2 * 1920, geglu=True, ln=4)]
    # ---------------------------------------------------------------- gemm_rowpanel: K = 320, M >= 65536, 256-row panels
    + [ConvCase(_k("gemm_rowpanel", 0, 1), 1, 1, 65536, 320, 320),
       ConvCase(_k("gemm_rowpanel", 0, 1, gn_part=True), 16, 64, 64 + 4, 320, 320, gn_part=True, note="M = 65536 + 256 x 17"),
       ConvCase(_k("gemm_rowpanel", 0, 1), 16, 64, 64, 320, 320, gn=True, note="GroupNorm affine on load"),
       ConvCase(_k("gemm_rowpanel", 0, 2), 1, 1, 65536 + 256, 320, 640, residual=True, out_scale=0.5),
       ConvCase(_k("gemm_rowpanel", 0, 2, gn_part=True), 16, 64, 64, 320, 320, residual=True, gn_part=True),
       ConvCase(_k("gemm_rowpanel", 0, 3), 1, 1, 65536, 320, 320, ln="pairs"),
       ConvCase(_k("gemm_rowpanel", 0, 3), 1, 1, 65536 + 256, 320, 320, ln=16, note="raw partials = DC_LN_PARTS_MAX"),
       ConvCase(_k("gemm_rowpanel", 0, 3, ln_first=True), 1, 1, 65536, 320, 320, ln=20, note="raw partials > DC_LN_PARTS_MAX"),
       ConvCase(_k("gemm_rowpanel", 0, 4), 1, 1, 65536, 320, 2 * 640, geglu=True),
       ConvCase(_k("gemm_rowpanel", 0, 5), 1, 1, 65536 + 256, 320, 2 * 640, geglu=True, ln=4),
       ConvCase(_k("gemm_rowpanel", 0, 5, ln_first=True), 1, 1, 65536, 320, 2 * 640, geglu=True, ln=20)]
    # ---------------------------------------------------------------- igemm: the gather GEMM (strided / odd 3x3 maps, GN on load)
    + [ConvCase(_k("igemm", 24, 0, k3=True), 3, 13, 9, 64, 48, k=3, note="odd map, Cout 48"),
       ConvCase(_k("igemm", 24, 0, k3=True), 3, 15, 17, 128, 144, k=3, stride=2, pad=1, note="stride 2, pad 1, odd map"),
       ConvCase(_k("igemm", 24, 0, k3=True), 1, 15, 17, 64, 64, k=3, stride=2, pad=0, note="stride 2, pad 0 (F.pad right / bottom)"),
       ConvCase(_k("igemm", 24, 0, k3=True), 2, 7, 5, 64, 128, k=3, up=True, note="upsample of an odd map"),
       ConvCase(_k("igemm", 24, 0, k3=True), 2, 13, 9, 64, 48, k=3, c2=128, residual=True, note="x2 concat C1 != C2"),
       ConvCase(_k("igemm", 24, 0, k3=True, gn=True), 3, 13, 9, 128, 48, k=3, gn=True, gn_silu=True, act=2),
       ConvCase(_k("igemm", 24, 0, True, k3=True), 1, 13, 9, 1280, 128, k=3, splitk=7, note="KT = 180, split 7 -> 7"),
       ConvCase(_k("igemm", 24, 0, True, k3=True), 1, 13, 9, 1280, 128, k=3, splitk=19, note="KT = 180, split 19 -> 18"),
       ConvCase(_k("igemm", 24, 0, True, k3=True, gn=True), 2, 13, 9, 320, 48, k=3, gn=True, splitk=4, out_f32=True),
       ConvCase(_k("igemm", 25, 0, k3=True), 16, 32, 32, 320, 320, k=3, stride=2, pad=1),
       ConvCase(_k("igemm", 25, 0, k3=True, gn=True), 16, 32, 32, 320, 320, k=3, stride=2, pad=0, gn=True),
       ConvCase(_k("igemm", 25, 0, True, k3=True), 16, 32, 32, 320, 320, k=3, stride=2, splitk=2),
       ConvCase(_k("igemm", 25, 0, True, k3=True, gn=True), 16, 32, 32, 320, 320, k=3, stride=2, gn=True, splitk=2),
       ConvCase(_k("igemm", 24, 0, gn=True), 1, 1, 77, 640, 2 * 640, geglu=True, gn=True),
       ConvCase(_k("igemm", 25, 0, gn=True), 1, 1, 77, 640, 640, gn=True, gn_silu=True, row_add=True),
       ConvCase(_k("igemm", 25, 0, True, gn=True), 1, 1, 77, 640, 640, gn=True, splitk=3),
       ConvCase(_k("igemm", 44, 0, gn=True), 1, 1, 4096, 1280, 2 * 1280, geglu=True, gn=True),
       ConvCase(_k("igemm", 45, 0, gn=True), 1, 1, 16384, 640, 1920, gn=True, residual=True),
       ConvCase(_k("igemm", 45, 0, True, gn=True), 1, 1, 4097, 1280, 1280, gn=True, splitk=3)]
    # ---------------------------------------------------------------- conv3x3_tile: the halo-tile kernel
    + _tile(2, (3, 12, 32, 128, 144), 4, ring=4)                         # 4-row tiles, Cout 144: ragged 128-column tile, odd N
    + _tile(2, (3, 16, 32, 320, 320), 5, ring=4)                         # 160-column tiles, deep ring (<= 256 workgroups)
    + _tile(2, (41, 12, 32, 320, 320), 5, ring=2)                        # 160-column tiles, > 256 workgroups, odd N
    + _tile(2, (41, 12, 32, 128, 144), 4, ring=2)
    + _tile(2, (1, 8, 8, 320, 320), 5, narrow=True, gn_tpl=(5, 3, False))   # narrow 8x8 map, one image
    + _tile(2, (3, 16, 8, 128, 48), 4, narrow=True, gn_tpl=(4, 3, False))   # narrow 16 x 8 map
    + _tile(2, (2, 8, 8, 128, 16), 4, narrow=True, gn_tpl=(1, 3, False))   # (the narrow and upsample forms keep 128-column tiles)
    + _tile(2, (3, 4, 16, 128, 16), 1)
    + _tile(2, (3, 4, 16, 320, 4), 1, ring=3, fast=False, splits=False)
    + _tile(2, (2, 4, 8, 128, 64), 4, up=True, gn_tpl=(4, 3, False))     # upsample 4x8 -> 8x16
    + _tile(2, (2, 4, 8, 320, 320), 5, up=True, gn_tpl=(5, 3, False))
    + _tile(2, (2, 4, 8, 128, 16), 4, up=True, gn_tpl=(1, 3, False))
    + _tile(2, (3, 2, 8, 320, 4), 1, ring=3, fast=False, up=True, splits=False)
    + _tile(4, (22, 32, 48, 128, 144), 4, c2=64)                         # 8-row tiles, x2 concat, ragged N tile
    + _tile(4, (22, 32, 48, 320, 320), 5)                                # 8-row tiles, 160-column tiles
    + _tile(4, (22, 16, 24, 128, 144), 4, up=True, gn_tpl=(4, 3, False))  # 8-row tiles with the fused upsample
    + _tile(4, (22, 16, 24, 320, 320), 5, up=True, gn_tpl=(5, 2, False))
    + _tile(8, (1026, 8, 8, 128, 128), 4, narrow=True, gn_opts=(False,))  # two 8x8 images per tile, 128-column tiles
    + _tile(8, (514, 8, 8, 128, 320), 5, narrow=True, gn_opts=(False,))   # two 8x8 images per tile
)


def conv_operands(ops, c, i, device="cuda"):
    """(packed weights, {name: guarded operand}, guarded x1, keyword arguments of ops.conv) of case i of CONV_CASES (seed 1000 + i):
    the one draw shared by tests/test_gpu_edges.py, tests/test_gpu_conv_bits.py and tools/record_conv_bits.py"""
    BF, F32 = torch.bfloat16, torch.float32

    def _g(shape, dtype, data, pitch=None):
        g = Guarded(shape, dtype, device, pitch=pitch)
        g.fill(data)
        return g

    gen = torch.Generator().manual_seed(1000 + i)
    cin = c.c1 + c.c2
    ho, wo, m = c.ho, c.wo, c.m
    w = torch.randn(c.cout, cin, c.k, c.k, generator=gen) / math.sqrt(cin * c.k * c.k)
    b = torch.randn(c.cout, generator=gen) * 0.1
    ln = None
    if c.ln is not None:
        ln = (1 + 0.1 * torch.randn(cin, generator=gen), 0.1 * torch.randn(cin, generator=gen), 1e-5)
    pc = ops.PackedConv(w, b, device, geglu=c.geglu, ln=ln, mfma_small_cout=c.cout < 16)
    gw, gb = _g(tuple(pc.w.shape), BF, pc.w), _g(tuple(pc.bias.shape), F32, pc.bias)
    pc.w, pc.bias = gw.view, gb.view
    guards = {"w": gw, "bias": gb}
    x1 = guards.setdefault("x1", _g((c.n, c.h, c.w, c.c1), BF, (torch.randn(c.n, c.h, c.w, c.c1, generator=gen) + 0.3).to(device)))
    kw = dict(stride=c.stride, pad=c.pad, upsample=c.up, out_scale=c.out_scale, out_f32=c.out_f32, splitk=c.splitk, act=c.act,
              gn_part=c.gn_part)
    if c.c2:
        kw["x2"] = guards.setdefault("x2", _g((c.n, c.h, c.w, c.c2), BF, torch.randn(c.n, c.h, c.w, c.c2, generator=gen).to(device))).view
    if c.gn:
        ab = torch.stack([1 + 0.2 * torch.randn(c.n, cin, generator=gen), 0.2 * torch.randn(c.n, cin, generator=gen)], 2)
        kw["gn_ab"] = guards.setdefault("gn_ab", _g((c.n, cin, 2), F32, ab.to(device))).view
        kw["gn_silu"] = c.gn_silu
    if c.row_add:
        kw["row_add"] = guards.setdefault("row_add", _g((c.n, c.cout), F32, torch.randn(c.n, c.cout, generator=gen).to(device),
                                                          pitch=c.row_add_pitch)).view
    if c.residual:
        kw["residual"] = guards.setdefault("residual", _g((c.n, ho, wo, c.cout), BF,
                                                          torch.randn(c.n, ho, wo, c.cout, generator=gen).to(device))).view
    xr = x1.view.reshape(-1, c.c1).to(torch.float64)
    if c.ln == "pairs":
        mean = xr.mean(1)
        rstd = 1.0 / torch.sqrt(xr.var(1, unbiased=False) + 1e-5)
        kw["ln_stats"] = guards.setdefault("ln_stats", _g((m, 2), F32, torch.stack([mean, rstd], 1).float())).view
    elif c.ln is not None:
        parts = c.ln
        bounds = [(p * cin) // parts for p in range(parts + 1)]
        pr = torch.stack([torch.stack([xr[:, lo:hi].sum(1), (xr[:, lo:hi] ** 2).sum(1)], 1) for lo, hi in zip(bounds, bounds[1:])], 1)
        kw["ln_partials"] = (guards.setdefault("ln_partials", _g((m, parts, 2), F32, pr.float())).view, 1e-5)
    return pc, guards, x1, kw


# the cases whose launch is handed a scratch by ops.conv, selected without the library from what each case declares: split-K,
# LayerNorm finalize first (key[3], key[4]), GroupNorm partials asked for.  tests/test_edge_coverage.py holds the selection to the plans.
CONV_SCRATCH_CASES = [i for i, c in enumerate(CONV_CASES) if c.key[3] or c.key[4] or c.gn_part]


# ------------------------------------------------------------------------------------------ attention instances
HEAD_DIMS = (8, 16, 32, 40, 64, 80, 128, 160)


def attention_key(b, heads, nq, nk, d):
    """(D, QB, SHORT, RAGGED, PP) of the attn_kernel instance dc_attention_bf16 launches (dc_attention_route)"""
    return tuple(int(v) for v in _ops.attention_route(b, heads, nq, nk, d))


def enumerate_attention_keys():
    """Every instance dc_attention_route yields over a grid of B x heads (grids below, at and far above the form thresholds),
    query counts and key counts (1 .. 4096: single key, one tile +- 1, the short-context limit, ragged and whole long tiles)."""
    keys = {}
    for d in HEAD_DIMS:
        for bh in ((1, 1), (2, 5), (9, 7), (8, 8), (16, 8), (32, 8), (64, 8)):
            for nq in (1, 100, 1000, 2304, 4100, 8192):
                for nk in (1, 63, 64, 65, 77, 128, 129, 192, 255, 256, 1000, 4096):
                    keys.setdefault(attention_key(*bh, nq, nk, d), (*bh, nq, nk, d))
    return keys


@dataclass(frozen=True)
class AttnCase:
    key: tuple
    b: int
    heads: int
    nq: int
    nk: int
    note: str = ""

    @property
    def d(self):
        return self.key[0]

    def label(self):
        return f"B={self.b} heads={self.heads} Nq={self.nq} Nk={self.nk} d={self.d}"


def _attn_cases():
    out = []
    for d in HEAD_DIMS:
        small = d <= 48
        # long form, one query block per wave (small grids): whole and ragged key tiles, Nk in {1, 63, 65, 64}
        out += [AttnCase((d, 1, 0, 0, 0), 2, 5, 333, 192), AttnCase((d, 1, 0, 1, 0), 2, 5, 333, 1000),
                AttnCase((d, 1, 0, 1, 0), 1, 3, 130, 1), AttnCase((d, 1, 0, 1, 0), 1, 3, 130, 63),
                AttnCase((d, 1, 0, 1, 0), 1, 3, 97, 65), AttnCase((d, 1, 0, 0, 0), 1, 3, 97, 64)]
        # short context (keys resident, 4 query blocks per workgroup): B x heads x ceil(Nq / 128) / 4 >= 512, one-half and
        # two-half last tiles (77, 96, 97, 128)
        out += [AttnCase((d, 1, 1, 1, 0), 9, 7, 4100, nk) for nk in (77, 97)]
        out += [AttnCase((d, 1, 1, 1, 0), 16, 8, 2050, nk) for nk in (96, 128)]
        if small:
            # two query blocks per wave: grids of >= 512 workgroups of 256 queries (Nq = 2300: a ragged last block); short contexts with too few workgroups for
            # the short form (Nk = 1, 63, 65) and long contexts below the ping-pong threshold (Nk < 256)
            out += [AttnCase((d, 2, 0, 1, 0), 9, 7, 2300, nk) for nk in (1, 63, 65)]
            out += [AttnCase((d, 2, 0, 0, 0), 9, 7, 2300, 64), AttnCase((d, 2, 0, 0, 0), 9, 7, 2300, 192),
                    AttnCase((d, 2, 0, 1, 0), 9, 7, 2300, 200)]
            # ping-pong (8 waves, 512 queries per workgroup): >= 256 workgroups and Nk >= 256
            out += [AttnCase((d, 2, 0, 0, 1), 9, 7, 2100, 256), AttnCase((d, 2, 0, 1, 1), 9, 7, 2100, 1000),
                    AttnCase((d, 2, 0, 1, 1), 5, 8, 3333, 300)]
    return out


ATTN_CASES = _attn_cases()


def attention_query_span(key):
    """queries per workgroup of an instance: 128 (4 waves) or 256 (8 waves, ping-pong) x QB, x 4 passes in the short form"""
    d, qb, short, ragged, pp = key
    return (256 if pp else 128) * qb * (4 if short else 1)


def attention_inputs(family, b, heads, nq, nk, d, gen):
    """fp32 (q, k, v) of an attention input family:
      random  q, k, v ~ N(0, 1);
      flat    q = 0: every real key gets the same weight and the output is the mean of V = 1 + 0.25 N(0, 1), so a masking or
              normalisation error shifts the whole row;
      peaked  the queries of head h share one direction u_h (plus 0.1 noise); the winner key of head h is c_w u_h, the others
              0.5 N(0, 1): the winner leads by a c_w scale = 25 after the softmax scale, |score| stays below ~30 (the bf16
              rounding of the prescaled queries cannot reorder keys).  Winner: first tile for heads h % 3 == 0, key Nk - 1 for head 1,
              inside the last (ragged) tile for the others — the running max, the rescale across tiles and the last-tile mask."""
    c = heads * d
    if family == "random":
        return torch.randn(b, nq, c, generator=gen), torch.randn(b, nk, c, generator=gen), torch.randn(b, nk, c, generator=gen)
    if family == "flat":
        return torch.zeros(b, nq, c), torch.randn(b, nk, c, generator=gen), 1 + 0.25 * torch.randn(b, nk, c, generator=gen)
    assert family == "peaked", family
    u = torch.randn(heads, d, generator=gen)
    u = u / u.norm(dim=1, keepdim=True)
    a = 8.0
    cw = 25.0 * math.sqrt(d) / a
    q = (a * u[None, None] + 0.1 * torch.randn(b, nq, heads, d, generator=gen)).reshape(b, nq, c)
    k = 0.5 * torch.randn(b, nk, heads, d, generator=gen)
    for h, j in enumerate(peaked_winners(heads, nk)):
        k[:, j, h] = cw * u[h]
    return q, k.reshape(b, nk, c), torch.randn(b, nk, c, generator=gen)


def peaked_winners(heads, nk):
    """key index of each head's winner in the peaked family"""
    last0 = (nk - 1) // 64 * 64
    return [min(3, nk - 1) if h % 3 == 0 else nk - 1 if h == 1 else last0 + (h * 7) % (nk - last0) for h in range(heads)]


# ------------------------------------------------------------------------------------------ normalisation cases
# group_norm_ab / gn_apply: (N, H, W, C1, C2, groups): HW not a multiple of the statistics chunking (15 x 8, 7 x 9, 1), N in {1, 3},
# a group straddling the x1 / x2 boundary (320 + 640 channels: 30 per group, group 10 = channels 300..329)
GN_CASES = [(1, 15, 8, 320, 0, 32), (3, 7, 9, 64, 0, 32), (1, 1, 1, 64, 0, 32), (3, 15, 8, 320, 640, 32), (1, 7, 9, 320, 640, 32),
            (3, 33, 17, 128, 0, 32)]
LN_CASES = [(77, c) for c in (8, 512, 520, 768, 1024, 1032, 2048)] + [(4097, 320)]          # (M, C): M % 4 != 0
ROW_STATS_CASES = [(77, 64), (77, 320), (333, 1280), (5, 2048)]
LN_FINALIZE_CASES = [(77, 1, 320), (77, 4, 640), (333, 16, 1280), (5, 20, 1280)]              # (M, parts, C)
SOFTMAX_CASES = [(5, c) for c in (1, 77, 255, 257, 4097)]                                      # (rows, cols)


# ------------------------------------------------------------------------------------------ direct (VALU) convs
@dataclass(frozen=True)
class SmallCase:
    """dc_conv_small_cin_bf16 (Cin <= 16: conv_in4_kernel for Cin = 4, 3x3 s1 p1, Cout % 8 == 0, W % 4 == 0 — 4-pixel strips —
    the generic per-pixel kernel otherwise) and dc_conv_small_cout_bf16 (COUT = 3 / 4 / 8 templates, 4 pixels per workgroup,
    GroupNorm (+ SiLU) on load, fp32 output)."""
    kind: str
    n: int
    h: int
    w: int
    cin: int
    cout: int
    k: int = 3
    stride: int = 1
    pad: int = 1
    gn: bool = False
    out_f32: bool = False

    out_hw = property(lambda s: _ops.conv_out_hw(s.h, s.w, s.k, s.stride, s.pad, False))
    ho = property(lambda s: s.out_hw[0])
    wo = property(lambda s: s.out_hw[1])

    @property
    def strip_kernel(self):
        return self.kind == "small_cin" and self.cin == 4 and self.k == 3 and self.stride == 1 and self.pad == 1 and \
            self.cout % 8 == 0 and self.w % 4 == 0

    def label(self):
        f = ["gn"] * self.gn + ["out_f32"] * self.out_f32
        return f"{self.kind} {self.n}x{self.h}x{self.w}x{self.cin}->{self.cout} k{self.k}s{self.stride}p{self.pad} [{','.join(f)}]"


SMALL_CASES = [
    SmallCase("small_cin", 2, 9, 32, 4, 320),                   # conv_in: 4-pixel strips, W % 4 == 0, odd H
    SmallCase("small_cin", 3, 7, 30, 4, 320),                   # W % 4 != 0: the per-pixel kernel
    SmallCase("small_cin", 1, 7, 13, 4, 20),                    # Cout % 8 != 0
    SmallCase("small_cin", 2, 15, 17, 4, 32, stride=2),         # stride 2 on an odd map
    SmallCase("small_cin", 1, 9, 11, 16, 24, k=1),              # 1x1, Cin 16
    SmallCase("small_cin", 2, 8, 12, 3, 16, stride=2, pad=1),   # Cin 3
] + [SmallCase("small_cout", n, 7, 9, 64, co, k=k, gn=gn, out_f32=f32)  # M = 63 or 189: a partial last 4-pixel workgroup
     for co in (3, 4, 8) for (n, k, gn, f32) in ((1, 3, False, False), (3, 3, True, False), (1, 1, False, True), (3, 3, True, True))]


# ------------------------------------------------------------------------------------------ fp32 extractor conv instances
@dataclass(frozen=True)
class F32ConvCase:
    """One dc_conv3x3_nchw_f32 launch (fp32 NCHW, 3x3, padding 1).  key = ("f32conv", form, STRIDE, output channels per workgroup,
    output pixels per workgroup): the instance it targets (f32_conv_key)."""
    key: tuple
    n: int
    cin: int
    h: int
    w: int
    cout: int
    stride: int
    note: str = ""

    @property
    def ho(self):
        return (self.h + 2 - 3) // self.stride + 1

    @property
    def wo(self):
        return (self.w + 2 - 3) // self.stride + 1

    @property
    def m(self):
        return self.n * self.ho * self.wo

    @property
    def last_row_read(self):
        """the last output row's taps reach input row H - 1 (not so at stride 4 with H = 0 or 3 mod 4)"""
        return (self.ho - 1) * self.stride + 1 >= self.h - 1

    def label(self):
        return f"{self.n}x{self.cin}x{self.h}x{self.w}->{self.cout} s{self.stride}"


def f32_conv_route(cin, h, w, cout, stride):
    return _ops.conv3x3_f32_route(cin, h, w, cout, stride)


def f32_conv_key(cin, h, w, cout, stride):
    """Instance key of one dc_conv3x3_nchw_f32 launch, from the launcher's own query (dc_conv3x3_f32_route)"""
    r = f32_conv_route(cin, h, w, cout, stride)
    return ("f32conv", r.form, r.stride, r.co_tile, r.pixel_tile)


def _f32(form, stride, co=None, pt=256):
    return ("f32conv", form, stride, co if co is not None else {"blk": 64, "direct": 16}[form], pt)


def _f32_cases(key, shapes, notes=()):
    """cases of one instance: N = 2, and N = 3 (an odd batch) for the first"""
    return [F32ConvCase(key, 3 if i == 0 else 2, *s, note=notes[i] if i < len(notes) else "") for i, s in enumerate(shapes)]


# (Cin, H, W, Cout, stride) per instance
F32_CONV_CASES = (
    # ---------------------------------------------------------------- conv3x3_f32_mfma_kernel<STRIDE, CO_T, PT>
    _f32_cases(_f32("mfma", 1, 64, 64), [(16, 8, 8, 64, 1), (24, 4, 16, 128, 1), (16, 64, 1, 64, 1)],
               ["8x8 map, 2 chunks", "4x16 map, 3 chunks, 2 channel tiles", "64x1 map: one-column tile"])
    + _f32_cases(_f32("mfma", 2, 64, 64), [(16, 16, 16, 64, 2), (24, 8, 32, 64, 2)], ["output 8x8", "output 4x16"])
    + _f32_cases(_f32("mfma", 1, 64, 128), [(16, 2, 256, 64, 1), (24, 16, 8, 64, 1), (16, 6, 64, 128, 1), (40, 128, 1, 64, 1),
                                            (16, 2, 256, 128, 1)],
                 ["cols_t 128, 2 tiles across x 2 down", "8 x 16 tile", "3 tile rows x 2 channel tiles", "one-column tile, 5 chunks",
                  "2 x 2 pixel tiles x 2 channel tiles"])
    + _f32_cases(_f32("mfma", 2, 64, 128), [(16, 4, 512, 64, 2), (24, 32, 16, 64, 2), (16, 256, 2, 64, 2), (16, 24, 128, 64, 2)],
                 ["widest patch 3 x 257", "cols_t 8", "tallest patch 257 x 3 (one-column tile)", "cols_t 64"])
    + _f32_cases(_f32("mfma", 1, 32, 128), [(16, 2, 256, 32, 1), (24, 12, 32, 96, 1)], ["1 channel tile", "3 channel tiles, 3 tile rows"])
    + _f32_cases(_f32("mfma", 2, 32, 128), [(16, 4, 512, 32, 2), (24, 24, 64, 96, 2)])
    # ---------------------------------------------------------------- conv3x3_nchw_f32_blk_kernel<STRIDE, 16, 4, 4, 8>
    + _f32_cases(_f32("blk", 1), [(3, 17, 66, 64, 1), (9, 5, 64, 80, 1), (17, 3, 35, 160, 1), (8, 16, 64, 64, 1),
                                  (4, 3, 67, 70, 1)],
                 ["Wo % 4 != 0: scalar-store arm, Cin 3", "ragged 16-channel group, Cin 9", "32-wide / 160-channel entry rule, Cin 17",
                  "exact tiles, vector stores", "Cout % 16 != 0: six channels in the second tile"])
    + _f32_cases(_f32("blk", 2), [(5, 9, 131, 65, 2), (8, 7, 66, 160, 2), (16, 33, 128, 64, 2), (16, 7, 130, 64, 2)],
                 ["output 5x66, one channel in the second tile", "output 4x33", "output 17x64: odd H refused by the MFMA rule",
                  "output 4x65"])
    # ---------------------------------------------------------------- conv3x3_nchw_f32_kernel<STRIDE, 8 | 2>
    + _f32_cases(_f32("direct", 1), [(1, 5, 7, 1, 1), (3, 17, 33, 17, 1), (9, 16, 16, 16, 1), (16, 8, 8, 48, 1)],
                 ["Cin 1, Cout 1", "ragged tiles, Cout 17", "exact tile", "Cout % 32 != 0 keeps a GEMM-shaped layer here"])
    + _f32_cases(_f32("direct", 2), [(1, 9, 6, 3, 2), (11, 33, 18, 20, 2)])
    + _f32_cases(_f32("direct", 4), [(3, 8, 8, 16, 4), (5, 66, 35, 33, 4), (2, 130, 9, 8, 4), (16, 64, 64, 64, 4)],
                 ["output 2x2", "output 17x9, H = 2 mod 4: the last input row is read", "output 33x3", "output 16x16"])
)

# route-only: the extractor pyramid at its true map sizes (tests/test_gpu_ops.py::test_conv3x3_nchw_f32_mfma_form launches them):
# (Cin, Cout, H = W, stride) -> instance key, cols_t x rows_t
F32_CONV_PYRAMID = [
    ((16, 32, 512, 2), _f32("mfma", 2, 32, 128), (128, 1)),    # 256-wide output: 1 x 128 pixel tiles, the widest stride-2 patch
    ((32, 32, 256, 1), _f32("mfma", 1, 32, 128), (128, 1)),
    ((32, 64, 64, 2), _f32("mfma", 2, 64, 128), (32, 4)),      # 32-wide output: 4 x 32 tiles
    ((64, 64, 128, 1), _f32("mfma", 1, 64, 128), (128, 1)),
    ((64, 160, 128, 2), _f32("mfma", 2, 32, 128), (64, 2)),    # Cout = 160: 32-channel tiles
    ((160, 160, 64, 2), _f32("mfma", 2, 32, 128), (32, 4)),
    ((160, 320, 64, 1), _f32("mfma", 1, 64, 128), (64, 2)),    # 2 x 64 tiles
    ((160, 320, 32, 1), _f32("mfma", 1, 64, 128), (32, 4)),
    ((160, 320, 32, 2), _f32("mfma", 2, 64, 128), (16, 8)),    # 16-wide output: 8 x 16 tiles
    ((320, 640, 16, 2), _f32("mfma", 2, 64, 64), (8, 8)),      # 8x8 output: the 64-pixel tile
    ((640, 1280, 8, 1), _f32("mfma", 1, 64, 64), (8, 8)),
    ((640, 64, 8, 1), _f32("mfma", 1, 64, 64), (8, 8)),
    ((320, 64, 16, 1), _f32("mfma", 1, 64, 128), (16, 8)),
    ((24, 96, 16, 1), _f32("mfma", 1, 32, 128), (16, 8)),      # Cin not a multiple of 16 (three 8-channel chunks)
]

F32_CONV_INSTANCES = 11


def enumerate_f32_conv_keys():
    """Every instance key dc_conv3x3_f32_route yields over Cin x H x W x Cout x stride: channel counts below / at / off the 8-channel
    chunk and the 16 / 32 / 64-channel tiles, power-of-two maps from 1 to 512 plus every odd and ragged size of the table.
    -> {key: example (Cin, H, W, Cout, stride)}"""
    sizes = sorted({1, 2, 4, 8, 16, 32, 64, 128, 256, 512} | {c.h for c in F32_CONV_CASES} | {c.w for c in F32_CONV_CASES})
    keys = {}
    for stride in (1, 2, 4):
        for cin in (1, 3, 8, 9, 16, 24, 40):
            for cout in (1, 3, 16, 17, 32, 48, 64, 65, 80, 96, 128, 160):
                for h in sizes:
                    for w in sizes:
                        keys.setdefault(f32_conv_key(cin, h, w, cout, stride), (cin, h, w, cout, stride))
    return keys


def f32_conv_inputs(c, i):
    """fp32 (x [N, Cin, H, W], w [Cout, Cin, 3, 3], bias [Cout]) of case i of F32_CONV_CASES (CPU; seed 2000 + i)"""
    gen = torch.Generator().manual_seed(2000 + i)
    x = torch.randn(c.n, c.cin, c.h, c.w, generator=gen) + 0.3
    w = torch.randn(c.cout, c.cin, 3, 3, generator=gen) / math.sqrt(c.cin * 9)
    b = torch.randn(c.cout, generator=gen) * 0.1
    return x, w, b


# ------------------------------------------------------------------------------------------ loop-state kernels
# (B, C, H, W): odd sizes inside one trip of the grid-stride loops, and the smallest latent-shaped state above their cap of
# 8192 workgroups x 256 threads (2,097,152 elements): 33 x 4 x 128 x 128 = 2,162,688 enters the second trip
STATE_SHAPES = [(3, 4, 5, 7), (33, 4, 128, 128)]
STATE_GUIDANCE = 3.7                              # 1 - g and g itself are not exact in fp32
DDIM_TABLE_STEPS = 100                            # timesteps 991, 981, ... 1: holds the rows the CPU tests use
DDIM_ROWS_T = (981, 951, 501, 1)


def ddim_table():
    """(timesteps list, coefficient table [steps, 4] fp32) of the SD-1.5 scaled-linear DDIM schedule at DDIM_TABLE_STEPS steps"""
    from diffcodec_amd.scheduler import DDIMScheduler
    s = DDIMScheduler()
    s.set_timesteps(DDIM_TABLE_STEPS)
    return s.timesteps.tolist(), s.coefficients()


def ddim_inputs(shape, cfg, seed):
    """fp32 (eps NHWC [(2 if cfg else 1) B, H, W, C], latents NCHW [B, C, H, W]) on the CPU"""
    b, c, h, w = shape
    gen = torch.Generator().manual_seed(seed)
    return torch.randn((2 if cfg else 1) * b, h, w, c, generator=gen), torch.randn(b, c, h, w, generator=gen)


def vae_inputs(shape, seed):
    """fp32 (moments NHWC [N, H, W, 2C], noise NCHW [N, C, H, W]) on the CPU.  Log-variances ~ N(-2, 3^2), and by flat index:
    exactly on the clamps (-30 every 7th, 20 every 11th) and beyond them (-45 every 13th, 33 every 17th).  Where the log-variance
    lies below the lower clamp the mean is 0, so that exp(-15) z is the whole result and a missing clamp is not hidden under it."""
    n, c, h, w = shape
    gen = torch.Generator().manual_seed(seed)
    mean = torch.randn(n, h, w, c, generator=gen)
    lv = (3 * torch.randn(n, h, w, c, generator=gen) - 2).reshape(-1)
    for step, v in ((7, -30.0), (11, 20.0), (13, -45.0), (17, 33.0)):
        lv[step - 1::step] = v
    lv = lv.reshape(n, h, w, c)
    mean = torch.where(lv < -30.0, torch.zeros_like(mean), mean)
    return torch.cat([mean, lv], 3).contiguous(), torch.randn(n, c, h, w, generator=gen)


# ------------------------------------------------------------------------------------------ control stage: splat
GRID_ELEMS = 8192 * 256                           # elements one trip of a grid-stride loop covers (8192 workgroups x 256 threads)
SPLAT_SHAPES = [(1, 1, 1, 1), (3, 5, 1, 13), (2, 3, 17, 1), (3, 7, 7, 9), (2, 5, 24, 40)]          # (n, c, h, w)
FLOW_FAMILIES = ("smooth", "collapse", "border", "away", "nonfinite")
METRIC_FAMILIES = ("normal", "wide")
SPLAT_LARGE = (1, 1, 1450, 1450, "smooth", "normal")      # N H W = 2,102,500 > GRID_ELEMS: every bin kernel and the gather take a
#                                                           second trip.  Smooth only: the rank pass is quadratic in the collisions.
SPLAT_CASES = [s + (f, m) for s in SPLAT_SHAPES for f in FLOW_FAMILIES for m in METRIC_FAMILIES] + [SPLAT_LARGE]


def splat_label(c):
    return "x".join(str(v) for v in c[:4]) + f"-{c[4]}-{c[5]}"


def splat_flow(family, n, h, w, gen):
    """fp32 flow [n, 2, h, w] (u = x displacement, v = y displacement) of a family:
      smooth     sigma = 1.5 px;
      collapse   every source lands on one fractional interior point (0.37 (w - 1), 0.61 (h - 1));
      border     landing coordinates exactly -1, 0, w - 1, w and -1, 0, h - 1, h, every pair: the weights are exactly 0 or 1;
      away       every source leaves the map, except source 0 of each image, which lands exactly on the last pixel;
      nonfinite  smooth with +inf, -inf, NaN and 1e30 components (every 13th flat element each)."""
    gy, gx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    if family in ("smooth", "nonfinite"):
        f = 1.5 * torch.randn(n, 2, h, w, generator=gen)
        if family == "nonfinite":
            flat = f.reshape(-1)
            for off, v in ((0, math.inf), (4, -math.inf), (8, math.nan), (12, 1e30)):
                flat[off::13] = v
        return f
    if family == "collapse":
        return torch.stack([0.37 * (w - 1) - gx, 0.61 * (h - 1) - gy])[None].repeat(n, 1, 1, 1).contiguous()
    i = torch.arange(h * w).reshape(h, w)
    if family == "border":
        tx = torch.tensor([-1.0, 0.0, w - 1.0, float(w)])[i % 4]
        ty = torch.tensor([-1.0, 0.0, h - 1.0, float(h)])[(i // 4) % 4]
        f = torch.stack([tx - gx, ty - gy])[None].repeat(n, 1, 1, 1)
        f[1::2] = torch.stack([tx - gx, torch.tensor([-1.0, 0.0, h - 1.0, float(h)])[(i // 4 + 1) % 4] - gy])   # odd images: shifted pairs
        return f.contiguous()
    assert family == "away", family
    f = torch.full((n, 2, h, w), float(w + h + 3))
    f[:, 0, 0, 0], f[:, 1, 0, 0] = w - 1.0, h - 1.0
    return f


def splat_inputs(case, seed):
    """fp32 (x [n, c, h, w], flow, metric [n, 1, h, w], mask [n, 1, h, w] of zeros and ones) of a SPLAT_CASES entry, on the CPU"""
    n, c, h, w, family, mfam = case
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(n, c, h, w, generator=gen) + 0.3
    flow = splat_flow(family, n, h, w, gen)
    if mfam == "normal":
        metric = torch.randn(n, 1, h, w, generator=gen)
    else:                                                  # exp(metric) down to 2e-9: the 1e-7 of the normaliser decides the quotient
        metric = torch.rand(n, 1, h, w, generator=gen) * 32 - 20
    mask = (torch.rand(n, 1, h, w, generator=gen) < 0.3).float()
    return x, flow, metric, mask


def splat_seed(i):
    return 11000 + i


# ------------------------------------------------------------------------------------------ control stage: occlusion mask
# (n, h, w, seed): fa ~ 0.6 N(0, 1), fb = -fa + 0.25 N(0, 1): the forward-backward residual straddles the 0.3 threshold.  Seeds are
# chosen (tests/test_launch_ref.py asserts it) so that the reference's own band |norm - 0.3| <= delta holds at most 0.5 % of the
# pixels (none below 200 pixels) and each mask value covers at least 5 %.
OCCLUSION_CASES = [(2, 24, 40, 0), (3, 7, 9, 0), (3, 1, 13, 0), (2, 33, 5, 0), (1, 64, 64, 0), (3, 128, 96, 0), (2, 17, 1, 0)]


def occlusion_inputs(case):
    n, h, w, seed = case
    gen = torch.Generator().manual_seed(12000 + seed)
    fa = 0.6 * torch.randn(n, 2, h, w, generator=gen)
    fb = -fa + 0.25 * torch.randn(n, 2, h, w, generator=gen)
    return fa, fb


# ------------------------------------------------------------------------------------------ control stage: flow resize, fusion
FLOW_RESIZE_CASES = [(2, 128, 128, 16, 16), (3, 7, 9, 5, 3), (1, 5, 3, 7, 9), (2, 1, 1, 2, 2), (2, 64, 96, 2, 2)]   # (n, H, W, h, w)
FLOW_RESIZE_DIVIDE_ONLY = [(1, 9, 7, 1, 1)]                        # the normalising launcher refuses h = 1 or w = 1 (a zero divisor)
FLOW_DIVISORS = (8.0, 4.0)                                          # div_x != div_y


def flow_resize_input(case, seed):
    """fp32 [n, 6, H, W]; the launch reads planes 2:4"""
    n, hh, ww, _, _ = case
    return 3 * torch.randn(n, 6, hh, ww, generator=torch.Generator().manual_seed(13000 + seed)) + 0.5


FUSE_CASES = [(3, 7, 5, 9), (1, 1, 1, 1), (2, 320, 8, 8)]          # (n, c, h, w)


def fuse_inputs(case, seed):
    """fp32 (wf, wl [n, c, h, w], cf, cb, of, ob [n, 1, h, w]).  Confidences ~ N(0.3, 1) and, by flat pixel index: both <= 0 (every
    5th), one negative (every 7th), 1e4 (every 11th).  Occlusion pairs cycle (0,0) (1,0) (0,1) (1,1): sums of exactly 0, 1 and 2."""
    n, c, h, w = case
    gen = torch.Generator().manual_seed(14000 + seed)
    wf, wl = torch.randn(n, c, h, w, generator=gen) + 0.2, torch.randn(n, c, h, w, generator=gen) - 0.1
    cf, cb = (torch.randn(n * h * w, generator=gen) + 0.3 for _ in range(2))
    cf[4::5], cb[4::5] = -0.5, 0.0
    cf[6::7] = -2.0
    cb[10::11] = 1e4
    if n * h * w == 1:
        cf[0], cb[0] = -0.5, 0.0
    i = torch.arange(n * h * w) + (n * h * w == 1) * 3          # a single pixel: the (1, 1) pair
    of, ob = (i % 2).float(), ((i // 2) % 2).float()
    return (wf, wl) + tuple(t.reshape(n, 1, h, w).contiguous() for t in (cf, cb, of, ob))


# ------------------------------------------------------------------------------------------ plain elementwise launchers
SILU_SPECIALS = (104.0, -104.0, 88.7, -88.7, 20.0, -20.0, 1e-30, -1e-30, 0.0, -0.0)
ELEMENTWISE_CASES = {
    "silu_f32": [1, 255, 257, GRID_ELEMS + 1],
    "add_f32": [1, 255, 257, GRID_ELEMS + 1],
    "lincomb": [(n, t) for n in (1, 255, 257, GRID_ELEMS + 1) for t in (1, 2, 3, 4)],
    "f32_to_bf16": [1, 255, 257, GRID_ELEMS + 1],
    "add_bf16": [8, 2056, 8 * (GRID_ELEMS + 1)],
    "nchw_f32_to_nhwc_bf16": [(3, 5, 7, 9), (1, 1, 1, 1), (2, 320, 3, 2), (1, 4, 725, 725)],          # (n, c, h, w)
    "nhwc_bf16_to_nchw_f32": [(3, 5, 7, 9), (1, 1, 1, 1), (2, 320, 3, 2), (1, 4, 725, 725)],
    "nhwc_f32_to_nchw_f32": [(3, 5, 7, 9), (1, 1, 1, 1), (2, 320, 3, 2), (1, 4, 725, 725)],
    "transpose_bf16": [(3, 33, 31), (1, 1, 1), (2, 77, 40)],                                           # (b, r, c)
    "freeu_lowfreq": [(2, 2, 2, 8), (2, 5, 16, 24)],                                                    # (n, h, w, c)
    "freeu_backbone": [(3, 5, 16), (2, 7, 80)],                                                         # (n, pixels, c)
    "timestep_embedding": [(3, 320, 2), (1, 6, 0)],                                                     # (n, dim, step index into 4)
    "embed_tokens": [(2, 5, 8, 11), (3, 77, 1024, 49), (1, 77, 1032, 49)],                              # (b, t, c, vocab)
    "postprocess_image": [(2, 3, 5, 7, xs, f32, u8) for xs in (3, 4) for f32, u8 in ((True, False), (False, True), (True, True))],
}
LINCOMB_COEFS = (0.7, -1.3, 0.21, 3.7)
TIMESTEP_TABLE = (981.0, 501.0, 21.0, 1.0)


def elementwise_input(n, seed, specials=()):
    x = 3 * torch.randn(n, generator=torch.Generator().manual_seed(15000 + seed))
    k = min(n, len(specials))
    x[:k] = torch.tensor(specials[:k])
    if n > len(specials) and specials:
        x[-len(specials):] = torch.tensor(specials)        # ... and at the tail (the second trip of the large case)
    return x


def postprocess_input(n, c, h, w, xs):
    """fp32 [n, h, w, xs] whose first c channels are the launch's input: ~ N(0, 1) with values below -1, above 1 and exactly +-1"""
    x = torch.randn(n, h, w, xs, generator=torch.Generator().manual_seed(16000 + xs))
    flat = x.reshape(-1)
    for off, v in ((0, -1.0), (1, 1.0), (2, -1.5), (3, 2.0), (4, -1.0000001), (5, 0.99999994)):
        flat[off::17] = v
    return x


# ------------------------------------------------------------------------------------------ frame quality metrics
# operand form -> (element type, storage of X, storage of Y).  nhwc / nchw: contiguous; pitched: NHWC rows of W C + 13 elements,
# the gap holding the guard pattern (a window cropped from a wider frame).  `mixed` gives X and Y different stride sets.
METRIC_FORMS = {"u8_nhwc": ("u8", "nhwc", "nhwc"), "u8_nchw": ("u8", "nchw", "nchw"), "f32_nchw": ("f32", "nchw", "nchw"),
                "f32_view": ("f32", "nhwc", "nhwc"), "pitched": ("u8", "pitched", "pitched"), "mixed": ("f32", "nhwc", "nchw")}
METRIC_FAMILIES_ALL = ("noisy", "identical", "constant", "anti", "extremes", "nan")
K_DEFAULT, K_WIDE = (0.01, 0.03), (0.02, 0.05)
PITCH_GAP = 13
MS_WEIGHTS = {1: (1.0,), 2: (0.4, 0.6), 3: (0.2, 0.3, 0.5), 5: (0.0448, 0.2856, 0.3001, 0.2363, 0.1333),
              8: (0.05, 0.1, 0.15, 0.2, 0.2, 0.15, 0.1, 0.05)}


@dataclass(frozen=True)
class MetricCase:
    """One dc_ssim (levels = 0), dc_ms_ssim (levels >= 1, weights MS_WEIGHTS[levels]) or dc_psnr (ws = 0) launch."""
    n: int
    c: int
    h: int
    w: int
    ws: int = 11
    form: str = "u8_nhwc"
    family: str = "noisy"
    L: float = 255.0
    K: tuple = K_DEFAULT
    levels: int = 0
    nonneg: bool = False
    note: str = ""

    @property
    def dtype(self):
        return METRIC_FORMS[self.form][0]

    @property
    def weights(self):
        return MS_WEIGHTS[self.levels] if self.levels else None

    @property
    def exact(self):
        """the value every output element must equal bit for bit, or None"""
        if self.family == "identical":
            return 1.0
        if self.family == "anti" and (self.levels or self.nonneg):
            return 0.0
        return None

    def label(self):
        f = [f"ws{self.ws}"] * bool(self.ws) + [f"lv{self.levels}"] * bool(self.levels) + [self.form, self.family, f"L{self.L:g}"]
        f += ["Kwide"] * (self.K != K_DEFAULT) + ["nonneg"] * self.nonneg
        return f"{self.n}x{self.c}x{self.h}x{self.w}-" + "-".join(f)


def ssim_instance(c):
    return ("ssim", c.ws, c.dtype)


def _ssim_cases():
    forms_u8, forms_f32 = ("u8_nhwc", "u8_nchw", "pitched"), ("f32_nchw", "f32_view", "mixed")
    out = []
    for i, ws in enumerate((1, 3, 5, 7, 9, 11, 13, 15)):
        for j, forms in enumerate((forms_u8, forms_f32)):
            L = 255.0 if (j == 0 or i % 2) else 1.0
            k = K_WIDE if (i + j) % 2 else K_DEFAULT
            # one output pixel; the seam shape: 2 x 2 tiles, the last tile 1 column by 1 row
            out.append(MetricCase(2, 1, ws, ws, ws, forms[i % 3], "noisy", L, k, nonneg=bool(i % 2), note="one output pixel"))
            out.append(MetricCase(3, 2, 32 + ws, 64 + ws, ws, forms[(i + 1) % 3], "noisy", L, k, note="seam: Ho 33, Wo 65"))
    out += [
        MetricCase(1, 2, 42, 74, 11, "u8_nhwc", note="Ho 32, Wo 64: exactly one tile"),
        MetricCase(1, 2, 42, 74, 11, "mixed", L=1.0, K=K_WIDE, note="Ho 32, Wo 64, two stride sets"),
        MetricCase(1, 1, 18, 30, 11, "f32_nchw", L=1.0, note="Ho 8: exactly one wave's rows"),
        MetricCase(2, 1, 19, 75, 11, "pitched", note="Ho 9, Wo 65"),
        MetricCase(1, 1, 1, 16385, 1, "f32_nchw", note="257 tiles: the reduce kernel's second trip"),
        MetricCase(1, 1, 1, 16385, 1, "u8_nchw", family="identical", note="257 tiles, exact"),
        MetricCase(257, 1, 3, 3, 3, "u8_nhwc", note="N = 257: the finalize kernel's second trip"),
        MetricCase(257, 1, 3, 3, 3, "f32_view", L=1.0, nonneg=True, note="N = 257"),
        MetricCase(2, 4, 13, 20, 11, "u8_nhwc", note="C = 4"),
        MetricCase(2, 4, 13, 20, 11, "mixed", note="C = 4, two stride sets"),
    ]
    # value families at a shape with a partial tile in each direction, nonnegative on and off
    for fam in ("identical", "constant", "anti", "extremes", "nan"):
        for nonneg in (False, True):
            forms = ("f32_view", "mixed") if fam == "nan" else ("u8_nhwc", "f32_nchw")
            L = 1.0 if (nonneg and fam != "nan") else 255.0
            out.append(MetricCase(2, 3, 21, 70, 7, forms[int(nonneg)], fam, L, K_WIDE if nonneg else K_DEFAULT, nonneg=nonneg))
    out += [MetricCase(2, 1, 5, 5, 5, "mixed", "nan", 1.0, note="one output pixel, NaN"),
            MetricCase(2, 2, 5, 5, 5, "u8_nchw", "anti", nonneg=True, note="one output pixel, anti")]
    return out


def _ms_ssim_cases():
    out = [
        MetricCase(3, 2, 33, 35, 3, "u8_nhwc", levels=5, note="33 -> 17 -> 9 -> 5 -> 3, 35 -> 18 -> 9 -> 5 -> 3"),
        MetricCase(3, 2, 33, 35, 3, "f32_view", L=1.0, K=K_WIDE, levels=5),
        MetricCase(3, 2, 33, 35, 3, "mixed", "nan", levels=5),
        MetricCase(3, 2, 33, 35, 3, "f32_nchw", "anti", 1.0, levels=5),
        MetricCase(3, 2, 33, 35, 3, "u8_nchw", "identical", levels=5),
        MetricCase(3, 2, 33, 35, 3, "pitched", "constant", levels=5),
        MetricCase(3, 2, 33, 35, 3, "u8_nhwc", "extremes", levels=5),
        MetricCase(1, 1, 225, 227, 15, "u8_nchw", levels=5, note="every scale ends at the 15-tap window"),
        MetricCase(2, 3, 161, 161, 11, "mixed", levels=5, note="the smallest default-window frame"),
        MetricCase(1, 3, 1, 1, 1, "f32_nchw", L=1.0, levels=8, note="eight levels of one pixel"),
        MetricCase(2, 1, 129, 2, 1, "u8_nhwc", levels=8, note="eight levels: 129 -> 65 -> 33 -> 17 -> 9 -> 5 -> 3 -> 2"),
        MetricCase(1, 3, 47, 90, 7, "f32_view", levels=1, note="one level through dc_ms_ssim"),
        MetricCase(1, 1, 45, 77, 5, "pitched", levels=3, note="three weights"),
    ]
    for h, w in ((23, 24), (24, 23), (23, 23), (24, 24)):            # the first pool of each element type meets every padding parity
        out.append(MetricCase(2, 2, h, w, 5, "u8_nhwc", levels=2))
        out.append(MetricCase(2, 2, h, w, 5, "mixed", L=1.0, K=K_WIDE, levels=2))
    return out


def _psnr_cases():
    shapes = [(3, 1, 1, 1), (3, 3, 21, 255), (3, 1, 64, 256), (3, 5, 13, 257), (3, 3, 43, 513), (3, 1, 63, 1), (3, 1, 129, 255)]
    forms = list(METRIC_FORMS)
    out = [MetricCase(*s, 0, forms[i % 6], "noisy", 255.0 if METRIC_FORMS[forms[i % 6]][0] == "u8" or i % 2 else 1.0) for i, s in enumerate(shapes)]
    out += [MetricCase(3, 3, 43, 257, 0, f, "noisy") for f in forms]           # every form at C H = 129, W = 257
    out += [MetricCase(3, 3, 43, 513, 0, "u8_nhwc", "extremes", note="every |d| = 255"),
            MetricCase(3, 1, 65, 257, 0, "u8_nchw", "onepixel", note="one pixel differs by 1"),
            MetricCase(3, 1, 65, 257, 0, "f32_view", "onepixel", 1.0),
            MetricCase(3, 1, 65, 257, 0, "pitched", "identical"),
            MetricCase(3, 2, 32, 256, 0, "mixed", "identical", 1.0)]
    return out


SSIM_CASES, MS_SSIM_CASES, PSNR_CASES = _ssim_cases(), _ms_ssim_cases(), _psnr_cases()


def metric_window(ws, sigma=1.5):
    """the fp32 taps a launch is given (diffcodec_amd.metrics.gaussian_window, rounded to fp32)"""
    c = torch.arange(ws, dtype=torch.float64) - ws // 2
    g = torch.exp(-(c ** 2) / (2.0 * sigma * sigma))
    return (g / g.sum()).float()


def nan_position(c):
    """(n, channel, y, x) of the NaN pixel of the `nan` family: the last channel of sample min(1, N - 1)"""
    return (min(1, c.n - 1), c.c - 1, c.h // 2, c.w // 2)


def metric_inputs(c, seed):
    """logical NCHW (X, Y) of a case on the CPU, uint8 or fp32 in [0, L]:
      noisy      a smooth field (a sinusoid of random phase per plane plus texture) and a noisy copy;
      identical  Y = X;                      constant  two different constants (0.3 L, 0.6 L);
      anti       Y = L - X (cs < 0);         extremes  0 against L;
      nan        noisy with one NaN pixel in X (nan_position; float forms only);
      onepixel   Y = X but for one element per sample, off by 1 (uint8) or L / 255 (PSNR only)."""
    gen = torch.Generator().manual_seed(17000 + seed)
    shape = (c.n, c.c, c.h, c.w)
    gy, gx = torch.arange(c.h, dtype=torch.float32)[:, None], torch.arange(c.w, dtype=torch.float32)[None, :]
    x = 0.5 + 0.3 * torch.sin(0.37 * gx + 0.23 * gy + 6.28 * torch.rand(c.n, c.c, 1, 1, generator=gen))
    x = (x + 0.08 * torch.randn(shape, generator=gen)).clamp(0, 1)
    y = (x + 0.05 * torch.randn(shape, generator=gen)).clamp(0, 1)
    if c.family == "constant":
        x, y = torch.full(shape, 0.3), torch.full(shape, 0.6)
    elif c.family == "extremes":
        x, y = torch.zeros(shape), torch.ones(shape)
    u8 = c.dtype == "u8"
    x, y = ((t * 255.0).round().to(torch.uint8) if u8 else (t * c.L).float() for t in (x, y))
    if c.family in ("identical", "onepixel"):
        y = x.clone()
    if c.family == "onepixel":
        for n in range(c.n):
            v = y[n, c.c - 1, c.h - 1, c.w - 1 - n]
            y[n, c.c - 1, c.h - 1, c.w - 1 - n] = (v + 1 if v < 255 else v - 1) if u8 else v + (c.L / 255 if v < c.L / 2 else -c.L / 255)
    if c.family == "anti":
        y = 255 - x if u8 else (c.L - x).float()
    if c.family == "nan":
        assert not u8 and c.n >= 2
        x[nan_position(c)] = math.nan
    return x, y


def metric_operand(t, layout, device):
    """a logical NCHW tensor stored as `layout` in a Guarded buffer -> (Guarded, element strides (n, c, h, w)); the operand's
    address is the view's data_ptr()"""
    n, c, h, w = t.shape
    if layout == "nchw":
        g, strides = Guarded((n, c, h, w), t.dtype, device), (c * h * w, h * w, w, 1)
        g.fill(t)
    elif layout == "nhwc":
        g, strides = Guarded((n, h, w, c), t.dtype, device), (h * w * c, 1, w * c, c)
        g.fill(t.permute(0, 2, 3, 1))
    else:
        assert layout == "pitched", layout
        pitch = w * c + PITCH_GAP
        g, strides = Guarded((n, h, w * c), t.dtype, device, pitch=pitch), (h * pitch, 1, pitch, c)
        g.fill(t.permute(0, 2, 3, 1).reshape(n, h, w * c))
    return g, strides


def metric_read(g, shape, strides):
    """the logical NCHW tensor a kernel reads from a metric_operand through `strides`"""
    return torch.as_strided(g.base, shape, strides, g.guard)


# (label, (N, C, H, W, win_size, levels)): dc_ssim_ws_bytes and the launch return -1 and the launch writes nothing
METRIC_REFUSALS = [("even window", (1, 1, 32, 32, 10, 1)), ("window 17", (1, 1, 32, 32, 17, 1)), ("levels 0", (1, 1, 32, 32, 3, 0)),
                   ("levels 9", (1, 1, 1024, 1024, 1, 9)), ("a scale below the window", (1, 1, 20, 20, 11, 2)),
                   ("N C = 65536", (65536, 1, 3, 3, 3, 1)), ("N C = 65536 by channels", (256, 256, 3, 3, 3, 1))]


# ------------------------------------------------------------------------------------------ FDN modulate, input side, tile blend
FDN_VEC_CAP = 4096 * 256                      # 8-channel vectors one trip of fdn_modulate_kernel covers
FDN_CASES = [(3, 2, 63, 64), (1, 1, 1, 8), (4, 4, 16, 320), (3, 1, 7, 1288), (3, 2, 4096, 704)]      # (N, Bp, HW, C)
FLOW_HW2_CASES = [(270, 480, 64, 64), (1, 7, 5, 9), (7, 1, 9, 5), (5, 3, 1, 1), (64, 96, 33, 1), (9, 9, 9, 9), (3, 5, 97, 131)]   # (H, W, th, tw)
PACK_CASES = [(1, 1), (37, 53), (1450, 1450)]                                                        # 1450^2 = 2,102,500 > GRID_ELEMS


def fdn_inputs(case, seed):
    """fp32 (x [N, HW, C], ab [N, C, 2], gamma, beta [Bp, HW, C]) on the CPU"""
    n, bp, hw, c = case
    gen = torch.Generator().manual_seed(18000 + seed)
    x = 2 * torch.randn(n, hw, c, generator=gen) + 0.5
    ab = torch.stack([1 + 0.3 * torch.randn(n, c, generator=gen), 0.5 * torch.randn(n, c, generator=gen)], -1)
    return x, ab, 0.5 * torch.randn(bp, hw, c, generator=gen), 0.5 * torch.randn(bp, hw, c, generator=gen)


def flow_hw2_input(case, seed):
    """fp32 [H, W, 2] (the .flo payload layout)"""
    return 6 * torch.randn(case[0], case[1], 2, generator=torch.Generator().manual_seed(19000 + seed)) + 0.5


def pack_inputs(case):
    """two uint8 [H, W, 3] images that together hold every byte value (each does, from 86 pixels up)"""
    h, w = case
    i = torch.arange(h * w * 3)
    a = ((i * 7 + 3) % 256).to(torch.uint8).reshape(h, w, 3)
    b = (255 - (i * 11) % 256).to(torch.uint8).reshape(h, w, 3)
    return a, b


@dataclass(frozen=True)
class BlendCase:
    """One dc_blend_tiles_ramp_u8 launch: tiles [T, C, th, tw] on the windows `coords` (y1, y2, x1, x2) of an H x W frame."""
    name: str
    c: int
    h: int
    w: int
    th: int
    tw: int
    feather: int
    coords: tuple
    scale: float = 255.0
    values: str = "unit"           # unit: [0, 1];  ties: k + 0.5 (scale 1);  clip: [-0.3, 1.3]


def _grid_coords(h, w, th, tw, ys, xs):
    return tuple((y, y + th, x, x + tw) for y in ys for x in xs)


BLEND_CASES = [
    BlendCase("single-window", 3, 20, 28, 20, 28, 4, ((0, 20, 0, 28),)),
    BlendCase("c1-abutting-feather0", 1, 16, 24, 8, 12, 0, _grid_coords(16, 24, 8, 12, (0, 8), (0, 12))),
    BlendCase("c2-feather-half-tile", 2, 12, 20, 8, 8, 4, _grid_coords(12, 20, 8, 8, (0, 4), (0, 4, 8, 12))),
    BlendCase("c4-3x3-nonsquare", 4, 40, 57, 20, 27, 5, _grid_coords(40, 57, 20, 27, (0, 10, 20), (0, 15, 30))),
    BlendCase("c3-ties", 3, 24, 24, 16, 16, 0, _grid_coords(24, 24, 16, 16, (0, 8), (0, 8)), 1.0, "ties"),
    BlendCase("c3-clip", 3, 40, 57, 20, 27, 5, _grid_coords(40, 57, 20, 27, (0, 10, 20), (0, 15, 30)), 255.0, "clip"),
]


def blend_inputs(case, seed):
    """fp32 tiles [T, C, th, tw] on the CPU.  ties: every tile of a window position holds the same k + 0.5 (k cycling 0 .. 254 by
    pixel of the frame), so that with feather = 0 every weighted mean is exactly k + 0.5 and rint must round to even."""
    t = len(case.coords)
    gen = torch.Generator().manual_seed(20000 + seed)
    if case.values == "ties":
        frame = ((torch.arange(case.h * case.w * case.c) * 3) % 255).float().reshape(case.c, case.h, case.w) + 0.5
        return torch.stack([frame[:, y1:y2, x1:x2] for (y1, y2, x1, x2) in case.coords]).contiguous()
    x = torch.rand(t, case.c, case.th, case.tw, generator=gen)
    return x * 1.6 - 0.3 if case.values == "clip" else x
