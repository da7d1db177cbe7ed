"""Shadow harness: checks every HIP launch of a model run against the fp64 references of oracle/launch_ref.py.

    with LaunchShadow() as sh:
        pipe(...)
    sh.raise_on_failure()

Inside the context the `ops.*` functions below are replaced by wrappers (every model file calls them as `ops.X`, and
`ops.linear` / `ops.conv_gn_silu` reach `ops.conv` through the module globals).  Each wrapper snapshots the inputs whose storage
overlaps `out=`, runs the real op, synchronises, and holds the sampled output rows against the reference computed from the
operands that launch read.  `lib.call` is wrapped too, to capture the `dc_conv_desc` of each `dc_conv_igemm_bf16` launch and ask
`dc_conv_route` which kernel ran.  Nothing in the product changes.  Per (route, epilogue mode, split-K > 1) the harness keeps the
launch count and the worst err/tol ratio."""
import contextlib
import math

import torch

from diffcodec_amd import lib, ops
from oracle import launch_ref as L


def _span(t):
    if t.numel() == 0:
        return t.data_ptr(), t.data_ptr()
    last = sum((n - 1) * st for n, st in zip(t.shape, t.stride()))
    return t.data_ptr(), t.data_ptr() + (last + 1) * t.element_size()


def _overlaps(a, b):
    if not (torch.is_tensor(a) and torch.is_tensor(b)):
        return False
    a0, a1 = _span(a)
    b0, b1 = _span(b)
    return a0 < b1 and b0 < a1


class LaunchShadow:
    def __init__(self, record=None, prefix="shadow"):
        self.stats = {}            # key -> [count, worst ratio]
        self.failures = []
        self.calls = 0
        self.record = record
        self.prefix = prefix
        self._last_route = None
        self._stack = None
        self.band = {}             # occlusion masks: (n, h, w) -> [launches, largest share of pixels inside the reference's own band]

    # ---------------------------------------------------------------- bookkeeping
    def _note(self, key, verdict, what):
        st = self.stats.setdefault(key, [0, 0.0])
        st[0] += 1
        st[1] = max(st[1], verdict["ratio"])
        if not verdict["ok"]:
            self.failures.append(f"call {self.calls} route {key}: {what}: worst (row, col) {verdict['worst']} err {verdict['err']:.3e} "
                                 f"tol {verdict['tol']:.3e} err/tol {verdict['ratio']:.3g} rel-rms {verdict['rms']:.3e}")

    def raise_on_failure(self):
        if self.failures:
            raise L.Mismatch(f"{len(self.failures)} launch(es) off their fp64 reference:\n" + "\n".join(self.failures[:20]))

    def report(self):
        if self.record is not None:
            for key, (n, worst) in sorted(self.stats.items(), key=lambda kv: str(kv[0])):
                self.record(f"{self.prefix}[{'/'.join(str(k) for k in key)}]", f"launches={n} worst_err_over_tol={worst:.4f}")
            for shape, (n, share) in sorted(self.band.items()):
                self.record(f"{self.prefix}[occlusion_mask/band/{'x'.join(str(v) for v in shape)}]", f"launches={n} band_share={share:.6f}")
        return self.stats

    def routes(self):
        return {k for k in self.stats if k[0] in ops.ROUTE_NAMES.values()}

    # ---------------------------------------------------------------- wrappers
    def _lib_call(self, real):
        def call(name, *args, meta=None):
            if name == "dc_conv_igemm_bf16":
                self._last_route = ops.conv_route(args[0])
            return real(name, *args, meta=meta)
        return call

    def _conv(self, real):
        def conv(x1, pc, **kw):
            self.calls += 1
            out = kw.get("out")
            snap = {}                       # operands the launch may overwrite: snapshots for the reference, the launch reads the originals
            if out is not None:
                for name in ("residual", "x2"):
                    if _overlaps(out, kw.get(name)):
                        snap[name] = kw[name].clone()
            x1_ref = x1.clone() if _overlaps(out, x1) else x1
            self._last_route = None
            y = real(x1, pc, **kw)
            torch.cuda.synchronize()
            kw = dict(kw, **snap)
            x1 = x1_ref
            rt = self._last_route
            key = (rt.kernel, rt.epi, rt.splitk > 1) if rt is not None else (pc.kind, 0, False)
            c = y.shape[-1]
            m = y.numel() // c
            spatial = (y.shape[0], y.shape[1], y.shape[2]) if pc.ksize == 3 else None
            rows = L.sample_rows(m, spatial=spatial, row_bytes=[c * y.element_size(), x1.shape[-1] * 2 if pc.ksize == 1 else 0])
            r, s = L.conv_ref(x1, pc, rows, x2=kw.get("x2"), gn_ab=kw.get("gn_ab"), gn_silu=kw.get("gn_silu", False),
                              row_add=kw.get("row_add"), residual=kw.get("residual"), stride=kw.get("stride", 1), pad=kw.get("pad", 1),
                              upsample=kw.get("upsample", False), out_scale=kw.get("out_scale", 1.0), act=kw.get("act", 0))
            yr = y.reshape(m, c)[rows.to(y.device)]
            flags = ",".join(f for f in ("x2", "gn_ab", "row_add", "residual", "ln_stats", "ln_partials", "stats_out") if kw.get(f) is not None)
            flags += (",gn_silu" if kw.get("gn_silu") else "") + (",geglu" if pc.geglu else "") + (f",act={kw['act']}" if kw.get("act") else "")
            what = f"{pc.ksize}x{pc.ksize} {tuple(x1.shape)} -> {tuple(y.shape)} splitk={rt.splitk if rt else 1} [{flags}]"
            self._note(key, L.check(yr, r, s, y.dtype), what)
            so = kw.get("stats_out")
            if so is not None:
                tr, ts = L.row_stats_totals_ref(yr)
                self._note(key + ("stats_out",), L.check(so[rows.to(so.device)].to(torch.float64).sum(1), tr, ts, torch.float32), what)
            gp = getattr(y, "gn_part", None)
            if gp is not None:
                tr, ts = L.gn_part_totals_ref(y)
                self._note(key + ("gn_part",), L.check(gp.to(torch.float64).sum(0), tr, ts, torch.float32), what)
            return y
        return conv

    def _simple(self, name, real, ref):
        """ops function -> wrapper that checks `ref(args, kwargs, y) -> (y_rows, r, s, out_dtype)`"""
        def fn(*a, **kw):
            self.calls += 1
            out = kw.get("out")
            a_ref = tuple(t.clone() if _overlaps(out, t) else t for t in a)     # snapshots for the reference only
            y = real(*a, **kw)
            torch.cuda.synchronize()
            yr, r, s, dt = ref(a_ref, kw, y)
            self._note((name, 0, False), L.check(yr, r, s, dt), f"{name} {tuple(y.shape) if torch.is_tensor(y) else ''}")
            return y
        return fn

    def __enter__(self):
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("the launch shadow cannot run inside a stream capture (it synchronises and reads results)")
        st = contextlib.ExitStack()
        self._stack = st
        mp = st.enter_context(_Patch())
        mp.set(lib, "call", self._lib_call(lib.call))
        mp.set(ops, "conv", self._conv(ops.conv))

        def rows_of(y, spatial=None):
            c = y.shape[-1]
            return L.sample_rows(y.numel() // c, spatial=spatial)

        def flat(y, rows):
            return y.reshape(-1, y.shape[-1])[rows.to(y.device)]

        def attention(a, kw, y):
            q, k, v, heads = a[:4]
            rows = rows_of(y)
            r, s = L.attention_ref(q, k, v, heads, rows, scale=kw.get("scale", a[4] if len(a) > 4 else None))
            return flat(y, rows), r, s, y.dtype

        def gn_apply(a, kw, y):
            x, ab = a[:2]
            silu = kw.get("silu", a[2] if len(a) > 2 else False)
            x2 = kw.get("x2", a[3] if len(a) > 3 else None)
            rows = rows_of(y)
            r, s = L.gn_apply_ref(x, ab, rows, silu=silu, x2=x2)
            return flat(y, rows), r, s, y.dtype

        def layer_norm(a, kw, y):
            x, g, b = a[:3]
            eps = kw.get("eps", a[3] if len(a) > 3 else 1e-5)
            rows = rows_of(y)
            r, s = L.layer_norm_ref(x, g, b, eps, rows)
            return flat(y, rows), r, s, y.dtype

        def fdn(a, kw, y):
            rows = rows_of(y)
            r, s = L.fdn_modulate_ref(*a[:4], rows)
            return flat(y, rows), r, s, y.dtype

        def row_stats(a, kw, y):
            rows = L.sample_rows(y.shape[0])
            r, s = L.row_stats_ref(a[0], rows)
            return y[rows.to(y.device)], r, s, torch.float32

        def ln_fin(a, kw, y):
            rows = L.sample_rows(y.shape[0])
            r, s = L.ln_finalize_ref(a[0], a[1], a[2], rows)
            return y[rows.to(y.device)], r, s, torch.float32

        def softmax(a, kw, y):
            rows = L.sample_rows(y.shape[0])
            r, s = L.softmax_rows_ref(a[0], a[1], rows)
            return y[rows.to(y.device)], r, s, y.dtype

        def add(a, kw, y):
            rows = rows_of(y)
            r, s = L.add_ref(a[0], a[1], rows)
            return flat(y, rows), r, s, y.dtype

        def f2b(a, kw, y):
            rows = rows_of(y)
            r, s = L.f32_to_bf16_ref(a[0], rows)
            return flat(y, rows), r, s, y.dtype

        def transpose(a, kw, y):
            b_, c_, r_ = y.shape
            rows = L.sample_rows(b_ * c_)
            r, _ = L.transpose_ref(a[0], rows)
            return y.reshape(-1, r_)[rows.to(y.device)], r, torch.zeros_like(r), torch.float32   # exact: e_out 2^-20 of |r| only

        def backbone(a, kw, y):
            rows = rows_of(y)
            r, s = L.freeu_backbone_ref(a[0], a[1], rows)
            return flat(y, rows), r, s, y.dtype

        def lowfreq(a, kw, y):
            rows = rows_of(y)
            r, s = L.freeu_lowfreq_ref(a[0], a[1], rows)
            return flat(y, rows), r, s, y.dtype

        def temb(a, kw, y):
            t_dev, n, dim = a[:3]
            step = kw.get("step_dev", a[3] if len(a) > 3 else None)
            t = float(t_dev.reshape(-1)[0 if step is None else int(step.reshape(-1)[0])])
            r, s = L.timestep_embedding_ref(t, n, dim)
            return y, r.to(y.device), s.to(y.device), y.dtype

        def attention_causal(a, kw, y):
            q, k, v, heads = a[:4]
            rows = rows_of(y)
            r, s = L.attention_ref(q, k, v, heads, rows, scale=kw.get("scale", a[4] if len(a) > 4 else None), causal=True)
            return flat(y, rows), r, s, y.dtype

        def conv_f32(a, kw, y):
            x, pc = a[:2]
            stride = kw.get("stride", a[2] if len(a) > 2 else 1)
            silu = kw.get("silu", a[3] if len(a) > 3 else False)
            n, co, ho, wo = y.shape
            rows = L.sample_rows(n * ho * wo, spatial=(n, ho, wo))
            r, s = L.conv3x3_nchw_f32_ref(x, pc.w, pc.bias, rows, stride=stride, silu=silu)
            yr = y.permute(0, 2, 3, 1).reshape(-1, co)[rows.to(y.device)]
            return yr, r, s, y.dtype

        for name, ref in (("attention", attention), ("attention_causal", attention_causal), ("conv3x3_nchw_f32", conv_f32), ("gn_apply", gn_apply), ("layer_norm", layer_norm), ("fdn_modulate", fdn),
                          ("row_stats", row_stats), ("ln_finalize", ln_fin), ("softmax_rows", softmax), ("add_bf16", add),
                          ("f32_to_bf16", f2b), ("transpose_bf16", transpose), ("freeu_backbone", backbone),
                          ("freeu_lowfreq", lowfreq), ("timestep_embedding", temb)):
            mp.set(ops, name, self._simple(name, getattr(ops, name), ref))
        mp.set(ops, "group_norm_ab", self._gn_ab(ops.group_norm_ab))

        # ------------------------------------------------ control stage, layout conversions, loop entry / exit (fp32 and exact)
        def sub(y, r, s):
            """full maps up to 2^22 elements; above, the usual row sample over the map's rows of W elements"""
            if r.numel() <= 1 << 22:
                return y, r, s
            w = r.shape[-1]
            rows = L.sample_rows(r.numel() // w).to(r.device)
            return tuple(t.reshape(-1, w)[rows] for t in (y, r, s))

        def splat_soft(a, kw, y):
            r, s, _ = L.splat_soft_ref(a[0], a[1], a[2], kw.get("mask", a[3] if len(a) > 3 else None))
            return sub(y, r, s) + (y.dtype,)

        def flow_norm(a, kw, y):
            h, w = a[1], a[2]
            return sub(y, *L.flow_resize_ref(a[0], h, w, (w - 1) / 2.0, (h - 1) / 2.0)) + (y.dtype,)

        def flow_div(a, kw, y):
            return sub(y, *L.flow_resize_ref(*a[:5])) + (y.dtype,)

        def fuse(a, kw, y):
            of = kw.get("of", a[4] if len(a) > 4 else None)
            ob = kw.get("ob", a[5] if len(a) > 5 else None)
            return sub(y, *L.fuse_warped_ref(*a[:4], of, ob)) + (y.dtype,)

        def add_f32(a, kw, y):
            return sub(y, *L.add_f32_ref(a[0], a[1])) + (y.dtype,)

        def exact(ref):
            def fn(a, kw, y):
                r = ref(a[0]).to(L.F64)
                return sub(y, r, torch.zeros_like(r)) + (torch.float32,)        # exact: e_out 2^-20 of |r| only, far below one bf16 ulp
            return fn

        def to_model_input(a, kw, y):
            mul = kw.get("mul", a[1] if len(a) > 1 else 1.0)
            rep = kw.get("rep", a[2] if len(a) > 2 else 1)
            return sub(y, *L.latents_to_model_input_ref(a[0], mul, rep)) + (y.dtype,)

        for name, ref in (("splat_soft", splat_soft), ("flow_resize_normalize", flow_norm), ("flow_resize_divide", flow_div),
                          ("fuse_warped", fuse), ("add_f32", add_f32), ("latents_to_model_input", to_model_input),
                          ("nchw_f32_to_nhwc_bf16", exact(L.nchw_f32_to_nhwc_bf16_ref)),
                          ("nhwc_bf16_to_nchw_f32", exact(L.nhwc_to_nchw_f32_ref)), ("nhwc_f32_to_nchw_f32", exact(L.nhwc_to_nchw_f32_ref))):
            mp.set(ops, name, self._simple(name, getattr(ops, name), ref))
        mp.set(ops, "occlusion_mask", self._occlusion(ops.occlusion_mask))
        mp.set(ops, "postprocess_image", self._postprocess(ops.postprocess_image))
        return self

    def _occlusion(self, real):
        def fn(flow_a, flow_b):
            self.calls += 1
            y = real(flow_a, flow_b)
            torch.cuda.synchronize()
            v = L.check_occlusion_mask(y, L.occlusion_mask_ref(flow_a, flow_b))
            n, _, h, w = y.shape
            b = self.band.setdefault((n, h, w), [0, 0.0])
            b[0], b[1] = b[0] + 1, max(b[1], v["band"])
            # the band condition of the edge cases holds for production masks too: at most 0.5 % of the pixels, none below 200 pixels
            wide = v["band"] > 0.005 or (n * h * w < 200 and v["band"] > 0.0)
            bad = v["flips"] + v["not_binary"] + int(wide)
            self._note(("occlusion_mask", 0, False), dict(ratio=float(bad), ok=bad == 0, worst=(), err=float(v["flips"]), tol=0.0, rms=v["band"]),
                       f"occlusion_mask {tuple(y.shape)}: {v['flips']} flips outside the band, {v['not_binary']} values not 0 / 1, band share {v['band']:.5f}")
            return y
        return fn

    def _postprocess(self, real):
        def fn(x, want_u8=False):
            self.calls += 1
            o32, o8 = real(x, want_u8=want_u8)
            torch.cuda.synchronize()
            r, s = L.postprocess_image_ref(x)
            self._note(("postprocess_image", 0, False), L.check(o32, r, s, o32.dtype), f"postprocess_image {tuple(o32.shape)}")
            if o8 is not None:
                wrong = int((o8 != torch.round(o32 * 255.0).to(torch.uint8).permute(0, 2, 3, 1)).sum())
                self._note(("postprocess_image", "u8", False), dict(ratio=float(wrong), ok=wrong == 0, worst=(), err=float(wrong), tol=0.0, rms=0.0),
                           f"postprocess_image uint8: {wrong} values are not round-half-even(255 o32)")
            return o32, o8
        return fn

    def _gn_ab(self, real):
        def fn(x, gamma, beta, groups, eps, x2=None):
            self.calls += 1
            y = real(x, gamma, beta, groups, eps, x2=x2)
            torch.cuda.synchronize()
            ref, st = L.group_norm_ab_ref(x, gamma, beta, groups, eps, x2=x2)
            path = "gn_part" if getattr(x, "gn_part", None) is not None else "read"
            self._note(("group_norm_ab", path, False), L.check_group_norm_ab(y, ref, st), f"group_norm_ab {tuple(x.shape)} groups={groups}")
            return y
        return fn

    def __exit__(self, *exc):
        self._stack.close()
        self.report()
        return False


class _Patch:
    """minimal monkeypatch: set attributes, restore them on exit (usable outside pytest fixtures)"""

    def __init__(self):
        self._saved = []

    def set(self, obj, name, value):
        self._saved.append((obj, name, getattr(obj, name)))
        setattr(obj, name, value)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for obj, name, v in reversed(self._saved):
            setattr(obj, name, v)
        return False


@contextlib.contextmanager
def capture_routes():
    """Yields a list that receives ops.ConvRoute of every dc_conv_igemm_bf16 launch made inside the block."""
    seen = []
    real = lib.call

    def call(name, *args, meta=None):
        if name == "dc_conv_igemm_bf16":
            seen.append(ops.conv_route(args[0]))
        return real(name, *args, meta=meta)
    lib.call = call
    try:
        yield seen
    finally:
        lib.call = real
