"""ctypes binding of the C-ABI declared in the headers under include/ (`ABI` lists them).

The product path has no CPU fallback: if the shared object is missing or a launcher returns non-zero, this
module raises.  (Loading the library and resolving symbols needs no GPU; launching does.)"""
import ctypes
import os
from ctypes import POINTER, c_double, c_float, c_int, c_longlong, c_void_p

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libdiffcodec_hip.so")

vp, i32, i64, f32, f64 = c_void_p, c_int, c_longlong, c_float, c_double


class ConvDesc(ctypes.Structure):
    """mirror of `dc_conv_desc` (include/diffcodec_hip.h)"""
    _fields_ = [
        ("x1", vp), ("x2", vp), ("w", vp), ("bias", vp), ("gn_ab", vp), ("row_add", vp), ("residual", vp),
        ("out", vp), ("splitk_ws", vp),
        ("N", i32), ("H", i32), ("W", i32), ("C1", i32), ("C2", i32), ("Cout", i32),
        ("ksize", i32), ("stride", i32), ("pad", i32), ("upsample", i32), ("Ho", i32), ("Wo", i32),
        ("gn_silu", i32), ("epilogue", i32), ("out_f32", i32), ("out_scale", f32), ("splitk", i32), ("gn_batch", i32),
        ("act", i32), ("row_add_stride", i64),
        ("ln_stats", vp), ("ln_colsum", vp), ("stats_out", vp), ("gn_part_out", vp),
        ("ln_parts", i32), ("ln_eps", f32), ("ln_scratch", vp),
    ]


# name -> argtypes (every symbol include/diffcodec_hip.h declares; tests/test_abi.py cross-checks every table below with its header)
SIGNATURES = {
    "dc_splat_soft_f32": [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp],
    "dc_splat_sum_f32": [vp, vp, vp, vp, i32, i32, i32, i32, vp],
    "dc_splat_ws_bytes": [i32, i32, i32],
    "dc_splat_norm_f32": [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp],
    "dc_splat_ingrad_f32": [vp, vp, vp, i32, i32, i32, i32, vp],
    "dc_splat_flowgrad_f32": [vp, vp, vp, vp, i32, i32, i32, i32, vp],
    "dc_occlusion_mask_f32": [vp, vp, vp, vp, i32, i32, i32, vp],
    "dc_flow_resize_normalize_f32": [vp, i64, vp, i32, i32, i32, i32, i32, vp],
    "dc_flow_resize_divide_f32": [vp, i64, vp, i32, i32, i32, i32, i32, f32, f32, vp],
    "dc_fuse_warped_f32": [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp],
    "dc_conv3x3_nchw_f32": [vp, i64, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp],
    "dc_conv3x3_f32_route": [i32, i32, i32, i32, i32, POINTER(i32)],
    "dc_nchw_f32_to_nhwc_bf16": [vp, vp, i32, i32, i32, i32, vp],
    "dc_nhwc_bf16_to_nchw_f32": [vp, vp, i32, i32, i32, i32, vp],
    "dc_nhwc_f32_to_nchw_f32": [vp, vp, i32, i32, i32, i32, vp],
    "dc_f32_to_bf16": [vp, vp, i64, vp],
    "dc_conv_igemm_bf16": [POINTER(ConvDesc), vp],
    "dc_conv_route": [POINTER(ConvDesc), POINTER(i32)],
    "dc_conv_instance": [POINTER(ConvDesc), POINTER(i32)],
    "dc_conv_igemm_ws_bytes": [POINTER(ConvDesc)],
    "dc_gemm_row_stats_parts": [i32],
    "dc_conv_gn_part_chunks": [POINTER(ConvDesc)],
    "dc_row_stats_bf16": [vp, vp, i64, i32, vp],
    "dc_ln_finalize": [vp, vp, i64, i32, i32, f32, vp],
    "dc_conv_small_cin_bf16": [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp],
    "dc_conv_small_cout_bf16": [vp, vp, vp, vp, i32, i32, vp, i32, i32, i32, i32, i32, i32, i32, vp],
    "dc_gn_stats_nhwc_bf16": [vp, vp, i32, i64, i32, vp],
    "dc_gn_stats_chunks": [i64, i32],
    "dc_gn_finalize": [vp, i32, i32, vp, i32, i32, vp, vp, vp, i32, i32, i64, f32, vp],
    "dc_gn_direct_nhwc_bf16": [vp, i32, vp, i32, vp, vp, vp, i32, i64, i32, f32, vp],
    "dc_gn_apply_nhwc_bf16": [vp, i32, vp, i32, vp, vp, i32, i64, i32, vp],
    "dc_fdn_modulate_nhwc_bf16": [vp, vp, vp, vp, vp, i32, i32, i64, i32, vp],
    "dc_layernorm_bf16": [vp, vp, vp, vp, i64, i32, f32, vp],
    "dc_attention_bf16": [vp, vp, vp, vp, i32, i32, i32, i32, i32, i64, i64, i64, i64, f32, vp],
    "dc_attention_route": [i32, i32, i32, i32, i32, POINTER(i32)],
    "dc_attention_causal_small_bf16": [vp, vp, vp, vp, i32, i32, i32, i32, i64, i64, i64, i64, f32, vp],
    "dc_embed_tokens_bf16": [vp, vp, vp, vp, i32, i32, i32, i32, vp],
    "dc_softmax_rows_f32_to_bf16": [vp, vp, i64, i32, f32, vp],
    "dc_timestep_embedding_f32": [vp, vp, vp, i32, i32, vp],
    "dc_freeu_lowfreq_nhwc_bf16": [vp, vp, i32, i32, i32, i32, f32, vp],
    "dc_freeu_backbone_nhwc_bf16": [vp, vp, i64, i32, f32, vp],
    "dc_lincomb4_f32": [vp, vp, vp, vp, f32, f32, f32, f32, vp, i64, vp],
    "dc_transpose_bf16": [vp, vp, i32, i32, i32, vp],
    "dc_vae_sample_latents": [vp, vp, vp, f32, i32, i32, i32, i32, vp],
    "dc_silu_f32": [vp, vp, i64, vp],
    "dc_add_bf16": [vp, vp, vp, i64, vp],
    "dc_add_f32": [vp, vp, vp, i64, vp],
    "dc_cfg_ddim_step": [vp, vp, vp, vp, vp, f32, i32, i32, i32, i32, i32, vp],
    "dc_cfg_unipc_step": [vp, vp, vp, vp, vp, vp, vp, vp, f32, i32, i32, i32, i32, i32, vp],
    "dc_latents_to_model_input": [vp, vp, f32, i32, i32, i32, i32, i32, vp],
    "dc_postprocess_image": [vp, vp, vp, i32, i32, i32, i32, i32, vp],
    "dc_flow_hw2_resize_scale_f32": [vp, i32, i32, vp, i32, i32, vp],
    "dc_pack_sixch_u8_f32": [vp, vp, vp, i32, i32, vp],
    "dc_blend_tiles_ramp_u8": [vp, vp, i32, i32, i32, i32, vp, i32, vp, i32, i32, f32, vp],
    "dc_ssim_ws_bytes": [i32, i32, i32, i32, i32, i32],
    "dc_ms_ssim": [vp, vp, i32, POINTER(i64), i32, i32, i32, i32, POINTER(f32), i32, POINTER(f32), i32, f32, f32, f32, vp, vp, vp],
    "dc_ssim": [vp, vp, i32, POINTER(i64), i32, i32, i32, i32, POINTER(f32), i32, f32, f32, f32, i32, vp, vp, vp],
    "dc_psnr_ws_bytes": [i32],
    "dc_psnr": [vp, vp, i32, POINTER(i64), i32, i32, i32, i32, f64, vp, vp, vp],
    "dc_lpips_weight_floats": [],
    "dc_lpips_ws_bytes": [i32, i32, i32],
    "dc_lpips_alex": [vp, vp, i32, POINTER(i64), i32, i32, i32, i32, i32, vp, vp, vp, vp],
    "dc_lpips_features_ws_bytes": [i32, i32, i32],
    "dc_lpips_alex_features": [vp, i32, POINTER(i64), i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp],
    "dc_lpips_conv": [i32, vp, i32, POINTER(i64), i32, i32, i32, i32, vp, vp, vp],
    "dc_fid_weight_floats": [],
    "dc_fid_ws_bytes": [i32, i32, i32],
    "dc_fid_features": [vp, i32, POINTER(i64), i32, i32, i32, vp, vp, vp, vp],
    "dc_fid_maps": [vp, i32, POINTER(i64), i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp],
    "dc_fid_conv": [i32, vp, i32, vp, vp, vp],
    "dc_fid_accumulate": [vp, i32, vp, vp],
    "dc_fvd_weight_floats": [],
    "dc_fvd_ws_bytes": [i32, i32, i32, i32],
    "dc_fvd_features": [vp, i32, i32, POINTER(i64), i32, i32, i32, i32, i32, i32, vp, vp, vp, vp],
    "dc_fvd_endpoints": [vp, i32, i32, POINTER(i64), i32, i32, i32, i32, i32, i32, vp, vp, POINTER(vp), vp, vp],
    "dc_fvd_preprocess": [vp, i32, i32, POINTER(i64), i32, i32, i32, i32, i32, i32, vp, vp],
    "dc_fvd_conv": [vp, i32, i32, i32, i32, i32, i32, i32, vp, i32, i32, vp, i32, i32, vp],
    "dc_fvd_maxpool": [vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp],
    "dc_resample_ws_bytes": [i32, i32, i32, i32],
    "dc_resample_u8": [vp, POINTER(i64), i32, i32, i32, i32, i32, i32, vp, vp, i32, vp, vp, i32, vp, vp, vp],
}

# name -> argtypes of include/diffcodec_flow_hip.h (csrc/cmp.hip)
FLOW_SIGNATURES = {
    "dc_cmp_conv": [vp, i32, POINTER(i64), POINTER(f32), i32, i32, i32, i32, i32, i32, i32, vp, i32, vp, i32, vp, i32, i32, vp],
    "dc_cmp_maxpool": [vp, i32, i32, i32, i32, i32, i32, vp, vp],
    "dc_cmp_avgpool": [vp, i32, i32, i32, i32, vp, i32, i32, vp],
    "dc_cmp_upsample": [vp, i32, i32, i32, i32, i32, i32, vp, i32, i32, vp],
    "dc_cmp_convert_flow": [vp, i32, i32, i32, i32, f32, vp, vp],
    "dc_cmp_sparse_grid": [vp, i32, i32, i32, i32, vp, vp],
    "dc_cmp_head": [vp, i32, i32, i32, i32, vp, i32, f32, vp, vp, vp],
    "dc_cmp_weight_floats": [i32, i32],
    "dc_cmp_ws_bytes": [i32, i32, i32, i32],
    "dc_cmp_forward": [i32, vp, i32, POINTER(i64), vp, i32, i32, i32, i32, f32, vp, vp, vp, vp, vp],
    "dc_cmp_flow": [i32, vp, i32, POINTER(i64), vp, i32, i32, i32, i32, f32, vp, vp, vp, vp],
    "dc_cmp_endpoints": [i32, vp, i32, POINTER(i64), vp, i32, i32, i32, i32, f32, vp, vp, POINTER(vp), vp, vp, vp, vp],
}

# name -> argtypes of include/diffcodec_loss_hip.h (csrc/lpips_grad.hip, csrc/edge_loss.hip)
LOSS_SIGNATURES = {
    "dc_lpips_dgrad_weight_floats": [],
    "dc_lpips_keep_ws_bytes": [i32, i32, i32],
    "dc_lpips_train_ws_bytes": [i32, i32, i32, i32],
    "dc_lpips_alex_keep": [vp, vp, POINTER(i64), i32, i32, i32, i32, vp, vp, vp, vp],
    "dc_lpips_alex_backward": [vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp],
    "dc_lpips_tail_grad": [i32, vp, i32, i32, i32, vp, vp, vp, vp],
    "dc_lpips_conv_dgrad": [i32, vp, i32, i32, i32, vp, vp, vp, vp, vp],
    "dc_lpips_pool_grad": [vp, vp, vp, i32, i32, i32, vp, vp],
    "dc_lpips_conv1_dgrad": [vp, i32, i32, i32, i32, i32, vp, vp, vp, vp],
    "dc_sobel_edge_ws_bytes": [i32, i32, i32, i32],
    "dc_sobel_edge_loss": [vp, vp, POINTER(i64), i32, i32, i32, i32, i32, vp, vp, vp, vp],
    "dc_sobel_edge_grad": [vp, vp, POINTER(i64), i32, i32, i32, i32, i32, vp, i32, f32, vp, vp],
}

# name -> argtypes of include/diffcodec_guide_hip.h (csrc/guide_points.hip)
GUIDE_SIGNATURES = {
    "dc_guide_ws_bytes": [i32, i32, i32],
    "dc_guide_edge": [vp, i32, i32, i32, vp, vp, vp, vp],
    "dc_guide_edt": [vp, i32, i32, i32, vp, vp, vp],
    "dc_guide_nms": [vp, i32, i32, i32, i32, vp, vp, vp],
    "dc_guide_select": [vp, i32, i32, i32, i32, i32, vp, vp, vp, i32, vp],
    "dc_guide_scatter": [vp, i32, i32, i32, i32, vp, vp, i32, vp, vp],
    "dc_guide_watershed": [vp, i32, i32, i32, i32, i32, vp, vp, vp, i32, vp, vp],
}

# name -> argtypes of include/diffcodec_train_hip.h (csrc/conv_f32_grad.hip)
TRAIN_SIGNATURES = {
    "dc_silu_grad_f32": [vp, vp, vp, i64, vp],
    "dc_conv3x3_f32_dgrad": [vp, vp, vp, i32, i32, i32, i32, i32, i32, vp],
    "dc_conv3x3_f32_wgrad_ws_bytes": [i32, i32, i32, i32, i32, i32],
    "dc_conv3x3_f32_wgrad": [vp, i64, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp],
    "dc_conv3x3_f32_grad_route": [i32, i32, i32, i32, i32, i32, i32, POINTER(i32)],
}

# name -> argtypes of include/diffcodec_pyramid_hip.h (csrc/pyramid_grad.hip)
PYRAMID_SIGNATURES = {
    "dc_pyramid_exp_f32": [vp, vp, i64, vp],
    "dc_pyramid_fuse_grad_f32": [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp],
    "dc_pyramid_warp_grad_f32": [vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp],
}

# name -> argtypes of include/diffcodec_fdn_hip.h (csrc/fdn_grad.hip)
FDN_SIGNATURES = {
    "dc_fdn_f32": [vp, vp, i64, vp, i64, vp, vp, vp, i32, i32, i32, i32, f32, vp],
    "dc_fdn_grad_f32": [vp, vp, vp, i64, vp, vp, vp, vp, i64, i32, i32, i32, i32, vp],
}

# the whole C surface: (header under include/, its table), one pair per launcher family.  load() binds what is listed here and
# tests/test_abi.py holds every pair to its header; a new family adds a header, a table and one line here.
ABI = (
    ("diffcodec_hip.h", SIGNATURES),
    ("diffcodec_flow_hip.h", FLOW_SIGNATURES),
    ("diffcodec_loss_hip.h", LOSS_SIGNATURES),
    ("diffcodec_guide_hip.h", GUIDE_SIGNATURES),
    ("diffcodec_train_hip.h", TRAIN_SIGNATURES),
    ("diffcodec_pyramid_hip.h", PYRAMID_SIGNATURES),
    ("diffcodec_fdn_hip.h", FDN_SIGNATURES),
)


def signatures():
    """name -> argtypes over every table of ABI; a name in two tables is an error"""
    out = {}
    for header, table in ABI:
        twice = sorted(set(out) & set(table))
        if twice:
            raise ValueError(f"{twice} of {header} are already in an earlier table of lib.ABI")
        out.update(table)
    return out


def restype_of(name):
    """the C return type by the ABI's naming rule: a byte count is a long long, everything else an int"""
    return c_longlong if name.endswith("_ws_bytes") else c_int


_lib = None


class HipLibraryMissing(RuntimeError):
    pass


def load():
    """Load libdiffcodec_hip.so (built by `python -m diffcodec_amd.build` / __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    path = LIB_PATH                                          # tools/ assign lib.LIB_PATH to A/B another build of the same ABI
    if not os.path.exists(path):
        raise HipLibraryMissing(f"{path} not built: run `python -c 'import __graft_entry__ as g; g.build()'`. "
                                "There is no CPU fallback on the product path.")
    lib = ctypes.CDLL(path)
    for name, args in signatures().items():
        fn = getattr(lib, name)          # AttributeError if the symbol is missing
        fn.argtypes = args
        fn.restype = restype_of(name)
    _lib = lib
    return lib


class HipLaunchError(RuntimeError):
    pass


class LaunchTimer:
    """In-situ per-launch timing for bench.py's roofline leg (never active in a timed region): while `lib.TIMER` is set, every
    C-ABI call is bracketed by two HIP events recorded on the launch stream (torch's current stream — the stream the launcher
    is given), so the elapsed time is the kernel's own duration inside the real step: real operands, real cache state, host
    launch gaps excluded.  `meta` = (family label, shape label, algorithmic FLOPs, algorithmic bytes) from the ops wrapper."""

    def __init__(self):
        self.records = []          # (name, meta, start event, end event)

    def summary(self):
        """{family: dict(calls, ms, flops, bytes, shapes={shape: [calls, ms, flops, bytes]})} — call after a device sync."""
        out = {}
        for name, meta, e0, e1 in self.records:
            fam, shape, fl, by = meta if meta is not None else (name, "", 0.0, 0.0)
            ms = e0.elapsed_time(e1)
            f = out.setdefault(fam, dict(calls=0, ms=0.0, flops=0.0, bytes=0.0, shapes={}))
            f["calls"] += 1
            f["ms"] += ms
            f["flops"] += fl
            f["bytes"] += by
            sh = f["shapes"].setdefault(shape, [0, 0.0, 0.0, 0.0])
            sh[0] += 1
            sh[1] += ms
            sh[2] += fl
            sh[3] += by
        return out


TIMER = None


def call(name, *args, meta=None):
    t = TIMER
    if t is None:
        rc = getattr(load(), name)(*args)
    else:
        import torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = getattr(load(), name)(*args)
        e1.record()
        t.records.append((name, meta, e0, e1))
    if rc != 0:
        raise HipLaunchError(f"{name} returned {rc} ({'invalid argument' if rc == -1 else 'launch failure'})")


def query(name, n_info, *args):
    """Call a routing query (`*_route`, `*_instance`) whose last parameter is an int[n_info] it fills; -> the entries as a tuple.
    Host code only: needs the library, not a GPU.  Raises HipLaunchError for what the launch would refuse."""
    info = (ctypes.c_int * n_info)()
    rc = getattr(load(), name)(*args, info)
    if rc != 0:
        raise HipLaunchError(f"{name} returned {rc} (invalid argument)")
    return tuple(info)
