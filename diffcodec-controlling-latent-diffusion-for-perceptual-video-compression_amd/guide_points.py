"""Guide points for the CMP network on the GPU: the 'watershed' strategy of the reference's flow_sampler
(cmp/utils/data_utils.py), alone or united with its 'grid' strategy, on csrc/guide_points.hip.

    sparse = sample_watershed(flow, nms_ks=15, stride=80)     # flow_sampler(flow, ['grid', 'watershed'], 1 / 6400, 15)
    counts, points = watershed_points(flow, nms_ks=15)         # the watershed points themselves

A guide point sits in the middle of every region of coherent motion: the flow is subsampled to below 800 pixels a side, its Sobel
magnitude thresholded into an edge map, and the local maxima of the exact distance to the nearest edge are thinned so that no two
lie within (nms_ks - 1) / 2 pixels of each other on both axes.  Where the reference draws a coin to decide which point of a close
pair goes, the later one in row-major order goes here, so the result is a function of the flow alone.  Everything after the
threshold is integer arithmetic; the calls only enqueue kernels (no host synchronisation) and can be captured into a graph.
There is no CPU path: without the built library or a GPU the calls raise."""
import math

import torch

from . import lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def working_size(H, W):
    """(ds, h, w): the subsampling step of flow_sampler and the size of flow[::ds, ::ds]"""
    ds = max(1, max(int(H), int(W)) // 400)
    return ds, -(-int(H) // ds), -(-int(W) // ds)


def max_points(h, w, nms_ks):
    """The most watershed points an h x w working image can keep: one per (nms_ks - 1) / 2 tile"""
    d = (int(nms_ks) - 1) // 2
    return -(-h // d) * -(-w // d)


def stride_from_bg_ratio(bg_ratio):
    """The 'grid' stride flow_sampler derives from its bg_ratio"""
    if not 0 < bg_ratio <= 1:
        raise ValueError(f"bg_ratio {bg_ratio} is not in (0, 1]")
    return int(math.sqrt(1.0 / bg_ratio))


def _check(flow, nms_ks, stride, max_num_guide):
    if flow.dim() != 4 or flow.shape[1] != 2 or flow.dtype != torch.float32:
        raise ValueError(f"flow is fp32 [N,2,H,W], got {flow.dtype} {tuple(flow.shape)}")
    if int(nms_ks) != nms_ks or int(nms_ks) < 3 or int(nms_ks) % 2 == 0:
        raise ValueError(f"nms_ks {nms_ks}: an odd window of at least 3")
    if stride is not None and int(stride) < 1:
        raise ValueError(f"stride {stride}")
    if max_num_guide != -1:
        raise ValueError("max_num_guide keeps a random subset of the points; only -1 (all of them) is built")
    if flow.device.type != "cuda":
        raise RuntimeError("the guide points are picked on the GPU only: flow must be on a cuda device")


def workspace(flow):
    N, _, H, W = flow.shape
    nbytes = lib.load().dc_guide_ws_bytes(N, H, W)
    if nbytes < 0:
        raise ValueError(f"dc_guide_ws_bytes refuses {N} x {H} x {W}")
    return torch.empty(nbytes, dtype=torch.uint8, device=flow.device)


def _watershed(flow, nms_ks, stride, want_sparse):
    flow = flow.contiguous()
    N, _, H, W = flow.shape
    _, h, w = working_size(H, W)
    cap = max_points(h, w, nms_ks)
    ws = workspace(flow)
    counts = torch.empty(N, dtype=torch.int32, device=flow.device)
    points = torch.empty(N, cap, 2, dtype=torch.int32, device=flow.device)
    sparse = torch.empty(N, 4, H, W, dtype=torch.float32, device=flow.device) if want_sparse else None
    lib.call("dc_guide_watershed", flow.data_ptr(), N, H, W, int(nms_ks), 0 if stride is None else int(stride), ws.data_ptr(),
             counts.data_ptr(), points.data_ptr(), cap, None if sparse is None else sparse.data_ptr(), _stream())
    return counts, points, sparse


def sample_watershed(flow, nms_ks=15, stride=None, max_num_guide=-1):
    """Dense flow [N,2,H,W] (fp32, on the GPU) -> the sparse operand [N,4,H,W] holding (u, v, 1, 1) at the 'watershed' guide
    points and, with a `stride`, at the 'grid' points of `sample_grid` as well; 0 elsewhere."""
    _check(flow, nms_ks, stride, max_num_guide)
    return _watershed(flow, nms_ks, stride, True)[2]


def watershed_points(flow, nms_ks=15, max_num_guide=-1):
    """-> (counts [N] int32, points [N,cap,2] int32): the watershed points of each flow as (y, x) in full-resolution pixels in
    row-major order, -1 past the first counts[n]; cap = max_points(h, w, nms_ks) of the working size."""
    _check(flow, nms_ks, None, max_num_guide)
    counts, points, _ = _watershed(flow, nms_ks, None, False)
    return counts, points
