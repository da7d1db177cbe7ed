"""GOP / tile decode driver: a clip -> decode units -> shard over ranks -> batched decode -> (optional) gather + blend.

What it mirrors in the reference: the per-frame harness of validation.py:85-146 (for every inter frame: its two intra
anchors + its forward / backward flow file -> `load_controls_and_flows` -> `pipe(...)`), the intra/inter split of
uvc_codec_eval.py:19-26 (`get_inter_frames`: every gop_size-th frame is intra) and the data layout both read:

    <root>/<video>/images/frame_%04d.png
    <root>/<video>/optical_flow/optical_flow_gop_<G>_raft/flow_<prev>_<cur>.flo        (forward:  prev anchor -> frame)
    <root>/<video>/optical_flow_bwd/optical_flow_gop_<G>_raft/flow_<next>_<cur>.flo    (backward: next anchor -> frame)

BASELINE configs 3-5 are this driver with different parameters:
    C3  GOP-12, 512x512, unit = inter frame, units round-robin over 8 ranks;
    C4  GOP-4, 960x512 as two 512x512 windows per frame, pipe built with [DualFlowControlNet, ResControlNet] + warp_cond;
    C5  GOP-12, 1080p tiled, 50 steps, unit = (frame, tile) sharded per tile (`shard="tile"`).

Units are independent: there is NO data-path collective.  The only collective here is the optional
gather of decoded units onto one rank (`gather=True`), needed when the tiles of one frame were decoded on different ranks
and must be blended.  What is gathered are the units as uint8 IMAGES (0.79 MB per 512x512 unit, one padded tensor
`dist.gather`, no pickling): the reference's notebook also blends the tiles as the 8-bit images `pipe(...)` returned
(patch_exp.ipynb cell 7), so a unit is quantised before the blend on every path and a sharded decode equals the
single-rank one bit for bit.  Trailing-frame policy: an inter frame needs a closing anchor, so frames after the last intra frame
are not decodable bidirectionally; `sharding.gop_inter_frames` drops them (the reference's `get_inter_frames` merely
counts them for metrics).  `trailing_frames()` reports which frames were dropped."""
import os
from dataclasses import dataclass
from typing import List, Optional, Tuple

import torch

from . import sharding
from .tiled_decode import plan_tiles


@dataclass(frozen=True)
class DecodeUnit:
    uid: int                 # position in the clip's unit list (what `shard_units` deals)
    frame: int               # inter frame index
    prev: int                # previous intra anchor
    next: int                # next intra anchor
    window: Tuple[int, int, int, int]   # (y1, y2, x1, x2) in frame pixels; the whole frame when it is one tile
    tile: int                # index of the window within its frame


def plan_units(num_frames, gop_size, height, width, tile=512, overlap=64) -> List[DecodeUnit]:
    """All decode units of a clip, frame-major: inter frames (uvc_codec_eval.py:19-26) x full-size windows (tiled_decode)."""
    wins = [(0, height, 0, width)] if (height, width) == (tile, tile) else plan_tiles(height, width, tile, overlap)
    units = []
    for f, p, n in sharding.gop_inter_frames(num_frames, gop_size):
        for ti, w in enumerate(wins):
            units.append(DecodeUnit(len(units), f, p, n, tuple(w), ti))
    return units


def trailing_frames(num_frames, gop_size):
    """Inter frames without a closing anchor (dropped; see module docstring)."""
    last_intra = ((num_frames - 1) // gop_size) * gop_size
    return [f for f in range(last_intra + 1, num_frames)]


def shard(units, rank, world, mode="unit"):
    """mode 'unit': round-robin over units (C3, C5 per-patch shard); 'frame': all windows of a frame on one rank, frames
    round-robin (blend without a gather)."""
    if mode == "unit":
        return [units[i] for i in sharding.shard_units(len(units), rank, world)]
    if mode != "frame":
        raise ValueError("mode must be 'unit' or 'frame'")
    frames = sorted({u.frame for u in units})
    mine = {frames[i] for i in sharding.shard_units(len(frames), rank, world)}
    return [u for u in units if u.frame in mine]


class DirectorySource:
    """Controls of one inter frame from the reference's on-disk layout (validation.py:85-93)."""

    def __init__(self, root, video, gop_size, size, device="cuda", flow_dir="optical_flow", flow_bwd_dir="optical_flow_bwd",
                 device_resize=False):
        """device_resize: with a GPU `device`, the PNG bytes are uploaded at their native size and the BICUBIC resize to `size` runs
        on the device (`io_utils._load_rgb_u8_device`): the same bytes without Pillow's pass over every frame on the host."""
        self.root, self.video, self.gop, self.size, self.device = root, video, gop_size, tuple(size), device
        self.flow_dir, self.flow_bwd_dir = flow_dir, flow_bwd_dir
        self.device_resize = device_resize

    def paths(self, frame, prev, nxt):
        base = os.path.join(self.root, self.video)
        sub = f"optical_flow_gop_{self.gop}_raft"
        return (os.path.join(base, "images", f"frame_{prev:04d}.png"), os.path.join(base, "images", f"frame_{nxt:04d}.png"),
                os.path.join(base, self.flow_dir, sub, f"flow_{prev:04d}_{frame:04d}.flo"),
                os.path.join(base, self.flow_bwd_dir, sub, f"flow_{nxt:04d}_{frame:04d}.flo"))

    def controls(self, frame, prev, nxt):
        from .io_utils import load_controls_and_flows
        return load_controls_and_flows(*self.paths(frame, prev, nxt), size=self.size, device=self.device,
                                       device_resize=self.device_resize)

    def ground_truth(self, frame):
        """The original frame <root>/<video>/images/frame_%04d.png as uint8 [H,W,3] on `device`, loaded like the anchors
        (BICUBIC resize to `size`, also Pillow's default behind validation.py:120's `.resize((512, 512))`)."""
        from .io_utils import _load_rgb_u8, _load_rgb_u8_device
        path = os.path.join(self.root, self.video, "images", f"frame_{frame:04d}.png")
        if self.device_resize and torch.device(self.device).type == "cuda":
            return _load_rgb_u8_device(path, self.size, self.device)
        return torch.from_numpy(_load_rgb_u8(path, self.size)).to(self.device)


class SyntheticSource:
    """Seeded synthetic controls of the shapes the reference feeds `pipe(...)`; frame f of every rank
    sees the same tensors, so sharded and unsharded decodes of a clip are comparable."""

    def __init__(self, height, width, device="cuda", seed=1234, with_warp=False):
        self.h, self.w, self.device, self.seed, self.with_warp = height, width, device, seed, with_warp

    def controls(self, frame, prev, nxt):
        from .synthetic import synth_controls
        s = max(self.h, self.w)
        cond, flow = synth_controls(1, s, seed=self.seed + 7919 * frame)
        return cond[:, :, :self.h, :self.w].contiguous().to(self.device), flow[:, :, :self.h, :self.w].contiguous().to(self.device)

    def warp(self, frame):
        g = torch.Generator().manual_seed(self.seed + 104729 * frame + 1)
        return torch.rand(1, 3, self.h, self.w, generator=g).to(self.device)


class ResidentSource:
    """Controls already resident in HBM (bench.py: inputs are on the device when the timed region starts): wraps another
    source and keeps what it returned, per frame."""

    def __init__(self, source, frames_prev_next, noise=None):
        """noise: optional {frame: latents [1,4,H/8,W/8] on the device} (otherwise `frame_noise` draws per call on the host)."""
        self.with_warp = getattr(source, "with_warp", False)
        self._c = {f: source.controls(f, p, n) for f, p, n in frames_prev_next}
        self._w = {f: source.warp(f) for f, _, _ in frames_prev_next} if self.with_warp else {}
        self._n = noise

    def noise(self, frame, height, width, seed):
        return None if self._n is None else self._n[frame]

    def controls(self, frame, prev, nxt):
        return self._c[frame]

    def warp(self, frame):
        return self._w[frame]


def frame_noise(frame, height, width, seed, channels=4):
    """Initial latents of a frame [1,4,H/8,W/8]: a CPU generator seeded per frame (pipeline.py:269-278 draws on the
    generator's device), so the result does not depend on which rank / batch decodes the frame."""
    g = torch.Generator().manual_seed(int(seed) * 1000003 + int(frame))
    return torch.randn((1, channels, height // 8, width // 8), generator=g)


@torch.no_grad()
def decode_units(pipe, units, source, prompt_embeds, negative_prompt_embeds=None, *, batch=16, seed=0, frame_size=None,
                 output="pt", unit_hw=(512, 512), **pipe_kwargs):
    """Decode `units` (this rank's share) `batch` at a time.  Returns fp32 [len(units), 3, th, tw] in [0,1] on the device
    (output='pt') or the latents (output='latent').  Controls of a frame are loaded once and cropped per window; flows keep
    frame units (patch_exp.ipynb does not re-base them).  An empty share (more ranks than units) returns an empty tensor
    of the same trailing shape, so callers can concatenate / gather rank outputs without a special case."""
    if not units:
        th, tw = unit_hw
        shape = (0, 4, th // 8, tw // 8) if output == "latent" else (0, 3, th, tw)
        return torch.empty(shape, device=pipe.device, dtype=torch.float32)
    for name, t in (("prompt_embeds", prompt_embeds), ("negative_prompt_embeds", negative_prompt_embeds)):
        if t is not None and t.shape[0] != 1 and t.shape[0] < min(batch, len(units)):
            raise ValueError(f"{name} has batch {t.shape[0]}: pass one row (shared by every unit) or at least one per unit "
                             f"of a chunk ({min(batch, len(units))})")
    cache = {}

    def frame_inputs(u):
        if u.frame not in cache:
            cache.clear()                                # units are frame-major: one frame's controls live at a time
            cond, flow = source.controls(u.frame, u.prev, u.next)
            h, w = (cond.shape[-2], cond.shape[-1]) if frame_size is None else frame_size
            warp = source.warp(u.frame) if getattr(source, "with_warp", False) else None
            nz = source.noise(u.frame, h, w, seed) if hasattr(source, "noise") else None
            cache[u.frame] = (cond, flow, frame_noise(u.frame, h, w, seed) if nz is None else nz, warp)
        return cache[u.frame]

    outs = []
    for i in range(0, len(units), batch):
        chunk = units[i:i + batch]
        cc, fc, lt, wc = [], [], [], []
        for u in chunk:
            cond, flow, noise, warp = frame_inputs(u)
            y1, y2, x1, x2 = u.window
            cc.append(cond[:, :, y1:y2, x1:x2])
            fc.append(flow[:, :, y1:y2, x1:x2])
            lt.append(noise[:, :, y1 // 8:y2 // 8, x1 // 8:x2 // 8])
            if warp is not None:
                wc.append(warp[:, :, y1:y2, x1:x2])
        n = len(chunk)
        pe = prompt_embeds.expand(n, -1, -1).contiguous() if prompt_embeds.shape[0] == 1 else prompt_embeds[:n]
        npe = None if negative_prompt_embeds is None else (
            negative_prompt_embeds.expand(n, -1, -1).contiguous() if negative_prompt_embeds.shape[0] == 1 else negative_prompt_embeds[:n])
        extra = dict(warp_cond=torch.cat(wc, 0).contiguous()) if wc else {}
        res = pipe(prompt_embeds=pe, negative_prompt_embeds=npe, controlnet_cond=torch.cat(cc, 0).contiguous(),
                   flow_cond=torch.cat(fc, 0).contiguous(), latents=torch.cat(lt, 0).contiguous(),
                   output_type="latent" if output == "latent" else "pt", **extra, **pipe_kwargs).images
        outs.append(res.float())
    return torch.cat(outs, 0).contiguous()


def units_to_u8(images):
    """fp32 unit images [n,3,th,tw] in [0,1] -> uint8 [n,th,tw,3]: `image_processor.postprocess(output_type='pil')`'s
    quantisation (pipeline.py:397-398: x * 255, round, uint8), applied to the tensor on whatever device it lives."""
    return (images.permute(0, 2, 3, 1) * 255.0).round().clamp(0, 255).to(torch.uint8).contiguous()


def gather_units(local_u8, units, rank=None, world=None, mode="unit", dst=0):
    """Collect this rank's uint8 unit images [n_local, th, tw, 3] on `dst` as [len(units), th, tw, 3] in unit order.  Every
    rank can list every other rank's share (`shard` is a pure function), so only pixels travel: ONE `dist.gather` of
    tensors padded to the largest share — device tensors over RCCL, host tensors over gloo (which gathers on the CPU
    only).  Returns None on the other ranks."""
    import torch.distributed as dist
    ini = dist.is_available() and dist.is_initialized()
    if rank is None or world is None:
        rank, world = (dist.get_rank(), dist.get_world_size()) if ini else (0, 1)
    shares = [[u.uid for u in shard(units, r, world, mode)] for r in range(world)]
    if local_u8.dtype != torch.uint8 or local_u8.shape[0] != len(shares[rank]):
        raise ValueError("gather_units takes this rank's uint8 unit images, one per unit of its share")
    if world == 1 or not ini:
        out = torch.empty((len(units),) + tuple(local_u8.shape[1:]), dtype=torch.uint8, device=local_u8.device)
        out[shares[rank]] = local_u8
        return out
    send = local_u8 if dist.get_backend() != "gloo" else local_u8.cpu()
    per = max(len(s_) for s_ in shares)
    pad = torch.zeros((per,) + tuple(send.shape[1:]), dtype=torch.uint8, device=send.device)
    pad[:send.shape[0]] = send
    bufs = [torch.empty_like(pad) for _ in range(world)] if rank == dst else None
    dist.gather(pad, bufs, dst=dst)
    if rank != dst:
        return None
    out = torch.empty((len(units),) + tuple(pad.shape[1:]), dtype=torch.uint8, device=pad.device)
    for r in range(world):
        if shares[r]:
            out[shares[r]] = bufs[r][:len(shares[r])]
    return out


def _blend_frame_tensors(unit_u8, units, height, width, overlap=64):
    """blend_frames before the host copy: {frame: uint8 [H,W,3] tensor on the device of `unit_u8`} (decode_clip scores these)."""
    from . import ops, tiling
    if unit_u8.dtype != torch.uint8:
        raise ValueError("blend_frames takes uint8 unit images (units_to_u8)")
    frames = {}
    by_frame = {}
    for k, u in enumerate(units):
        by_frame.setdefault(u.frame, []).append((u.tile, k, u.window))
    for f, lst in by_frame.items():
        lst.sort()
        idx = [k for _, k, _ in lst]
        coords = [w for _, _, w in lst]
        tiles = unit_u8[idx]
        if len(lst) == 1 and coords[0] == (0, height, 0, width):
            frames[f] = tiles[0]
        elif tiles.is_cuda:
            frames[f] = ops.blend_tiles_ramp(tiles.permute(0, 3, 1, 2).float().contiguous(), coords, (height, width), overlap,
                                             scale=1.0)
        else:
            frames[f] = torch.from_numpy(tiling.merge_ramp([t.numpy() for t in tiles], coords, (height, width), order="hwc",
                                                           feather=overlap))
    return frames


def blend_frames(unit_u8, units, height, width, overlap=64):
    """uint8 unit images [n,th,tw,3] of COMPLETE frames -> {frame: uint8 [H,W,3]} (device blend kernel when the tensor
    lives on the GPU, `tiling.merge_ramp` on the host otherwise; both blend the 8-bit tiles in fp32 with the same op
    order, so the two are bit-identical)."""
    return {f: t.cpu().numpy() for f, t in _blend_frame_tensors(unit_u8, units, height, width, overlap).items()}


def _to_score_size(x, score_size):
    """uint8 [..., H, W, 3] -> the operand the scores see: resized as test_utils.py:17-21 resizes its PIL frames (Pillow's
    antialiased BILINEAR, on the device, the same bytes) when `score_size` is given and differs from (H, W); `x` itself otherwise."""
    if score_size is None or tuple(x.shape[-3:-1]) == tuple(score_size):
        return x
    from .resample import resize_u8
    return resize_u8(x.reshape((-1,) + tuple(x.shape[-3:])), score_size, "bilinear").reshape(tuple(x.shape[:-3]) + tuple(score_size) + (x.shape[-1],))


def _score_frames(frames, source, lpips=None, fid=None, score_size=None):
    """(scores, {frame: (decoded [64], truth [64])} fp32 FID feature rows on the host, empty without `fid`, {frame: ground truth on
    the frame's device, at the frame's size})"""
    from . import metrics
    scores, rows, truth = {}, {}, {}
    for f, pred in sorted(frames.items()):
        gt = source.ground_truth(f).to(pred.device)
        if gt.shape != pred.shape:
            raise ValueError(f"ground truth of frame {f} has shape {tuple(gt.shape)}, the decoded frame {tuple(pred.shape)}")
        truth[f] = gt
        x, y = _to_score_size(pred.unsqueeze(0), score_size), _to_score_size(gt.unsqueeze(0), score_size)
        scores[f] = dict(psnr=float(metrics.psnr(x, y, data_range=255.0)[0]), ms_ssim=float(metrics.ms_ssim(x, y, data_range=255)))
        if lpips is not None:
            scores[f]["lpips"] = float(lpips(x, y, normalize=False).reshape(-1)[0])
        if fid is not None and not scores[f]["psnr"] > 1000:
            r = fid.features(torch.cat([x, y])).cpu()
            rows[f] = (r[0], r[1])
    return scores, rows, truth


def fid_update_rows(fid, rows):
    """Add {frame: (decoded [64], truth [64])} to `fid` in ascending frame order: decoded rows to the fake side, truth rows to the
    real side.  The state depends on the rows and their order only, not on which rank computed them."""
    order = sorted(rows)
    if order:
        fid.update_features(torch.stack([rows[f][0] for f in order]), real=False)
        fid.update_features(torch.stack([rows[f][1] for f in order]), real=True)


def _fid_value(fid):
    real, fake = fid.state()
    return fid.compute() if min(float(real[0]), float(fake[0])) >= 2 else float("nan")


def fvd_of_frames(fvd, frames, truth, scores, score_size=None):
    """The clip's FVD as test_utils.py:45-70 forms it: the decoded video is the scored frames in ascending order (frames whose PSNR
    exceeds 1000 dB left out, as for FID), the truth video the same frames of ground truth; each is ONE video, which the reference
    stacks twice (`repeat(2, ...)`, test_utils.py:69-70).  The features are computed once and the row is added twice: with two
    identical rows the covariance is exactly zero and the value is |f_decoded - f_truth|^2.  NaN with fewer than 9 such frames.
    `fvd` (a `metrics.FrechetVideoDistance` with weights loaded) is reset first.  `score_size`: the two stacked videos are resized
    to it first (`score_frames`)."""
    from . import metrics
    keep = [f for f in sorted(frames) if not scores[f]["psnr"] > 1000]
    fvd.reset()
    if len(keep) < metrics.FVD_MIN_FRAMES:
        return float("nan")
    rows = fvd.features(_to_score_size(torch.stack([torch.stack([frames[f] for f in keep]), torch.stack([truth[f] for f in keep])]),
                                       score_size))
    fvd.update_features(rows[0:1].expand(2, -1), real=False)
    fvd.update_features(rows[1:2].expand(2, -1), real=True)
    return fvd.compute()


def score_frames(frames, source, lpips=None, fid=None, score_size=None):
    """{frame: uint8 [H,W,3] tensor} -> {frame: {"psnr": dB, "ms_ssim": value}} against `source.ground_truth(frame)`, with L = 255
    (test_utils.py:23-24, :55; validation.py:147-150 on x / 255 gives the same values), on the device of the frames.
    `lpips` (a `metrics.LPIPS` with weights loaded) adds "lpips": as test_utils.py:58 computes it, on frame / 255 with
    normalize=False.  That is the reference's quirk, kept for comparable numbers: it feeds [0,1] images where the net expects
    [-1,1] (the library's `normalize=True` would map them).
    `fid` (a `metrics.FrechetInceptionDistance` with weights loaded) is updated with every frame (fake side) and its ground truth
    (real side) in ascending frame order, as test_utils.py:62-63 does; it is not reset here, `fid.compute()` gives the value.  FID is
    a statistic of the set, so the per-frame dicts do not change.  test_utils.py:51-52 `continue`s past identical frames before the
    update: a frame whose PSNR exceeds 1000 dB is left out.
    `score_size=(h, w)`: every frame and its ground truth are first resized to it on the device (`resample.resize_u8`, "bilinear":
    the bytes of the reference's `transforms.Resize((512, 512))` on its PIL frames, test_utils.py:17-21, :45-46) and all scores,
    the PSNR behind the 1000 dB rule and the FID rows come from the resized pair; a frame already of that size is scored as it is.
    The ground truth must still have the decoded frame's shape.  None scores the frames at their own size."""
    scores, rows, _ = _score_frames(frames, source, lpips, fid, score_size)
    if fid is not None:
        fid_update_rows(fid, rows)
    return scores


def gather_scores(scores, units, rank, world, dst=0, lpips=False):
    """Every rank's {frame: {"psnr", "ms_ssim"[, "lpips"]}} -> the union on `dst` (None elsewhere): ONE `dist.gather` of a float64
    [inter frames, 3] tensor (scored flag, PSNR, MS-SSIM) per rank, with a fourth column (LPIPS) when `lpips` is set (every rank
    passes the same value); no pixels travel."""
    import torch.distributed as dist
    frames = sorted({u.frame for u in units})
    row = {f: i for i, f in enumerate(frames)}
    dev = "cpu" if dist.get_backend() == "gloo" else torch.device("cuda", torch.cuda.current_device())
    keys = ("psnr", "ms_ssim", "lpips") if lpips else ("psnr", "ms_ssim")
    send = torch.zeros((len(frames), 1 + len(keys)), dtype=torch.float64)
    for f, s in scores.items():
        send[row[f]] = torch.tensor([1.0] + [s[k] for k in keys], dtype=torch.float64)
    send = send.to(dev)
    bufs = [torch.empty_like(send) for _ in range(world)] if rank == dst else None
    dist.gather(send, bufs, dst=dst)
    if rank != dst:
        return None
    out = {}
    for b in bufs:
        for f, (have, *vals) in zip(frames, b.cpu().tolist()):
            if have:
                out[f] = dict(zip(keys, vals))
    return dict(sorted(out.items()))


def gather_fid_rows(rows, units, rank, world, dst=0):
    """Every rank's {frame: (decoded [64], truth [64])} -> the union on `dst` (None elsewhere): ONE `dist.gather` of a float64
    [inter frames, 1 + 128] tensor (flag, decoded row, truth row) per rank, shaped like `gather_scores`.  The rows travel, not the
    sums: `dst` accumulates them in frame order, so the value has the bits of a single-rank run (fp32 -> fp64 -> fp32 is exact)."""
    import torch.distributed as dist
    frames = sorted({u.frame for u in units})
    row = {f: i for i, f in enumerate(frames)}
    dev = "cpu" if dist.get_backend() == "gloo" else torch.device("cuda", torch.cuda.current_device())
    send = torch.zeros((len(frames), 129), dtype=torch.float64)
    for f, (d, t) in rows.items():
        send[row[f], 0] = 1.0
        send[row[f], 1:65] = d.double()
        send[row[f], 65:] = t.double()
    send = send.to(dev)
    bufs = [torch.empty_like(send) for _ in range(world)] if rank == dst else None
    dist.gather(send, bufs, dst=dst)
    if rank != dst:
        return None
    out = {}
    for b in bufs:
        b = b.cpu()
        for i, f in enumerate(frames):
            if b[i, 0]:
                out[f] = (b[i, 1:65].float(), b[i, 65:].float())
    return dict(sorted(out.items()))


@torch.no_grad()
def decode_clip(pipe, source, num_frames, gop_size, height, width, prompt_embeds, negative_prompt_embeds=None, *, tile=512,
                overlap=64, batch=16, seed=0, rank=None, world=None, shard_mode="unit", gather=True, score=False, lpips=None,
                fid=None, fvd=None, score_size=None, **pipe_kwargs):
    """Whole pipeline for one clip on this rank.  Returns dict(units=all units, mine=this rank's, images=this rank's fp32 unit
    images, frames={frame: uint8 HxWx3} on the gathering rank (or for locally complete frames when gather=False)).
    score=True adds scores={frame: {"psnr": dB, "ms_ssim": value}}: each blended frame against `source.ground_truth(frame)` on
    the device, from the uint8 frames `frames` holds (score_frames); `lpips=` (a `metrics.LPIPS` with weights loaded) adds "lpips"
    to each frame's dict and a fourth column to the gather.  With gather=False and world > 1 every rank scores its
    complete frames and one gather of the scores (not the pixels) gives rank 0 all of them; other ranks keep their own.
    `fid=` (a `metrics.FrechetInceptionDistance` with weights loaded) leaves the per-frame dicts as they are and adds
    fid_features={frame: (decoded [64], truth [64])} (fp32 rows on the host; frames whose PSNR exceeds 1000 dB are left out, as
    test_utils.py:51-52 skips them) and, on the rank that holds the scores, fid = the value (NaN with fewer than two frames): the
    model is reset, then updated in ascending frame order.  With gather=False and world > 1 one more gather brings the feature rows
    (not the sums) to rank 0, which accumulates them in frame order: the value has the bits of a single-rank run.
    `fvd=` (a `metrics.FrechetVideoDistance` with weights loaded) adds fvd = the clip's FVD on the rank that holds the scores
    (`fvd_of_frames`: the scored frames as one decoded and one truth video, each row added twice; NaN with fewer than 9 scored
    frames).  With gather=False and world > 1 no rank holds the whole video: ValueError, raised before anything is decoded.
    `score_size=(h, w)`: the reference first resizes its PIL frames to 512 x 512 (test_utils.py:17-21); with score_size=(512, 512)
    every decoded frame and its ground truth are resized the same way on the device before all five scores (`score_frames`; the
    stacked videos for FVD), fid_features come from the resized frames and `frames` stay at the decode size.  None (the default)
    scores at the decode size, which is the same thing for a 512 x 512 decode.  With lpips=, fid=, fvd= and score_size=(512, 512)
    one call returns the reference's five numbers for a decode of any size."""
    if rank is None or world is None:
        ini = torch.distributed.is_available() and torch.distributed.is_initialized()
        rank = torch.distributed.get_rank() if ini else 0
        world = torch.distributed.get_world_size() if ini else 1
    have_fvd = score and fvd is not None
    if have_fvd and not gather and world > 1:
        raise ValueError("fvd= scores the clip as one video: with gather=False and world > 1 no rank holds all its frames")
    units = plan_units(num_frames, gop_size, height, width, tile, overlap)
    mine = shard(units, rank, world, shard_mode)
    unit_hw = (min(height, tile), min(width, tile))            # a frame smaller than the tile is one frame-sized unit (ranks with an empty
    #                                                            share must pad their gather buffers to the SAME unit size as the others)
    images = decode_units(pipe, mine, source, prompt_embeds, negative_prompt_embeds, batch=batch, seed=seed,
                          frame_size=(height, width), unit_hw=unit_hw, **pipe_kwargs)
    u8 = units_to_u8(images)
    frames = None
    scores = None
    rows = {}
    have_fid = score and fid is not None
    if have_fid:
        fid.reset()
    holds_scores = rank == 0 or not (gather and world > 1)      # whether this rank's result carries the clip's (or its own) scores

    fvd_value = None

    def blend(unit_u8, us):
        nonlocal scores, rows, fvd_value
        dev = _blend_frame_tensors(unit_u8, us, height, width, overlap)
        if score:
            scores, rows, truth = _score_frames(dev, source, lpips, fid, score_size)
            if have_fvd:
                fvd_value = fvd_of_frames(fvd, dev, truth, scores, score_size)
        return {f: t.cpu().numpy() for f, t in dev.items()}

    if gather and world > 1:
        allimg = gather_units(u8, units, rank, world, shard_mode, dst=0)
        if rank == 0:
            frames = blend(allimg, units)
    else:
        per_frame = {}
        for u in units:
            per_frame[u.frame] = per_frame.get(u.frame, 0) + 1
        have = {}
        for u in mine:
            have[u.frame] = have.get(u.frame, 0) + 1
        complete = [k for k, u in enumerate(mine) if have[u.frame] == per_frame[u.frame]]
        if complete:
            frames = blend(u8[complete], [mine[k] for k in complete])
        if score and world > 1 and torch.distributed.is_available() and torch.distributed.is_initialized():
            merged = gather_scores(scores or {}, units, rank, world, dst=0, lpips=lpips is not None)
            if have_fid:
                allrows = gather_fid_rows(rows, units, rank, world, dst=0)
                holds_scores = rank == 0
            if rank == 0:
                scores = merged
                if have_fid:
                    rows = allrows
    out = dict(units=units, mine=mine, images=images, frames=frames)
    if score:
        out["scores"] = scores if scores is not None else {}
    if have_fid:
        out["fid_features"] = rows
        if holds_scores:
            fid_update_rows(fid, rows)
            out["fid"] = _fid_value(fid)
    if have_fvd and holds_scores:
        out["fvd"] = fvd_value if fvd_value is not None else float("nan")
    return out
