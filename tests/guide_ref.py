"""Restatement, in numpy and torch only, of the 'watershed' strategy of the reference's flow_sampler (cmp/utils/data_utils.py:
get_edge, distance_transform_edt, nms, remove_border, neighbor_elim) and of its union with the 'grid' strategy: what
csrc/guide_points.hip is held to.  No scipy: squared distances are exhaustive minima in int64, the NMS window is clipped to the
image (scipy's 'reflect' boundary only repeats values from inside it), and the comparisons are made on squared distances (sqrt is
monotone).  tests/test_guide_ref.py pins all of it to tests/golden/guide_points.npz, recorded from the reference itself.

The synthetic flows of the golden (overlapping moving discs on a gradient) are rebuilt here from their parameters."""
import numpy as np
import torch
import torch.nn.functional as F

NO_EDGE = 1 << 29                 # d2 of an image without an edge pixel (dc_guide_edt)


def working_ds(H, W):
    return max(1, max(H, W) // 400)


def synth_params(seed, H, W, discs=5):
    """[discs + 1][6] float64: row 0 the background (u0, ux, uy, v0, vx, vy), then (cx, cy, radius, du, dv, 0) per disc; a row
    (x0, 0, width, du, dv, 1) is the vertical band x0 <= x < x0 + width instead"""
    rng = np.random.RandomState(seed)
    p = np.zeros((discs + 1, 6))
    p[0] = rng.uniform(-1.0, 1.0, 6)
    for k in range(1, discs + 1):
        p[k, :5] = (rng.uniform(0, W), rng.uniform(0, H), rng.uniform(0.08, 0.3) * min(H, W), rng.uniform(-12, 12), rng.uniform(-12, 12))
    return p


def synth_flow(params, H, W):
    """float32 [H,W,2]: a linear background, then each disc painted over what is below it (+, *, <= only: the same bits anywhere)"""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    b = params[0]
    u = b[0] + b[1] * (x / W) + b[2] * (y / H)
    v = b[3] + b[4] * (x / W) + b[5] * (y / H)
    for cx, cy, r, du, dv, band in params[1:]:
        inside = ((x >= cx) & (x < cx + r)) if band else ((x - cx) * (x - cx) + (y - cy) * (y - cy) <= r * r)
        u = np.where(inside, du, u)
        v = np.where(inside, dv, v)
    return np.stack([u, v], 2).astype(np.float32)


def to_nchw(flow_hw2):
    return torch.from_numpy(np.ascontiguousarray(flow_hw2.transpose(2, 0, 1)))[None]


# ------------------------------------------------------------------------------------------------ stage 1
def edge_magnitude(flow, dtype=torch.float64):
    """flow [N,2,H,W] -> the normalised edge magnitude [N,h,w] in `dtype`, in the device's operation order"""
    ds = working_ds(flow.shape[2], flow.shape[3])
    p = F.pad(flow[:, :, ::ds, ::ds].to(dtype), (1, 1, 1, 1), mode="replicate")
    a00, a01, a02 = p[..., :-2, :-2], p[..., :-2, 1:-1], p[..., :-2, 2:]
    a10, a12 = p[..., 1:-1, :-2], p[..., 1:-1, 2:]
    a20, a21, a22 = p[..., 2:, :-2], p[..., 2:, 1:-1], p[..., 2:, 2:]
    ex = ((a00 - a02) + 2 * (a10 - a12)) + (a20 - a22)
    ey = ((a00 - a20) + 2 * (a01 - a21)) + (a02 - a22)
    s = torch.sqrt(ex * ex + ey * ey)
    s = s[:, 0] + s[:, 1]
    peak = s.amax(dim=(1, 2), keepdim=True)
    return s / torch.maximum(peak, torch.tensor(0.01, dtype=dtype))


def edge_map(norm):
    return norm > torch.tensor(0.1, dtype=norm.dtype)


# ------------------------------------------------------------------------------------------------ stage 2
def sqdist(edge):
    """edge [h,w] (bool) -> int64 [h,w]: the squared distance to the nearest edge pixel, every pair of rows and columns tried"""
    edge = np.asarray(edge).astype(bool)
    h, w = edge.shape
    if not edge.any():
        return np.full((h, w), NO_EDGE, dtype=np.int64)
    big = np.int64(1) << 40
    xs = np.arange(w, dtype=np.int64)
    dx2 = (xs[:, None] - xs[None, :]) ** 2
    row = np.full((h, w), big, dtype=np.int64)                          # row[y'][x] = min over the edge pixels x' of row y'
    for y in range(h):
        cols = np.nonzero(edge[y])[0]
        if cols.size:
            row[y] = dx2[:, cols].min(1)
    ys = np.arange(h, dtype=np.int64)
    out = np.empty((h, w), dtype=np.int64)
    for y in range(h):
        out[y] = (((ys - y) ** 2)[:, None] + row).min(0)
    return out


# ------------------------------------------------------------------------------------------------ stage 3
def window_max(a, ks):
    """the maximum over the ks x ks window clipped to the image"""
    r = (ks - 1) // 2
    h, w = a.shape
    rows = a.copy()
    for o in range(1, min(r, w - 1) + 1):
        rows[:, o:] = np.maximum(rows[:, o:], a[:, :-o])
        rows[:, :-o] = np.maximum(rows[:, :-o], a[:, o:])
    out = rows.copy()
    for o in range(1, min(r, h - 1) + 1):
        out[o:] = np.maximum(out[o:], rows[:-o])
        out[:-o] = np.maximum(out[:-o], rows[o:])
    return out


def candidates(d2, ks):
    """bool [h,w]: nms(...) > 0 after remove_border; none where the image has no edge pixel"""
    assert ks % 2 == 1 and ks >= 3
    d2 = np.asarray(d2).astype(np.int64)
    c = (d2 >= window_max(d2, ks)) & (d2 > 0) & (d2 < NO_EDGE)
    c[0, :] = c[-1, :] = False
    c[:, 0] = c[:, -1] = False
    return c


# ------------------------------------------------------------------------------------------------ stage 4
def neighbor_elim(ys, xs, d, coin=None):
    """The reference's pair-visiting order: every ordered pair (i, j) inside the box, by i then j.  coin(): a draw above 0.5 removes
    i, otherwise j, drawn only for a pair that is still whole (the reference's np.random.rand); None: the later point of the pair
    goes.  -> the surviving (ys, xs)"""
    ys, xs = np.asarray(ys), np.asarray(xs)
    valid = np.ones(len(ys), dtype=bool)
    near = (np.abs(ys[:, None] - ys[None, :]) < d) & (np.abs(xs[:, None] - xs[None, :]) < d)
    for i, j in zip(*np.nonzero(near)):
        if valid[i] and valid[j] and i != j:
            if coin is None:
                valid[max(i, j)] = False
            elif coin() > 0.5:
                valid[i] = False
            else:
                valid[j] = False
    return ys[valid], xs[valid]


def greedy(ys, xs, d):
    """The deterministic rule stated directly: in row-major order, a candidate survives iff no earlier survivor is inside its box"""
    keep_y, keep_x = [], []
    for y, x in zip(np.asarray(ys).tolist(), np.asarray(xs).tolist()):
        if not keep_y or not ((np.abs(np.array(keep_y) - y) < d) & (np.abs(np.array(keep_x) - x) < d)).any():
            keep_y.append(y)
            keep_x.append(x)
    return np.array(keep_y, dtype=np.int64), np.array(keep_x, dtype=np.int64)


# ------------------------------------------------------------------------------------------------ the path
def grid_points(H, W, stride):
    y0, x0 = int((H - H // stride * stride) / 2), int((W - W // stride * stride) / 2)
    return np.arange(y0, H, stride), np.arange(x0, W, stride)


def watershed(flow, ks, coin=None, dtype=torch.float32, big=False):
    """flow [2,H,W] (torch) -> (candidate mask [h,w], surviving ys, xs in working pixels, ds); `big`: the direct rule instead of
    the reference's pair matrix (the same set, without its K x K memory)"""
    H, W = flow.shape[1:]
    edge = edge_map(edge_magnitude(flow[None], dtype))[0].numpy()
    cand = candidates(sqdist(edge), ks)
    ys, xs = np.nonzero(cand)
    ys, xs = greedy(ys, xs, (ks - 1) / 2) if big else neighbor_elim(ys, xs, (ks - 1) / 2, coin)
    return cand, ys, xs, working_ds(H, W)


def final_mask(flow, ks, stride, coin=None, big=False):
    """bool [H,W]: flow_sampler(strategy=['grid', 'watershed'])'s mask (stride None: 'watershed' alone)"""
    H, W = flow.shape[1:]
    _, ys, xs, ds = watershed(flow, ks, coin, big=big)
    m = np.zeros((H, W), dtype=bool)
    if stride is not None:
        gy, gx = grid_points(H, W, stride)
        m[np.ix_(gy, gx)] = True
    m[ys * ds, xs * ds] = True
    return m


def sparse_of(flow, mask):
    """flow [2,H,W], mask bool [H,W] -> the sparse operand [4,H,W] fp32"""
    m = torch.from_numpy(mask)
    return torch.cat([torch.where(m, flow.float(), torch.zeros(())), m[None].float(), m[None].float()], 0)


# ------------------------------------------------------------------------------------------------ the golden
def load_golden(path):
    """{name: dict(H, W, ks, stride, seed, params, edge [h,w], cand [h,w], mask [H,W])} of tests/golden/guide_points.npz"""
    z = np.load(path)
    out = {}
    for name in z["names"].tolist():
        H, W, ks, stride, seed = (int(v) for v in z[name + ".case"])
        ds = working_ds(H, W)
        h, w = -(-H // ds), -(-W // ds)
        bits = lambda key, a, b: np.unpackbits(z[name + key])[:a * b].reshape(a, b).astype(bool)
        out[name] = dict(H=H, W=W, ks=ks, stride=stride, seed=seed, params=z[name + ".params"], edge=bits(".edge", h, w),
                         cand=bits(".cand", h, w), mask=bits(".mask", H, W))
    return out
