"""CPU: the integer restatement of Pillow's 8-bit resize (tests/resample_ref.py) against Pillow's recorded bytes
(tests/golden/pil_resample.npz) and against the Pillow installed here; `diffcodec_amd.resample.coeffs` against the restatement's
tables; and the `score_size` wiring of the clip scorer where no resize happens.  Every comparison is on bytes."""
import numpy as np
import pytest
import torch

import metrics_ref
import resample_ref as R
from diffcodec_amd import clip_decode as CD, metrics, resample
from test_clip_decode import FakePipe


@pytest.fixture(scope="module")
def golden():
    return np.load(R.GOLDEN)


@pytest.mark.parametrize("case", range(len(R.SMALL_CASES)))
def test_restatement_equals_the_recorded_pillow_bytes(golden, case):
    a = R.small_input(case)
    assert np.array_equal(a, golden[f"in_{case}"])
    for name in R.FILTERS:
        want = golden[f"out_{case}_{name}"]
        got = R.resize(a, R.SMALL_CASES[case][1], name)
        assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want), (case, name)


def test_restatement_equals_live_pillow():
    pytest.importorskip("PIL")
    for case, (_, size) in enumerate(R.SMALL_CASES):
        for c in (1, 3, 4):
            a = R.small_input(case, c)
            for name in R.FILTERS:
                assert np.array_equal(R.resize(a, size, name), R.pillow_resize(a, size, name)), (case, c, name)
    a = R.random_bytes((1024, 1920, 3), 7)
    assert np.array_equal(R.resize(a, (512, 512), "bilinear"), R.pillow_resize(a, (512, 512), "bilinear"))
    b = R.checkerboard(37, 53)
    for name in R.FILTERS:
        assert np.array_equal(R.resize(b, (64, 41), name), R.pillow_resize(b, (64, 41), name)), name


AXES = sorted({(i, o) for (hw, size) in R.SMALL_CASES for i, o in zip(hw, size)} | {(1920, 512), (1024, 512), (270, 1080), (480, 1920), (512, 299)})


@pytest.mark.parametrize("name", R.FILTERS)
def test_coeffs_equal_the_restatement_tables(name):
    for i, o in AXES:
        bounds, K, ksize = resample.coeffs(i, o, name)
        rb, rk, rks = R.table(i, o, name)
        assert ksize == rks and bounds.dtype == torch.int32 and K.dtype == torch.int32 and tuple(K.shape) == (o, ksize), (i, o)
        assert np.array_equal(bounds.numpy(), rb) and np.array_equal(K.numpy(), rk), (i, o)
    with pytest.raises(ValueError):
        resample.coeffs(4, 4, "nearest")
    with pytest.raises(ValueError):
        resample.coeffs(0, 4, name)


def test_byte_to_float_and_back_is_exact():
    """the reference scores ToTensor(frame) * 255 in fp32: (b / 255) * 255 is b for every byte, so scoring the bytes is the same"""
    b = torch.arange(256, dtype=torch.uint8)
    f = b.float().div(255.0) * 255
    assert f.dtype == torch.float32 and torch.equal(f, b.float())


class _Source:
    """seeded controls and ground truth of H x W frames on the host"""

    def __init__(self, h, w):
        self.h, self.w = h, w

    def controls(self, frame, prev, nxt):
        g = torch.Generator().manual_seed(100 + frame)
        return torch.rand(1, 6, self.h, self.w, generator=g), torch.randn(1, 4, self.h, self.w, generator=g)

    def ground_truth(self, frame):
        g = torch.Generator().manual_seed(200 + frame)
        return torch.randint(0, 256, (self.h, self.w, 3), generator=g, dtype=torch.uint8)


def test_score_size_none_and_frame_size_change_nothing(monkeypatch):
    """no GPU here: the two metric calls are replaced by their fp64 restatements, the driver and its `score_size` path are the
    product's.  None is the call without the keyword; a score_size equal to the frame size resizes nothing."""
    monkeypatch.setattr(metrics, "psnr", lambda x, y, data_range=255.0: metrics_ref.psnr(x, y, data_range))
    monkeypatch.setattr(metrics, "ms_ssim", lambda x, y, data_range=255: metrics_ref.ms_ssim(x, y, data_range=data_range))
    h = w = 176
    src = _Source(h, w)
    pe = torch.zeros(1, 77, 8)
    kw = dict(tile=h, batch=4, seed=3, rank=0, world=1, score=True)
    plain = CD.decode_clip(FakePipe(), src, 5, 4, h, w, pe, pe, **kw)
    assert sorted(plain["scores"]) == [1, 2, 3] and all(5 < s["psnr"] < 1000 for s in plain["scores"].values())
    for size in (None, (h, w)):
        out = CD.decode_clip(FakePipe(), src, 5, 4, h, w, pe, pe, score_size=size, **kw)
        assert out["scores"] == plain["scores"]
        assert all(np.array_equal(out["frames"][f], plain["frames"][f]) for f in plain["frames"])
    frames = {f: torch.from_numpy(a) for f, a in plain["frames"].items()}
    assert CD.score_frames(frames, src) == CD.score_frames(frames, src, score_size=None) == plain["scores"]
    assert CD.score_frames(frames, src, score_size=(h, w)) == plain["scores"]


def test_out_of_range_arguments_are_refused_before_any_launch():
    """every call below is invalid, so the library returns its error code without touching a pointer (none of them is real)"""
    import ctypes
    from diffcodec_amd import lib
    L = lib.load()
    assert L.dc_resample_ws_bytes(2, 37, 41, 3) == 2 * 37 * 41 * 3
    for bad in ((0, 37, 41, 3), (2, 0, 41, 3), (2, 37, 0, 3), (2, 37, 41, 0), (2, 37, 41, 5)):
        assert L.dc_resample_ws_bytes(*bad) == -1
    st = (ctypes.c_longlong * 4)(37 * 53 * 3, 1, 53 * 3, 3)
    p = 4096                                                       # a non-null pointer value; never dereferenced
    kh, kv = resample.coeffs(53, 41, "bicubic")[2], resample.coeffs(37, 64, "bicubic")[2]
    good = dict(inp=p, strides=st, n=2, h_in=37, w_in=53, c=3, h_out=64, w_out=41, k_h=p, b_h=p, ks_h=kh, k_v=p, b_v=p, ks_v=kv,
                scratch=p, out=p)
    bad = [dict(n=0), dict(h_in=0), dict(w_in=0), dict(h_out=0), dict(w_out=0), dict(c=0), dict(c=5), dict(inp=0), dict(out=0),
           dict(strides=None), dict(scratch=0), dict(k_h=0), dict(b_h=0), dict(k_v=0), dict(b_v=0),     # a null table, sizes differ
           dict(ks_h=kh + 1), dict(ks_v=kv - 1), dict(ks_h=0),                                           # ksize not the table's
           dict(w_out=53), dict(h_out=37),                                                              # a table for a skipped pass
           dict(w_out=53, h_out=37, k_h=0, b_h=0, k_v=0, b_v=0)]                                         # nothing to resample
    for change in bad:
        a = dict(good, **change)
        with pytest.raises(lib.HipLaunchError, match="invalid argument"):
            lib.call("dc_resample_u8", a["inp"], a["strides"], a["n"], a["h_in"], a["w_in"], a["c"], a["h_out"], a["w_out"], a["k_h"],
                     a["b_h"], a["ks_h"], a["k_v"], a["b_v"], a["ks_v"], a["scratch"], a["out"], None)
