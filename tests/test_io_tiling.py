"""CPU: §8 rows a20 (loaders, controlnet/utils.py:10-52) and a22 (tiling, patch_utils.py).  Round 3: both rows are PINNED — the
bottom half of this file checks tiling.py / io_utils.py against goldens captured from the imported reference modules
(oracle/make_goldens.py --only-host); the top half keeps the file-format, arithmetic and partition-of-unity properties.  Not
pinned: `load_pair_to_sixch` (needs torchvision's `to_tensor`) and the cv2 LANCZOS4 resize branch of the merges."""
import numpy as np
import pytest
import torch

from diffcodec_amd import io_utils as IO
from diffcodec_amd import tiling as T


def test_flo_roundtrip_and_bad_magic(tmp_path):
    flow = np.random.RandomState(0).randn(7, 11, 2).astype(np.float32)
    p = tmp_path / "a.flo"
    IO.write_flo(str(p), flow)
    raw = p.read_bytes()
    assert len(raw) == 12 + 7 * 11 * 2 * 4 and np.frombuffer(raw[:4], np.float32)[0] == 202021.25
    assert np.frombuffer(raw[4:12], np.int32).tolist() == [11, 7]               # width, then height
    assert np.array_equal(IO.read_flo(str(p)), flow)
    bad = tmp_path / "b.flo"
    bad.write_bytes(np.array([1.0], np.float32).tobytes() + raw[4:])
    with pytest.raises(ValueError, match="Invalid .flo"):
        IO.read_flo(str(bad))


def test_resize_flow_rescales_vectors_to_pixel_units():
    flow = np.zeros((10, 20, 2), np.float32)
    flow[..., 0] = 4.0
    flow[..., 1] = -2.0
    out = IO.resize_flow_to(flow, 30, 40)
    assert out.shape == (1, 2, 30, 40)
    assert torch.allclose(out[:, 0], torch.full((1, 30, 40), 8.0)) and torch.allclose(out[:, 1], torch.full((1, 30, 40), -6.0))
    # align_corners=True keeps the corner samples
    ramp = np.stack([np.tile(np.arange(20, dtype=np.float32), (10, 1)), np.zeros((10, 20), np.float32)], -1)
    r = IO.resize_flow_to(ramp, 10, 39)
    assert r[0, 0, 0, 0].item() == 0.0 and abs(r[0, 0, 0, -1].item() - 19.0 * 39 / 20) < 1e-5


def test_load_controls_and_flows(tmp_path):
    from PIL import Image
    rs = np.random.RandomState(1)
    for n in ("f0.png", "f1.png"):
        Image.fromarray(rs.randint(0, 255, (48, 64, 3), dtype=np.uint8)).save(tmp_path / n)
    for n in ("fw.flo", "bw.flo"):
        IO.write_flo(str(tmp_path / n), rs.randn(48, 64, 2).astype(np.float32))
    six, flow = IO.load_controls_and_flows(tmp_path / "f0.png", tmp_path / "f1.png", str(tmp_path / "fw.flo"),
                                           str(tmp_path / "bw.flo"), size=(32, 32), device="cpu")
    assert six.shape == (1, 6, 32, 32) and flow.shape == (1, 4, 32, 32)
    assert six.dtype == torch.float32 and 0.0 <= six.min() and six.max() <= 1.0
    img0 = np.asarray(Image.open(tmp_path / "f0.png").convert("RGB").resize((32, 32), Image.BICUBIC), np.float32) / 255
    assert torch.allclose(six[0, :3], torch.from_numpy(img0).permute(2, 0, 1))


def test_crop_into_tiles_geometry_matches_the_notebook():
    img = np.zeros((3, 1024, 1024), np.float32)
    tiles, coords, full = T.crop_into_tiles(img, (512, 512), overlap=64, order="chw")
    assert full == (1024, 1024) and len(tiles) == 9                               # patch_exp.ipynb: x,y in {0,448,896}
    assert sorted({c[0] for c in coords}) == [0, 448, 896]
    assert tiles[0].shape == (3, 512, 512) and tiles[2].shape == (3, 512, 128) and tiles[8].shape == (3, 128, 128)


@pytest.mark.parametrize("order", ["hwc", "chw"])
def test_merges_reconstruct_the_image(order):
    rs = np.random.RandomState(2)
    img = rs.randint(0, 255, (96, 130, 3)).astype(np.float32)
    if order == "chw":
        img = img.transpose(2, 0, 1)
    tiles, coords, full = T.crop_into_tiles(img, (48, 64), overlap=16, order=order)
    flat = T.merge_tiles(tiles, coords, full, order)
    cos = T.merge_costiles(tiles, coords, full, order, feather=8)
    assert flat.dtype == np.uint8 and flat.shape == img.shape and cos.shape == img.shape
    assert np.abs(flat.astype(np.float32) - img).max() <= 1.0                     # weights are a partition of unity
    # reference arithmetic kept as is: `cosine_window(f)[:f]` is a whole 0->1->0 hump, so a tile's weight vanishes at its
    # pixels 0, f-1, h-f, h-1; where no other tile covers (the image's outer f-wide frame) the output drops to 0 there.
    # Away from that frame every pixel has positive total weight and the normalised blend reproduces the image.
    f = 8
    d = np.abs(cos.astype(np.float32) - img)
    inner = d[f:-f, f:-f] if order == "hwc" else d[:, f:-f, f:-f]
    assert inner.max() <= 1.0
    assert (cos[0] == 0).all() if order == "hwc" else (cos[:, 0] == 0).all()


def test_merge_costiles_weights_follow_the_reference_formula():
    """Two constant tiles that disagree: the output must be the weight-normalised mix with the reference's window
    (patch_utils.py:32-48: ones, with both f-wide ends replaced by a full (cos+1)/2 hump over linspace(-pi, pi, f))."""
    f = 16
    hump = (np.cos(np.linspace(-np.pi, np.pi, f)) + 1) / 2
    wx = np.ones(48)
    wx[:f] = hump
    wx[-f:] = hump
    a, b = np.full((32, 48, 1), 200.0, np.float32), np.full((32, 48, 1), 100.0, np.float32)
    out = T.merge_costiles([a, b], [(0, 32, 0, 48), (0, 32, 32, 80)], (32, 80), "hwc", feather=f)
    wa, wb = np.zeros(80), np.zeros(80)
    wa[0:48] = wx
    wb[32:80] = wx
    wy = np.ones(32)
    wy[:f] = hump
    wy[-f:] = hump
    y = 20                                                                            # a row with wy > 0
    exp = (200.0 * wa + 100.0 * wb) * wy[y] / np.maximum((wa + wb) * wy[y], 1e-8)
    assert np.array_equal(out[y, :, 0], exp.astype(np.float32).astype(np.uint8))


def test_latent_merge_partition_and_coordinate_quirk():
    lat = torch.randn(1, 4, 16, 16)
    # the function reads each tuple as (x1, x2, y1, y2) (patch_utils.py:140)
    coords = [(0, 64, 0, 64), (64, 128, 0, 64), (0, 64, 64, 128), (64, 128, 64, 128)]
    tiles = [lat[:, :, y1 // 8:y2 // 8, x1 // 8:x2 // 8] for (x1, x2, y1, y2) in coords]
    merged = T.merge_latent_tiles_from_pixel_coords(tiles, coords, (1, 4, 16, 16), (128, 128))
    w = torch.hann_window(8, periodic=False)
    inner = (w[:, None] * w[None, :]) > 1e-6
    m = inner.repeat(2, 2)                                                          # Hann is 0 on each tile's border
    assert torch.allclose(merged[0, :, m], lat[0, :, m], atol=1e-5)


def test_merge_ramp_is_a_partition_of_unity_everywhere():
    rs = np.random.RandomState(4)
    img = rs.randint(0, 255, (96, 130, 3)).astype(np.float32)
    from diffcodec_amd.tiled_decode import plan_tiles
    coords = plan_tiles(96, 130, 64, 16)
    tiles = [img[y1:y2, x1:x2] for y1, y2, x1, x2 in coords]
    out = T.merge_ramp(tiles, coords, (96, 130), "hwc", feather=16)
    assert np.array_equal(out, img.astype(np.uint8))                        # consistent tiles reproduce the frame exactly


def test_plan_tiles_full_windows_cover_the_frame():
    from diffcodec_amd.tiled_decode import plan_tiles
    assert plan_tiles(512, 960, 512, 64) == [(0, 512, 0, 512), (0, 512, 448, 960)]          # config 4: two tiles, x = 0 and 448
    c = plan_tiles(1080, 1920, 512, 64)
    assert all(y2 - y1 == 512 and x2 - x1 == 512 for y1, y2, x1, x2 in c)                    # no undersized edge tiles
    cover = np.zeros((1080, 1920), np.int32)
    for y1, y2, x1, x2 in c:
        cover[y1:y2, x1:x2] += 1
    assert cover.min() >= 1 and max(y2 for _, y2, _, _ in c) == 1080 and max(x2 for *_, x2 in c) == 1920
    assert len(plan_tiles(1024, 1024, 512, 0)) == 4                                          # config 5: 4 x 512 patches
    with pytest.raises(ValueError):
        plan_tiles(256, 1024, 512, 64)


def test_package_never_imports_the_oracle():
    import os, re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "diffcodec-controlling-latent-diffusion-for-perceptual-video-compression_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, re.M), f
                assert "oracle/" not in src or f == "selftest.py", f


# ------------------------------------------------------------------------------------------- reference-pinned (goldens)
# tests/golden/host_tiling.npz and host_flow_io.npz were captured by `python -m oracle.make_goldens --only-host` from the
# IMPORTED reference modules (/root/reference/patch_utils.py, controlnet/utils.py; empty stub modules for cv2 / test_utils /
# torchvision, none of whose symbols is reached on these branches).  Integer / byte results: bit-exact.
def _split(flat, shapes):
    out, off = [], 0
    for s in shapes:
        n = int(np.prod(s))
        out.append(flat[off:off + n].reshape(s))
        off += n
    assert off == flat.size
    return out


@pytest.mark.parametrize("order", ["hwc", "chw"])
def test_tiling_equals_reference_patch_utils(golden_dir, order):
    """crop_into_tiles (patch_utils.py:189-209), merge_tiles (:212-248), merge_costiles (:13-80) on a 120x176 image with
    ragged edge tiles: coordinates, tile contents and merged uint8 images equal the reference's, byte for byte."""
    z = np.load(f"{golden_dir}/host_tiling.npz")
    img = z["img"] if order == "hwc" else np.ascontiguousarray(z["img"].transpose(2, 0, 1))
    tiles, coords, full = T.crop_into_tiles(img, (64, 80), overlap=24, order=order)
    assert np.array_equal(np.asarray(coords), z[f"coords_{order}"]) and tuple(full) == tuple(z[f"full_{order}"])
    assert np.array_equal(np.asarray([t.astype(np.float64).sum() for t in tiles]), z[f"tile_sums_{order}"])
    assert np.array_equal(T.merge_tiles(tiles, coords, full, order=order), z[f"merge_tiles_{order}"])
    assert np.array_equal(T.merge_costiles(tiles, coords, full, order=order, feather=16), z[f"merge_costiles_{order}"])


def test_merge_costiles_truncates_like_the_reference(golden_dir):
    """Float tiles off the integer grid: the reference ends in `astype(np.uint8)` (truncation, patch_utils.py:80), kept."""
    z = np.load(f"{golden_dir}/host_tiling.npz")
    coords = [tuple(c) for c in z["coords_hwc"].tolist()]
    tiles = _split(z["img_float_tiles"], [(y2 - y1, x2 - x1, 3) for (y1, y2, x1, x2) in coords])
    assert np.array_equal(T.merge_costiles(tiles, coords, (120, 176), feather=24), z["img_float_tiles_merge_costiles"])


def test_latent_merge_equals_reference_including_its_coordinate_quirk(golden_dir):
    """merge_latent_tiles_from_pixel_coords (patch_utils.py:83-174) fed the (y1,y2,x1,x2) tuples crop_into_tiles emits, which it
    unpacks as (x1,x2,y1,y2) (:140): on a 256x384 frame most tiles are resized (bilinear) into the wrong slot — reproduced."""
    z = np.load(f"{golden_dir}/host_tiling.npz")
    coords = [tuple(c) for c in z["lat_coords"].tolist()]
    lats = [torch.from_numpy(a.copy()) for a in _split(z["lat_tiles"], [(1, 4, (y2 - y1) // 8, (x2 - x1) // 8) for (y1, y2, x1, x2) in coords])]
    got = T.merge_latent_tiles_from_pixel_coords(lats, coords, (1, 4, 32, 48), (256, 384))
    torch.testing.assert_close(got, torch.from_numpy(z["lat_merged"]), rtol=0, atol=0)


def test_flo_reader_and_flow_resize_equal_reference_utils(golden_dir, tmp_path):
    """read_flo (controlnet/utils.py:10-19) on the fixture's bytes, its bad-magic error text, and resize_flow_to (:21-28) up,
    down and at the identity size: equal to the reference's outputs bit for bit (same torch build, same arithmetic)."""
    z = np.load(f"{golden_dir}/host_flow_io.npz")
    p = tmp_path / "g.flo"
    p.write_bytes(z["flo_bytes"].tobytes())
    flow = IO.read_flo(str(p))
    assert flow.dtype == np.float32 and np.array_equal(flow, z["flow"])
    bad = tmp_path / "bad.flo"
    bad.write_bytes(np.array([1.0], np.float32).tobytes() + z["flo_bytes"].tobytes()[4:])
    with pytest.raises(ValueError) as ei:
        IO.read_flo(str(bad))
    assert str(ei.value).replace(str(bad), "<path>") == str(z["bad_magic_error"])
    for key, (h, w) in (("up_64x96", (64, 96)), ("down_24x20", (24, 20)), ("same_40x56", (40, 56))):
        torch.testing.assert_close(IO.resize_flow_to(flow, h, w), torch.from_numpy(z[key]), rtol=0, atol=0)


def test_product_package_reads_no_developer_environment():
    """The header promises no hidden state: the kernel sources hold no launcher A/B switches (no source reads the environment)
    and the Python side keeps plain module constants; only the launcher variables of `sharding` remain."""
    import os
    pkg = os.path.dirname(IO.__file__)
    for root, _, files in os.walk(pkg):
        if os.path.basename(root) in ("build", "__pycache__"):
            continue
        for f in files:
            src = open(os.path.join(root, f), errors="ignore").read() if f.endswith((".py", ".hip", ".h")) else ""
            if f.endswith((".hip", ".h")):
                assert "getenv" not in src, f
            elif f.endswith(".py") and f not in ("sharding.py", "build.py"):
                assert "os.environ" not in src and "getenv" not in src, f


def test_kernel_sources_have_no_build_switches():
    """The product kernels exist in one form: the only preprocessor conditional in csrc/*.hip and csrc/dc_common.h is the
    `#ifdef DC_STAMP` of the phase-stamp instrumentation (tools/*_stamp.py), with its #else / #endif.  A/B variants are compared
    as two builds of two commits, not as switches in the product sources."""
    import glob
    import os
    import re
    csrc = os.path.join(os.path.dirname(IO.__file__), "csrc")
    files = sorted(glob.glob(os.path.join(csrc, "*.hip"))) + [os.path.join(csrc, "dc_common.h")]
    assert len(files) > 10
    for path in files:
        for no, line in enumerate(open(path).read().splitlines(), 1):
            m = re.match(r"\s*#\s*(if|ifdef|ifndef|elif|elifdef|elifndef|else|endif)\b(.*)", line)
            if not m:
                continue
            kind, rest = m.group(1), m.group(2).split("//")[0].strip()
            where = f"{os.path.basename(path)}:{no}: {line.strip()}"
            if kind in ("else", "endif"):
                continue            # every opener is `#ifdef DC_STAMP` (checked below), so these close or split one of them
            assert kind == "ifdef" and rest == "DC_STAMP", where
