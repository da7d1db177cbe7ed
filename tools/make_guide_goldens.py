"""Record tests/golden/guide_points.npz from the reference's own flow_sampler (cmp/utils/data_utils.py).

    python tools/make_guide_goldens.py --reference /path/to/reference

Needs scipy and Pillow; `cv2` is replaced by a stub (the module only switches OpenCL off at import).  For every case the file
holds the parameters of a synthetic flow (tests/guide_ref.py rebuilds it), the candidate mask from the reference's get_edge,
distance_transform_edt, nms and remove_border, and the mask of flow_sampler(['grid', 'watershed']) under np.random.seed(seed).
Data only.  A case is refused when a pixel's normalised edge magnitude lies within 1e-4 of the 0.1 threshold."""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import guide_ref as G  # noqa: E402

# name: (H, W, nms_ks, grid stride, seed, discs); discs 0 = constant flow, -1 = vertical bands 16 apart (plateaus of ties)
CASES = {
    "small": (64, 96, 15, 16, 11, 4),
    "bands": (48, 80, 15, 16, 12, -1),
    "bands_ks5": (48, 80, 5, 16, 13, -1),
    "odd": (37, 53, 3, 8, 2, 3),
    "qvga": (120, 160, 15, 32, 3, 5),
    "wide_window": (24, 40, 81, 8, 4, 2),
    "square512": (512, 512, 41, 80, 5, 6),
    "half_hd": (540, 960, 15, 80, 6, 6),
    "full_hd": (1080, 1920, 49, 80, 7, 6),
    "constant": (64, 96, 15, 16, 8, 0),
    "constant512": (512, 512, 15, 80, 9, 0),
    "constant_hd": (1080, 1920, 15, 80, 10, 0),
}
GAP = 1e-4


def load_reference(root):
    cv2 = types.ModuleType("cv2")
    cv2.ocl = types.SimpleNamespace(setUseOpenCL=lambda flag: None)
    sys.modules.setdefault("cv2", cv2)
    spec = importlib.util.spec_from_file_location("reference_data_utils", os.path.join(root, "cmp", "utils", "data_utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference checkout")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "guide_points.npz"))
    args = ap.parse_args()
    D = load_reference(args.reference)
    import scipy.ndimage as ndimage
    out = {"names": np.array(sorted(CASES))}
    for name, (H, W, ks, stride, seed, discs) in sorted(CASES.items()):
        params = G.synth_params(seed, H, W, max(discs, 0))
        if discs == 0:
            params[0, [1, 2, 4, 5]] = 0.0
        if discs < 0:
            params = np.concatenate([params, [[x0, 0, 16, 6.0, -3.0, 1] for x0 in range(8, W, 32)]])
        flow = G.synth_flow(params, H, W)
        ds = max(1, max(H, W) // 400)
        edge = D.get_edge(flow[::ds, ::ds, :])
        edge /= max(edge.max(), 0.01)
        gap = float(np.abs(edge.astype(np.float64) - 0.1).min())
        assert gap >= GAP, f"{name}: a pixel lies {gap:.3g} from the threshold; pick another seed"
        binary = (edge > 0.1).astype(np.float32)
        res = D.nms(ndimage.distance_transform_edt(1 - binary), ks)
        D.remove_border(res)
        cand = res > 0
        if discs == 0:
            assert not binary.any() and not cand.any(), f"{name}: a constant flow gave {int(cand.sum())} candidates"
        np.random.seed(seed)
        sparse, mask = D.flow_sampler(flow, strategy=["grid", "watershed"], bg_ratio=1.0 / (stride * stride), nms_ks=ks)
        assert int(np.sqrt(1.0 / (1.0 / (stride * stride)))) == stride and (mask[:, :, 0] == mask[:, :, 1]).all()
        assert (sparse[mask == 1] == flow[mask == 1]).all() and not sparse[mask == 0].any()
        out[name + ".case"] = np.array([H, W, ks, stride, seed], dtype=np.int64)
        out[name + ".params"] = params
        out[name + ".edge"] = np.packbits(binary.astype(bool))
        out[name + ".cand"] = np.packbits(cand)
        out[name + ".mask"] = np.packbits(mask[:, :, 0].astype(bool))
        print(f"{name}: {H}x{W} ds {ds} ks {ks}: {int(binary.sum())} edge pixels (gap {gap:.2e}), {int(cand.sum())} candidates, "
              f"{int(mask[:, :, 0].sum())} guide points")
    np.savez_compressed(args.out, **out)
    print(args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
