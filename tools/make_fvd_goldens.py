"""Write tests/golden/fvd_i3d.npz: what the reference's own FVD code (fvd_utils/models/fvd/pytorch_i3d.py and fvd.py) computes on the
CPU for seeded inputs and the seeded weights of tests/fvd_ref.synth_weights.  Arrays only: no weights (they are regenerated from
the seed) and no program text.

    python tools/make_fvd_goldens.py --reference <checkout of the reference project>

Also prints the error of the restatement against the reference and of its fp32 run against its fp64 run per endpoint (the table
in tests/test_gpu_fvd.py and DESIGN.md)."""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fvd_ref  # noqa: E402

WEIGHT_SEED = 1234
SAMPLES = 1000                       # values kept per endpoint


def net_input(t, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(1, 3, t, 224, 224, generator=g, dtype=torch.float64) * 2 - 1


def source_video(h, w, seed, frames=2):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(1, frames, 3, h, w, generator=g, dtype=torch.float64)


def subsample(t, count=SAMPLES):
    flat = t.reshape(-1)
    return flat[::max(1, flat.numel() // count)][:count].contiguous()


def row_sets():
    """name -> (fake rows, real rows), fp64 [n,400]"""
    g = torch.Generator().manual_seed(99)
    mix = torch.randn(400, 400, generator=g, dtype=torch.float64) / 20
    a = torch.randn(450, 400, generator=g, dtype=torch.float64) @ (torch.eye(400, dtype=torch.float64) + mix)
    b = 1.3 * torch.randn(450, 400, generator=g, dtype=torch.float64) + 0.1
    f1 = 11 * torch.randn(1, 400, generator=g, dtype=torch.float64)
    f2 = f1 + torch.randn(1, 400, generator=g, dtype=torch.float64)
    c = 11 * torch.randn(16, 400, generator=g, dtype=torch.float64)
    d = 11 * torch.randn(16, 400, generator=g, dtype=torch.float64) + 0.5
    return {"rows450": (a, b), "rows2": (f1.repeat(2, 1), f2.repeat(2, 1)), "rows16": (c, d)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("DIFFCODEC_REFERENCE"), help="checkout of the reference project")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "fvd_i3d.npz"))
    args = ap.parse_args()
    if not args.reference or not os.path.isdir(args.reference):
        sys.exit("the reference project is needed: --reference DIR")
    def load(name):                                  # the two files by path: the reference's package __init__ needs its own cwd
        spec = importlib.util.spec_from_file_location("reference_" + name, os.path.join(args.reference, "fvd_utils", "models", "fvd", name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod

    ref_fvd = load("fvd")
    InceptionI3d = load("pytorch_i3d").InceptionI3d

    torch.set_grad_enabled(False)
    sd = fvd_ref.synth_weights(WEIGHT_SEED)
    model = InceptionI3d(400, in_channels=3).double().eval()
    model.load_state_dict({k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}, strict=True)

    out = {"weight_seed": np.int64(WEIGHT_SEED)}
    for t, seed in ((10, 510), (11, 511)):
        x = net_input(t, seed)
        want = model(x)
        ours = fvd_ref.endpoints(x, sd)
        y = x
        for e, name in enumerate(model.VALID_ENDPOINTS[:16]):
            y = model._modules[name](y)
            out[f"t{t}_ep{e:02d}"] = subsample(y).numpy()
            err = float((ours[e] - y).abs().max() / y.abs().max())
            print(f"T={t} {name:18s} shape {tuple(y.shape)} positive {float((y > 0).double().mean()):.2f} restatement-reference {err:.1e}")
        out[f"t{t}_logits"] = want.numpy()
        out[f"t{t}_input_seed"] = np.int64(seed)
        mine = fvd_ref.head(ours[-1], sd)
        print(f"T={t} logits std {float(want.std()):.2f} restatement-reference {float((mine - want).abs().max() / want.abs().max()):.1e}")
        eps32 = fvd_ref.endpoints(x, sd, dtype=torch.float32)
        for e, name in enumerate(model.VALID_ENDPOINTS[:16]):
            print(f"T={t} {name:18s} fp32-fp64 {float((eps32[e].double() - ours[e]).abs().max() / ours[e].abs().max()):.2e}")
        l32 = fvd_ref.head(eps32[-1], sd, dtype=torch.float32).double()
        print(f"T={t} logits             fp32-fp64 {float((l32 - mine).abs().max() / mine.abs().max()):.2e}")

    for name, (h, w, seed) in {"wide": (40, 56, 520), "tall": (96, 64, 521)}.items():
        v = source_video(h, w, seed)                                     # [1,T,3,H,W]
        ctHW = v[0].permute(1, 0, 2, 3).contiguous()
        r64 = ref_fvd.preprocess_single(ctHW)
        r32 = ref_fvd.preprocess_single(ctHW.float())
        mine = fvd_ref.preprocess(v)[0]
        out[f"prep_{name}_f64"] = subsample(r64, 8000).numpy()
        out[f"prep_{name}_f32"] = subsample(r32, 8000).numpy()
        out[f"prep_{name}_seed"] = np.int64(seed)
        print(f"preprocess {name}: restatement-reference(fp64) {float((mine - r64).abs().max()):.1e} "
              f"reference fp32-restatement {float((r32.double() - mine).abs().max()):.1e}")

    for name, (fake, real) in row_sets().items():
        want = ref_fvd.frechet_distance(fake.numpy().copy(), real.numpy().copy())
        mine = fvd_ref.frechet(fake, real)
        out[f"frechet_{name}"] = np.float64(want)
        print(f"frechet {name}: reference {want:.12g} restatement {mine:.12g} relative {abs(mine - want) / abs(want):.1e}")

    np.savez_compressed(args.out, **out)
    print(args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
