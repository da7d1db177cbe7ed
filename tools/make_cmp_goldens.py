"""Write tests/golden/cmp_flow.npz: what the reference's own CMP module (cmp/models/modules/cmp.py), Fuser.convert_flow
(cmp/utils/visualize_utils.py) and the align_corners upsample of CMP.eval (cmp/models/cmp.py) compute on the CPU for the seeded
inputs and the seeded weights of tests/cmp_ref.py, in fp64 and in fp32.  Arrays only: fixed-stride subsamples of every endpoint,
the seeds and the reference's own fp32-minus-fp64 error per endpoint; no weights (they are regenerated from the seed) and no
program text.

    python tools/make_cmp_goldens.py --reference <checkout of the reference project>

Also prints the statistics the seeding rules ask for (share of one-hot pixels, spread of the flow) and the error of the
restatement against the reference per endpoint."""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cmp_ref as R  # noqa: E402

CASES = {"skip": (2, 64, 88, 810), "plain": (2, 64, 88, 811)}          # arch -> (N, H, W, input seed)


def reference_modules(root):
    """The reference's network files loaded by path under stand-in `cmp.*` packages (`import cmp` itself needs cv2)."""
    def package(name):
        m = types.ModuleType(name)
        m.__path__ = []
        sys.modules[name] = m
        return m

    def load(name, path, into=None):
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        if into is not None:
            into.__dict__.update({k: v for k, v in mod.__dict__.items() if not k.startswith("_")})
        return mod

    top, models = package("cmp"), package("cmp.models")
    backbone, modules, utils = package("cmp.models.backbone"), package("cmp.models.modules"), package("cmp.utils")
    top.models, models.backbone, models.modules, top.utils = models, backbone, modules, utils
    sys.modules["cmp.utils.flowlib"] = utils.flowlib = types.ModuleType("cmp.utils.flowlib")
    base = os.path.join(root, "cmp")
    load("cmp.models.backbone.resnet", os.path.join(base, "models", "backbone", "resnet.py"), backbone)
    load("cmp.models.modules.shallownet", os.path.join(base, "models", "modules", "shallownet.py"), modules)
    load("cmp.models.modules.decoder", os.path.join(base, "models", "modules", "decoder.py"), modules)
    net = load("cmp.models.modules.cmp", os.path.join(base, "models", "modules", "cmp.py"))
    vis = load("cmp.utils.visualize_utils", os.path.join(base, "utils", "visualize_utils.py"))
    return net.CMP, vis.Fuser


def reference_run(CMP, Fuser, arch, sd, image, sparse, dtype):
    """dict of R.ENDPOINTS[arch] through the reference's modules (hooks pick the intermediates up)"""
    cfg = R.CONFIGS[arch]
    model = CMP(cfg).to(dtype).eval()
    model.load_state_dict({k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}, strict=True)
    got = {}
    keep = lambda name: (lambda mod, inp, out: got.__setitem__(name, out[0] if isinstance(out, tuple) else out))
    model.flow_encoder.register_forward_hook(keep("sparse_enc"))
    model.image_encoder.register_forward_hook(keep("img_enc"))
    model.image_encoder.relu.register_forward_hook(lambda mod, inp, out: got.setdefault("skip2", out.clone()))
    model.image_encoder.layer1.register_forward_hook(keep("skip4"))
    if arch == "skip":
        for name in ("fusion8", "fusion4", "fusion2"):
            getattr(model.flow_decoder, name).register_forward_hook(keep("f" + name[-1]))
    else:
        model.flow_decoder.head.register_forward_hook(lambda mod, inp, out: got.__setitem__("cat8", inp[0]))
    got["logits"] = model(image.to(dtype), sparse.to(dtype))
    standin = types.SimpleNamespace(nbins=cfg["nbins"])                 # Fuser.__init__ moves its mesh to a GPU
    step = 2 * cfg["fmax"] / float(cfg["nbins"])
    standin.mesh = torch.arange(cfg["nbins"]).view(1, -1, 1, 1).to(dtype) * step - cfg["fmax"] + step / 2     # Fuser.__init__'s, in dtype
    got["flow"] = Fuser.convert_flow(standin, got["logits"].clone())
    got["flow_up"] = torch.nn.functional.interpolate(got["flow"], size=image.shape[2:4], mode="bilinear", align_corners=True)
    return got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("DIFFCODEC_REFERENCE"), help="checkout of the reference project")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "cmp_flow.npz"))
    ap.add_argument("--head-scale", type=float, default=None, help="override cmp_ref.HEAD_SCALE (to calibrate it)")
    args = ap.parse_args()
    if not args.reference or not os.path.isdir(args.reference):
        sys.exit("the reference project is needed: --reference DIR")
    CMP, Fuser = reference_modules(args.reference)
    torch.set_grad_enabled(False)
    out = {"weight_seed": np.int64(R.WEIGHT_SEED)}
    for arch, (n, h, w, seed) in CASES.items():
        sd = R.synth_weights(arch, R.WEIGHT_SEED, args.head_scale)
        u8, sparse = R.inputs(n, h, w, seed)
        img64 = R.normalise(u8)
        r64 = reference_run(CMP, Fuser, arch, sd, img64, sparse, torch.float64)
        r32 = reference_run(CMP, Fuser, arch, sd, img64.float(), sparse, torch.float32)
        mine = R.endpoints(img64, sparse, sd, arch)
        out[f"{arch}_case"] = np.array([n, h, w, seed], dtype=np.int64)
        for name in R.ENDPOINTS[arch]:
            ref = r64[name]
            peak = float(ref.abs().max())
            e32 = float((r32[name].double() - ref).abs().max())
            out[f"{arch}_{name}"] = R.subsample(ref).numpy()
            out[f"{arch}_{name}_f32"] = R.subsample(r32[name]).numpy()
            out[f"{arch}_{name}_err32"] = np.float64(e32)
            out[f"{arch}_{name}_peak"] = np.float64(peak)
            print(f"{arch} {name:10s} shape {tuple(ref.shape)} peak {peak:9.3f} positive {float((ref > 0).double().mean()):.2f} "
                  f"reference fp32-fp64 {e32:.2e} ({e32 / peak:.2e} of peak) restatement-reference {float((mine[name] - ref).abs().max()) / peak:.1e}")
        lg = r64["logits"]
        nb = R.CONFIGS[arch]["nbins"]
        pk = torch.maximum(torch.softmax(lg[:, :nb], 1).max(1).values, torch.softmax(lg[:, nb:], 1).max(1).values)
        onehot = float((pk > 0.99).double().mean())
        print(f"{arch} logits std {float(lg.std()):.2f} |max| {float(lg.abs().max()):.1f} one-hot pixels {onehot:.3f} "
              f"flow std {float(r64['flow'].std()):.2f} range {float(r64['flow'].min()):.1f} .. {float(r64['flow'].max()):.1f}")
        out[f"{arch}_onehot"] = np.float64(onehot)
    np.savez_compressed(args.out, **out)
    print(args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
