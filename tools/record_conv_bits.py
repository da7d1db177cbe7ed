"""Record the bits of every routed bf16 GEMM / conv instance (csrc/gemm_dma.hip, gemm_wide.hip, gemm_p8.hip, gemm_rowpanel.hip,
igemm.hip, conv3x3_tile.hip) into tests/golden/conv_epilogue_bits.json: one row per case of tests/edge_cases.py::CONV_CASES with the
sha256 of

    operands   the bytes of every operand view, in name order (a moved random stream shows here, not as changed arithmetic)
    out        the output view
    stats_out  the LayerNorm row statistics, where the case asks for them
    gn_part    the GroupNorm partials, where the launch emits them

    python tools/record_conv_bits.py [--lib PATH] [--out FILE]

`--lib` points diffcodec_amd.lib at another build of the same ABI.  The golden was recorded through `--lib` from a build of the
sources that preceded csrc/dc_epilogue.h, twice, with identical files: the code under test never records.  It pins every rounding
of the epilogues (tests/test_gpu_conv_bits.py); the fp64 comparisons of tests/test_gpu_edges.py would pass a reordered sum.  A
mismatch after a refactor means the arithmetic changed: fix the code, do not record again."""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import edge_cases as E  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_epilogue_bits.json")
DEV = "cuda"


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(E.ws_bits(t.detach()).cpu().numpy().tobytes())
    return h.hexdigest()


def name(i):
    return f"{i:03d} {E.CONV_CASES[i].label()}"


def run(i):
    """The row of case i: {"operands", "out"[, "stats_out"][, "gn_part"]} -> sha256"""
    from diffcodec_amd import ops
    c = E.CONV_CASES[i]
    pc, guards, x1, kw = E.conv_operands(ops, c, i, DEV)
    row = {"operands": sha(*[guards[k].view for k in sorted(guards)])}
    og = E.Guarded((c.n, c.ho, c.wo, c.cout // 2 if c.geglu else c.cout), torch.float32 if c.out_f32 else torch.bfloat16, DEV)
    sog = E.Guarded((c.m, ops.row_stats_parts(c.cout), 2), torch.float32, DEV) if c.stats_out else None
    y = ops.conv(x1.view, pc, out=og.view, stats_out=None if sog is None else sog.view, **kw)
    torch.cuda.synchronize()
    row["out"] = sha(og.view)
    if sog is not None:
        row["stats_out"] = sha(sog.view)
    gp = getattr(y, "gn_part", None)
    if gp is not None:
        row["gn_part"] = sha(gp)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="another build of libdiffcodec_hip.so (same ABI)")
    ap.add_argument("--out", default=GOLDEN)
    a = ap.parse_args()
    if a.lib:
        from diffcodec_amd import lib
        lib.LIB_PATH = os.path.abspath(a.lib)
    assert torch.cuda.is_available(), "recording needs the GPU"
    rows = {name(i): run(i) for i in range(len(E.CONV_CASES))}
    with open(a.out, "w") as fh:
        json.dump(rows, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(f"wrote {len(rows)} rows to {a.out}")


if __name__ == "__main__":
    main()
