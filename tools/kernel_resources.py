"""Developer tool (host only, nothing is run on a GPU): did a refactor of the bf16 matrix kernels change their code?

    python tools/kernel_resources.py PARENT_TREE [CHANGE_TREE] [--files a.hip,b.hip] [--keep DIR] > profiles/<name>.txt

A tree is a checkout of this repository (at least <package>/csrc and include/); CHANGE_TREE defaults to the working tree.  Every file
is cross-compiled to gfx950 assembly with the product flags of build.py (FLAGS + the file's EXTRA_FLAGS) plus --cuda-device-only -S.
One row per kernel symbol: VGPR / AGPR / SGPR, scratch bytes per lane, occupancy (waves per SIMD), instruction count, and
  identical     the same instruction stream once local labels are renumbered
  same opcodes  the same multiset of mnemonics (scheduling and register allocation may differ)
  differs       followed by every mnemonic whose count moved, parent->change
A cell "a->b" = parent -> change; a single value = unchanged."""
import collections
import glob
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from diffcodec_amd import build as dcbuild

FILES = ["gemm_dma.hip", "gemm_wide.hip", "gemm_p8.hip", "gemm_rowpanel.hip", "conv3x3_tile.hip", "igemm.hip"]
INFO = {"vgpr": "NumVgprs", "agpr": "NumAgprs", "sgpr": "TotalNumSgprs", "scratch": "ScratchSize", "occ": "Occupancy"}


def compile_asm(tree, name, outdir):
    src = glob.glob(os.path.join(tree, "*", "csrc", name))
    assert len(src) == 1, "expected one %s under %s/*/csrc" % (name, tree)
    out = os.path.join(outdir, name.replace(".hip", ".s"))
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    deps = glob.glob(os.path.join(os.path.dirname(src[0]), "*.h")) + src
    if os.path.exists(out) and os.path.getmtime(out) > max(os.path.getmtime(d) for d in deps):
        return out                                   # --keep DIR: a tree that did not change is not compiled again
    subprocess.check_call([hipcc] + dcbuild.FLAGS + dcbuild.EXTRA_FLAGS.get(name, []) + ["--cuda-device-only", "-S", src[0], "-o", out])
    return out


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}
    clean = lambda s: re.sub(r"^void |\(anonymous namespace\)::|\(dc_conv_desc.*\)$", "", s)
    return {n: clean(o) for n, o in zip(names, out)}


def kernels(path):
    """symbol -> dict(instr=[normalised instruction lines], vgpr=.., agpr=.., sgpr=.., scratch=.., occ=..) for every kernel of a .s file"""
    res, sym, body = {}, None, None
    for line in open(path):
        m = re.match(r"^(\w+):\s", line)
        if m and not m.group(1).startswith(".") and body is None:
            sym, body = m.group(1), []
        elif line.startswith(".Lfunc_end") and body is not None:
            labels = {}
            ren = lambda t: re.sub(r"\.LBB\d+_\d+", lambda x: labels.setdefault(x.group(0), "L%d" % len(labels)), t)
            res[sym] = {"instr": [ren(i) for i in body]}
            body = None
        elif body is not None:
            t = line.split(";")[0].strip()
            if t and not t.startswith(".") or re.match(r"\.LBB\d+_\d+:", t):
                body.append(t)
        elif sym in res:
            for key, tag in INFO.items():
                m = re.match(r"; %s: (\d+)" % tag, line)
                if m:
                    res[sym][key] = int(m.group(1))
    return {s: k for s, k in res.items() if "occ" in k}              # kernels only: device functions carry no occupancy line


def mnemonics(instr):
    return collections.Counter(i.split()[0] for i in instr if not i.endswith(":"))


def cell(a, b):
    return str(a) if a == b else "%s->%s" % (a, b)


def main(argv):
    args = [a for a in argv if not a.startswith("--")]
    opts = dict(a[2:].split("=", 1) if "=" in a else (a[2:], "") for a in argv if a.startswith("--"))
    if not args:
        sys.exit(__doc__)
    trees = [os.path.abspath(args[0]), os.path.abspath(args[1]) if len(args) > 1 else ROOT]
    files = opts["files"].split(",") if opts.get("files") else FILES
    keep = opts.get("keep") or tempfile.mkdtemp(prefix="kernel_resources_")
    jobs = []
    for side, tree in zip(("parent", "change"), trees):
        os.makedirs(os.path.join(keep, side), exist_ok=True)
        jobs += [(tree, f, os.path.join(keep, side)) for f in files]
    with ThreadPoolExecutor(max_workers=min(6, os.cpu_count() or 1)) as ex:
        asm = list(ex.map(lambda j: compile_asm(*j), jobs))
    tally = collections.Counter()
    print("%-84s %10s %6s %10s %8s %5s  %s" % ("kernel instance", "VGPR", "AGPR", "SGPR", "scratch", "occ", "code"))
    for i, f in enumerate(files):
        old, new = kernels(asm[i]), kernels(asm[len(files) + i])
        names = demangle(list(new))
        for sym, n in new.items():
            o = old.get(sym)
            if o is None:
                print("%-84s (not in the parent)" % names[sym])
                tally["new"] += 1
                continue
            ho, hn = mnemonics(o["instr"]), mnemonics(n["instr"])
            verdict = "identical" if o["instr"] == n["instr"] else "same opcodes" if ho == hn else "differs"
            tally[verdict] += 1
            count = cell(sum(ho.values()), sum(hn.values()))
            print("%-84s %10s %6s %10s %8s %5s  %s, %s instr" % ((names[sym],) + tuple(cell(o[k], n[k]) for k in ("vgpr", "agpr", "sgpr", "scratch", "occ"))
                                                                + (verdict, count)))
            if verdict == "differs":
                print("    moved: " + ", ".join("%s %d->%d" % (m, ho[m], hn[m]) for m in sorted(set(ho) | set(hn)) if ho[m] != hn[m]))
        for sym in set(old) - set(new):
            print("%-84s (parent only)" % demangle([sym])[sym])
            tally["gone"] += 1
    print("\n" + ", ".join("%d %s" % (v, k) for k, v in tally.items()))


if __name__ == "__main__":
    main(sys.argv[1:])
