"""CPU: the dispatcher's route query (dc_conv_route: host code, launches nothing) — its kernel codes match the header, and the
Python rule `ops.rowpanel_takes` that steers the transformer's proj_in agrees with the library on every shape the models launch."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as g
    from diffcodec_amd import lib, ops as o
    if not os.path.exists(lib.LIB_PATH):
        g.build()
    return o


def _desc(ops, rows, per_sample, cin, cout, **kw):
    from diffcodec_amd.lib import ConvDesc
    n = rows // per_sample
    base = dict(x1=16, w=16, out=16, bias=16, N=n, H=1, W=per_sample, C1=cin, Cout=cout, ksize=1, stride=1, pad=0, Ho=1,
                Wo=per_sample, out_scale=1.0, splitk=1)
    base.update(kw)
    return ConvDesc(**base)


def test_route_names_match_the_header(ops):
    src = open(os.path.join(ROOT, "include", "diffcodec_hip.h")).read()
    codes = {int(v): k.lower() for k, v in re.findall(r"#define DC_ROUTE_([A-Z0-9_]+) (\d+)", src) if k != "INFO_INTS"}
    assert ops.ROUTE_NAMES == codes
    assert int(re.search(r"#define DC_ROUTE_INFO_INTS (\d+)", src).group(1)) == 5


# transformer widths x map sizes (512x512 frames / windows: latent 64x64 and its three down levels) x the samples of one launch
# (cfg-shared halves and full CFG batches of the 1 / 2 (C4 windows) / 11 / 16 / 44-frame legs)
SHAPES = [(c, hw, n) for c, hw in ((320, 4096), (640, 1024), (1280, 256), (1280, 64))
          for n in (1, 2, 4, 11, 16, 22, 32, 44, 88)]


@pytest.mark.parametrize("c,hw,n", SHAPES)
def test_rowpanel_takes_agrees_with_the_route(ops, c, hw, n):
    rows = n * hw
    want = ops.rowpanel_takes(rows, hw, c, c)
    from diffcodec_amd import lib
    r = ops.conv_route(_desc(ops, rows, hw, c, c, gn_ab=16, gn_batch=n))
    assert (r.kernel == "gemm_rowpanel") == want, (c, hw, n, r)
    # blocks.py asks for the statistics epilogue together with the affine on load exactly when the rule admits the shape; the
    # gather GEMM that takes the other shapes has no such epilogue, and the library refuses the combination there
    d = _desc(ops, rows, hw, c, c, gn_ab=16, gn_batch=n, stats_out=16)
    if want:
        assert ops.conv_route(d).kernel == "gemm_rowpanel"
    else:
        with pytest.raises(lib.HipLaunchError):
            ops.conv_route(d)
    for extra in ({}, {"stats_out": 16}):                    # the same GEMM without the affine on load
        r = ops.conv_route(_desc(ops, rows, hw, c, c, **extra))
        assert (r.kernel == "gemm_rowpanel") == want, (c, hw, n, extra, r)


@pytest.mark.parametrize("extra", [dict(residual=16), dict(stats_out=16), dict(row_add=16), dict(act=1)])
def test_folded_layernorm_partials_route_finalizes_first(ops, extra):
    """K = 320, M = 65536 with raw LayerNorm partials and an epilogue the row-panel kernel does not specialise: the library
    finalizes first (needs ln_scratch); the plain form stays on the row-panel kernel, which finalizes in its prologue."""
    r = ops.conv_route(_desc(ops, 65536, 4096, 320, 320, ln_stats=16, ln_colsum=16, ln_parts=4, **extra))
    assert r.ln_first and r.kernel != "gemm_rowpanel", r
    r = ops.conv_route(_desc(ops, 65536, 4096, 320, 320, ln_stats=16, ln_colsum=16, ln_parts=4))
    assert not r.ln_first and r.kernel == "gemm_rowpanel", r


def test_route_reports_the_split_k_fixpoint_and_refuses_invalid_descriptors(ops):
    from diffcodec_amd import lib
    # 3x3 stride-2 gather GEMM, K = 9 * 20 steps: split 7 owns ceil(180/7) = 26 steps -> 7 splits; 19 -> 10 steps each -> 18
    d = _desc(ops, 32 * 32, 32 * 32, 1280, 1280, ksize=3, stride=2, pad=1, N=1, H=64, W=64, Ho=32, Wo=32, splitk=19)
    r = ops.conv_route(d)
    assert r.kernel == "igemm" and r.splitk == 18, r
    with pytest.raises(lib.HipLaunchError):
        ops.conv_route(_desc(ops, 4096, 4096, 320, 320, Cout=330))
