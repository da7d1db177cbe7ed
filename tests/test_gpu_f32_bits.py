"""GPU: the bits of csrc/lpips.hip, fid.hip, fvd.hip and cmp.hip against tests/golden/f32_mfma_bits.json (sha256 of the output
bytes per case, tools/record_f32_bits.py): every conv seam on the smallest shapes that reach each mask and template instance, the
four networks end to end, and one case per family with a NaN and an inf in its input.  The fp64 comparisons of
tests/test_gpu_{lpips,fid,fvd,cmp}.py would pass a reordered sum; this does not.  A mismatch means the arithmetic changed: fix the
code, do not record again."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, "tools"))

import record_f32_bits as B  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with open(B.GOLDEN) as fh:
        return json.load(fh)


@pytest.mark.parametrize("name", list(B.GPU_CASES))
def test_bits(golden, name):
    assert B.run(name) == golden[name], name
