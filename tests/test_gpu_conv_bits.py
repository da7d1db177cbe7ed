"""GPU: the bits of every routed bf16 GEMM / conv instance against tests/golden/conv_epilogue_bits.json (sha256 per case of
tests/edge_cases.py::CONV_CASES, tools/record_conv_bits.py): the output, the LayerNorm row statistics and the GroupNorm partials of
each case equal those of the build that preceded the shared epilogue of csrc/dc_epilogue.h.  The operand hash is compared first, so
a moved random stream is told apart from changed arithmetic.  A mismatch in an output means the arithmetic changed: fix the code, do
not record again."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, "tools"))

import edge_cases as E  # noqa: E402
import record_conv_bits as B  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with open(B.GOLDEN) as fh:
        return json.load(fh)


@pytest.mark.parametrize("i", range(len(E.CONV_CASES)), ids=[c.label() for c in E.CONV_CASES])
def test_conv_bits(golden, i):
    want, got = golden[B.name(i)], B.run(i)
    assert got["operands"] == want["operands"], f"{B.name(i)}: the operands differ from the recorded ones (the random stream moved)"
    assert sorted(got) == sorted(want), f"{B.name(i)}: outputs {sorted(got)}, recorded {sorted(want)}"
    for k in sorted(got):
        assert got[k] == want[k], f"{B.name(i)}: {k} differs from the recorded bits"
