"""CPU: the host-side rows of tests/golden/f32_mfma_bits.json (tools/record_f32_bits.py): the bytes of the three weight packers and
of `fold_and_pack` on seeded state dicts, and what the workspace planners and dc_*_weight_floats return over a grid of arguments
that includes the refused ones.  Recorded before the fp32 MFMA core was shared (csrc/dc_f32_mfma.h, metrics._PackedNet); a
mismatch means a refactor changed a layout, a rounding or an alignment."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, "tools"))

import record_f32_bits as B  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    with open(B.GOLDEN) as fh:
        return json.load(fh)


def test_golden_holds_exactly_the_recorders_cases(golden):
    assert sorted(golden) == sorted(list(B.CPU_CASES) + list(B.GPU_CASES))
    assert not set(B.CPU_CASES) & set(B.GPU_CASES)


@pytest.mark.parametrize("name", list(B.CPU_CASES))
def test_cpu_row(golden, name):
    assert B.run(name) == golden[name], name
