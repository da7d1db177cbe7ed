"""CPU: every (header, table) pair of diffcodec_amd.lib.ABI agrees with its header in names, argument kinds and return types, the
built library exports every symbol bound as the table says, the families share no name, and the ctypes mirror of `dc_conv_desc`
has the header's fields in order and kind (no compute calls)."""
import pytest

import abi_check as A
from diffcodec_amd import lib

FAMILIES = pytest.mark.parametrize("header,table", lib.ABI, ids=[h for h, _ in lib.ABI])
TRAIN_NAMES = ("dc_silu_grad_f32", "dc_conv3x3_f32_dgrad", "dc_conv3x3_f32_wgrad", "dc_conv3x3_f32_wgrad_ws_bytes", "dc_conv3x3_f32_grad_route")


def test_every_table_of_the_binding_is_in_the_registry():
    """a table that lib.ABI does not list would be neither bound nor checked"""
    tables = {k: v for k, v in vars(lib).items() if k.endswith("SIGNATURES")}
    assert sorted(map(id, tables.values())) == sorted(id(t) for _, t in lib.ABI), sorted(tables)
    assert len(lib.signatures()) == sum(len(t) for _, t in lib.ABI) and len(lib.SIGNATURES) >= 25


@FAMILIES
def test_header_declares_what_the_binding_binds(header, table):
    """names, argument kinds and return types"""
    src = A.header_source(header)
    hdr = A.header_symbols(header)
    assert sorted(table) == hdr, set(hdr) ^ set(table)
    for name, args in table.items():
        got, want = A.binding_kinds(args), A.arg_kinds(src, name)
        assert got == want, (name, got, want)
        assert lib.restype_of(name) is A.RETURN_TYPES[A.return_kind(src, name)], (name, A.return_kind(src, name))


@FAMILIES
def test_library_exports_every_declared_symbol(header, table):
    l = A.built_lib().load()
    for name in A.header_symbols(header):
        assert hasattr(l, name), name
        fn = getattr(l, name)
        assert fn.argtypes == table[name], name
        assert fn.restype is lib.restype_of(name) is A.RETURN_TYPES[A.return_kind(A.header_source(header), name)], name


def test_families_share_no_name_and_keep_their_prefixes():
    pairs = [(h, set(A.header_symbols(h)), set(t)) for h, t in lib.ABI]
    for i, (h1, hdr1, tab1) in enumerate(pairs):
        for h2, hdr2, tab2 in pairs[i + 1:]:
            shared = (hdr1 | tab1) & (hdr2 | tab2)
            assert not shared, f"{sorted(shared)}: in both {h1} and {h2} (header or table)"
    for h, hdr, tab in pairs:
        for prefix, owner in (("dc_cmp_", "diffcodec_flow_hip.h"), ("dc_guide_", "diffcodec_guide_hip.h")):
            if h != owner:
                assert not [n for n in hdr | tab if n.startswith(prefix)], (h, prefix)
        if h != "diffcodec_train_hip.h":
            assert not set(TRAIN_NAMES) & (hdr | tab), h


def test_a_name_in_two_tables_is_refused(monkeypatch):
    name = next(iter(lib.SIGNATURES))
    monkeypatch.setattr(lib, "ABI", lib.ABI + (("diffcodec_new_hip.h", {name: []}),))
    with pytest.raises(ValueError, match=name):
        lib.signatures()


def test_conv_desc_layout_matches_header():
    """field order and field kinds of the ctypes mirror == those of `dc_conv_desc`: a 4-byte field bound as 8 bytes would shift
    every later field"""
    want = A.struct_fields(A.header_source("diffcodec_hip.h"), "dc_conv_desc")
    got = list(zip([f[0] for f in lib.ConvDesc._fields_], A.binding_kinds([f[1] for f in lib.ConvDesc._fields_])))
    assert len(want) == len(got) >= 30
    for g, w in zip(got, want):
        assert g == w, f"ConvDesc has {g} where dc_conv_desc has {w}"


def test_product_path_fails_loudly_without_the_library(monkeypatch):
    monkeypatch.setattr(lib, "_lib", None)
    monkeypatch.setattr(lib, "LIB_PATH", "/nonexistent/libdiffcodec_hip.so")
    with pytest.raises(lib.HipLibraryMissing):
        lib.load()
