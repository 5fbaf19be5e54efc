"""Every header under include/ against `_backend.ABI`, the library and the build, without a GPU: one case per header.

`_backend.ABI` maps each header to its ctypes table and is all that `load_library` binds; a header that is missing there would
load with ctypes' default `int` signatures and show as stack garbage on the GPU only.  The tables below are literal on purpose:
a new header adds one row ("Adding a header").
"""

import ctypes
import os
import re

import pytest

import _abi_cases as A
from torchsparsegradutils_amd import _backend

ROOT = os.path.dirname(A.INCLUDE)
FIRST = "tsgu_hip.h"

# header -> (its table in _backend, its entries in declaration order, how many of the first are host-only queries: the rest are
# launchers).  The first header is not additive: its table keeps the order it grew in, and its launchers are found by their last
# two parameters (_abi_cases.LAUNCHERS, literal in test_abi_refusals_cpu.py).
HEADERS = {
    FIRST: ("SIGNATURES", None, None),
    "tsgu_hip_softmax.h": (
        "SIGNATURES_SOFTMAX", ("tsgu_segment_softmax_workspace", "tsgu_segment_softmax", "tsgu_segment_softmax_backward"), 1),
    "tsgu_hip_attention.h": (
        "SIGNATURES_ATTENTION", ("tsgu_csr_attention_supported", "tsgu_csr_attention_geometry", "tsgu_csr_attention",
                                 "tsgu_csr_attention_backward_rows", "tsgu_csr_attention_backward_cols"), 2),
    "tsgu_hip_mm_reduce.h": (
        "SIGNATURES_MM_REDUCE", ("tsgu_csr_spmm_reduce_geometry", "tsgu_csr_spmm_reduce", "tsgu_csr_spmm_reduce_backward_values",
                                 "tsgu_csr_spmm_reduce_backward_dense"), 1),
    "tsgu_hip_spgemm.h": (
        "SIGNATURES_SPGEMM", ("tsgu_spgemm_bins", "tsgu_spgemm_row_bound", "tsgu_spgemm_symbolic", "tsgu_spgemm_numeric",
                              "tsgu_spgemm_grad_a", "tsgu_spgemm_grad_b"), 1),
    "tsgu_hip_bsr.h": ("SIGNATURES_BSR", ("tsgu_bsr_mm_geometry", "tsgu_bsr_spmm", "tsgu_bsr_sddmm", "tsgu_bsr_spmm_t"), 1),
    "tsgu_hip_bsr_attention.h": (
        "SIGNATURES_BSR_ATTENTION", ("tsgu_bsr_attention_supported", "tsgu_bsr_attention_geometry", "tsgu_bsr_attention",
                                     "tsgu_bsr_attention_backward_rows", "tsgu_bsr_attention_backward_cols"), 2),
    "tsgu_hip_factor.h": (
        "SIGNATURES_FACTOR", ("tsgu_csr_factor_work_bytes", "tsgu_csr_factor_geometry", "tsgu_csr_ilu0", "tsgu_csr_ic0"), 2),
    "tsgu_hip_fsai.h": ("SIGNATURES_FSAI", ("tsgu_csr_fsai_geometry", "tsgu_csr_fsai"), 1),
}

# (header, word): no entry of the header has the word in its name — an op's entries live in the op's own header
ABSENT = [
    ("tsgu_hip.h", "softmax"),
    ("tsgu_hip.h", "attention"), ("tsgu_hip_softmax.h", "attention"),
    ("tsgu_hip.h", "spmm_reduce"), ("tsgu_hip_softmax.h", "spmm_reduce"), ("tsgu_hip_attention.h", "spmm_reduce"),
    ("tsgu_hip.h", "spgemm"), ("tsgu_hip_softmax.h", "spgemm"), ("tsgu_hip_attention.h", "spgemm"), ("tsgu_hip_mm_reduce.h", "spgemm"),
    ("tsgu_hip.h", "bsr"), ("tsgu_hip_softmax.h", "bsr"), ("tsgu_hip_attention.h", "bsr"), ("tsgu_hip_mm_reduce.h", "bsr"),
    ("tsgu_hip_spgemm.h", "bsr"),
    ("tsgu_hip.h", "bsr_attention"), ("tsgu_hip_softmax.h", "bsr_attention"), ("tsgu_hip_attention.h", "bsr_attention"),
    ("tsgu_hip_mm_reduce.h", "bsr_attention"), ("tsgu_hip_spgemm.h", "bsr_attention"), ("tsgu_hip_bsr.h", "bsr_attention"),
]

PROTOS = {h: A.prototypes(h) for h in HEADERS}


def _text(*path):
    return open(os.path.join(ROOT, *path)).read()


def test_every_header_is_registered_once():
    assert set(os.listdir(A.INCLUDE)) == set(_backend.ABI) == set(HEADERS)
    for header, table in _backend.ABI.items():
        assert getattr(_backend, HEADERS[header][0]) is table, header
    names = [n for h in HEADERS for n, _ in PROTOS[h]]
    assert len(names) == len(set(names)), "an entry is declared in two headers"
    assert sum(len(t) for t in _backend.ABI.values()) == len(names)


@pytest.mark.parametrize("header", list(HEADERS))
def test_the_entries_are_exported_and_are_the_tables_keys(header):
    table = _backend.ABI[header]
    declared = [n for n, _ in PROTOS[header]]
    raw = ctypes.CDLL(_backend.LIB_PATH)
    for name in declared:
        assert hasattr(raw, name), f"{name} is declared in include/{header} but not exported by libtsgu_hip.so"
    assert set(declared) == set(table)
    _, entries, _ = HEADERS[header]
    if header == FIRST:
        assert len(declared) >= 40
        # every name the text calls, comments included, is an entry
        mentioned = set(re.findall(r"\b(tsgu_[a-z0-9_]+)\s*\(", _text("include", header)))
        assert len(mentioned) >= 15 and mentioned == set(table)
    else:
        assert tuple(table) == entries and declared == list(entries)


@pytest.mark.parametrize("header", list(HEADERS))
def test_load_library_binds_the_tables_signatures(header):
    lib = _backend.load_library()
    for name, (restype, argtypes) in _backend.ABI[header].items():
        assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype == restype, name


@pytest.mark.parametrize("header", list(HEADERS))
def test_ctypes_signatures_agree_with_the_header_prototypes(header):
    """The same number of parameters, and for each one the same class (pointer / 64-bit integer / int / double) — a mismatch
    would only show as stack garbage on the GPU box.  The launchers end in (device, stream)."""
    table = _backend.ABI[header]
    for name, params in PROTOS[header]:
        want = [A.klass_of_decl(t) for _, t in params]
        got = [A.klass_of_ctype(t) for t in table[name][1]]
        assert got == want, (name, got, want)
    _, entries, queries = HEADERS[header]
    protos = dict(PROTOS[header])
    for name in entries[queries:] if entries else ():
        assert protos[name][-2:] == [("device", "int"), ("stream", "void*")], name


@pytest.mark.parametrize("header,word", ABSENT)
def test_an_ops_entries_live_in_its_own_header(header, word):
    assert not any(word in n for n, _ in PROTOS[header])


def test_the_abi_version():
    assert _backend.load_library().tsgu_abi_version() == 7 == _backend.ABI_VERSION
    assert "TSGU_ABI_VERSION 7" in _text("include", FIRST)


@pytest.mark.parametrize("header", list(HEADERS))
def test_the_build_knows_the_header(header):
    if header != FIRST:
        assert '#include "tsgu_hip.h"' in _text("include", header)
    # every object is rebuilt when the header changes: the rule names it, or all of include/
    rule = re.search(r"^%\.o:.*(?:\\\n.*)*", _text("torchsparsegradutils_amd", "csrc", "Makefile"), flags=re.M).group(0)
    assert header in rule or "$(wildcard ../../include/*.h)" in rule
