"""The structural log-sum-exp cases without a GPU: their constants against the kernel sources, the events the coverage model
reports for every value type, the needle arithmetic, and the fp64 cases through the CPU operand path against float64."""

import os
import re

import numpy as np
import pytest
import torch

import _lse_cases
import _lse_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "torchsparsegradutils_amd", "csrc")


def _const(text, name):
    m = re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*(\d+)\s*;", text)
    assert m, name
    return int(m.group(1))


def test_constants_match_the_kernel_sources():
    impl = open(os.path.join(CSRC, "logsumexp_impl.h")).read()
    assert _const(impl, "kLseStageBytes") == _lse_cases.STAGE_BYTES
    assert _const(impl, "kLseLaneMax") == _lse_cases.LANE_MAX
    assert _const(impl, "kLseBwdWindow") == _lse_cases.BWD_WINDOW
    assert re.search(r"lse_range\(\)\s*\{\s*return\s+kLseStageBytes\s*/\s*\(int\)sizeof\(Acc\)", impl)
    common = open(os.path.join(CSRC, "tsgu_common.h")).read()
    for ctype, name in (("float", "float32"), ("double", "float64"), ("bf16_t", "bfloat16")):
        m = re.search(r"struct\s+VT<" + ctype + r">\s*\{(.*?)\n\};", common, re.S)
        assert m, ctype
        assert _const(m.group(1), "kWide") == _lse_cases.K_WIDE[name], name
        acc = re.search(r"using\s+Acc\s*=\s*(\w+)\s*;", m.group(1)).group(1)
        assert {"float": 4, "double": 8}[acc] == _lse_cases.ACC_BYTES[name], name
    assert [_lse_cases.range_len(d) for d in _lse_cases.DTYPES] == [2048, 1024, 2048]
    assert [_lse_cases.span_len(d) for d in _lse_cases.DTYPES] == [256, 128, 512]


@pytest.mark.parametrize("dtype", _lse_cases.DTYPES)
def test_every_structural_event_is_hit(dtype):
    seen = set()
    for _, ptr, v in _lse_cases.structural_cases(dtype):
        assert ptr[0] == 0 and (np.diff(ptr) >= 0).all() and v.size == ptr[-1]
        seen |= _lse_cases.events(ptr, dtype)
    assert set(_lse_cases.EVENTS) - seen == set(), dtype
    # the needle cases alone reach every event but the value-independent nnz = 0 one
    needles = set()
    for name, ptr, _ in _lse_cases.structural_cases(dtype):
        if name.endswith("_needles"):
            needles |= _lse_cases.events(ptr, dtype)
    assert set(_lse_cases.EVENTS) - needles == set(), dtype


def test_coverage_model_on_hand_made_pointers():
    R = _lse_cases.range_len("float32")
    # a group of exactly R entries; groups of 10 and R − 10 (ending on 2R); an empty group at 2R; a group over three ranges
    ptr = np.array([0, R, R + 10, 2 * R, 2 * R, 4 * R + 3], dtype=np.int64)
    m = _lse_cases.forward_model(ptr, R)
    assert len(m) == 5
    assert m[0][2:4] == (0, 1) and m[0][4] is None and m[0][5] == -1
    assert m[1][2:4] == (1, 3) and m[1][5] == -1                         # groups 1, 2 owned; group 2 ends on 2R
    assert m[2][2:4] == (3, 5) and m[2][5] == 4                          # the empty group 3 at 2R, then group 4's tail
    assert m[3][4] == 3 * R + R and m[3][2] == 5                         # head-only range, ga == n_groups
    assert m[4][4] == 4 * R + 3
    ev = _lse_cases.events(ptr, "float32")
    assert {"range_exact_group", "wide_ends_on_range_end", "empty_at_range_start", "head_only_range", "ga_is_n_groups",
            "wide_tail"} <= ev
    assert "merge_gt_64" not in ev and "bwd_unstaged" not in ev
    assert list(_lse_cases.pieces(ptr, R)) == [1, 1, 1, 1, 3]
    assert list(_lse_cases.backward_windows(np.array([0, 1] + [1] * 400 + [600]), 256)) == [403, 2, 2]   # r0 = 0, r1 = 401


def test_needles_outweigh_the_forward_bound():
    """A needle lost or counted twice moves its group by far more than the fp32 bound the GPU tests allow."""
    for dtype in ("float32", "bfloat16", "float64"):
        R = _lse_cases.range_len(dtype)
        for name, ptr, v in _lse_cases.structural_cases(dtype):
            if not name.endswith("_needles") or ptr[-1] == 0:
                continue
            for axis in (None, _lse_cases.axis_len_of(ptr)):
                ref, k = _lse_ref.group_lse(ptr, v, axis)
                sens = _lse_cases.needle_sensitivity(ptr, v, axis)
                bound = _lse_ref.fwd_bound(ref, k, _lse_cases.pieces(ptr, R), 2.0 ** -23)
                has = np.diff(ptr) > 0                      # (inf: a group whose only terms are needles)
                assert (sens[has] >= 20 * bound[has]).all(), (dtype, name, float((sens[has] / bound[has]).min()))


def test_depth_bound_is_never_looser_than_the_term_count_bound():
    k = np.array([1, 10, 45, 1000, 1 << 20, 1_000_000], dtype=np.float64)
    p = np.array([1, 1, 1, 1, 512, 100], dtype=np.float64)
    lse = np.array([0.0, 3.0, -2.0, 10.0, 14.0, 13.8])
    eps = 2.0 ** -23
    b = _lse_ref.fwd_bound(lse, k, p, eps)
    assert (b <= (2 * k + 8) * eps + 4 * eps * np.abs(lse)).all()
    assert b[0] == (2 + 8) * eps                                          # short groups keep the term-count form
    assert b[4] < 2.5e-5                                                  # the 2^20-entry row: ≈ 2.1e-5, not 0.25


@pytest.mark.filterwarnings("ignore")
def test_fp64_structural_cases_on_the_cpu_path():
    """The fp64 cases through the public API on CPU tensors (CSR rows and CSC columns) against group_lse, forward and
    gradient: this pins the generator, the needle arithmetic and the reference the GPU tests use."""
    import torchsparsegradutils_amd as tsgu

    for name, ptr, v in _lse_cases.structural_cases("float64"):
        G, N = ptr.size - 1, _lse_cases.axis_len_of(ptr)
        idx = torch.from_numpy(_lse_cases.columns(ptr))
        grp = np.repeat(np.arange(G), np.diff(ptr))
        for iz in (False, True):
            ref, _ = _lse_ref.group_lse(ptr, v, N if iz else None)
            for layout in ("csr", "csc"):
                vals = torch.from_numpy(v.copy())
                if layout == "csr":
                    A = torch.sparse_csr_tensor(torch.from_numpy(ptr), idx, vals, (G, N))
                else:
                    A = torch.sparse_csc_tensor(torch.from_numpy(ptr), idx, vals, (N, G))
                A.requires_grad_(True)
                out = tsgu.sparse_logsumexp(A, 1 if layout == "csr" else 0, include_zeros=iz)
                got = out.detach().numpy()
                what = (name, layout, iz)
                assert np.array_equal(np.isnan(got), np.isnan(ref)), what
                assert np.array_equal(np.isposinf(got), np.isposinf(ref)) and np.array_equal(np.isneginf(got), np.isneginf(ref)), what
                fin = np.isfinite(ref)
                np.testing.assert_allclose(got[fin], ref[fin], rtol=1e-12, atol=1e-12, err_msg=str(what))
                gA, = torch.autograd.grad(out, A, torch.ones(G, dtype=torch.float64))
                with np.errstate(invalid="ignore", over="ignore"):
                    gref = np.exp(v - ref[grp])
                np.testing.assert_allclose(gA.values().numpy(), gref, rtol=1e-9, atol=1e-300, equal_nan=True, err_msg=str(what))
