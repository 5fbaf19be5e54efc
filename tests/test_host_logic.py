"""CPU-side checks: index helpers bit-exact vs the reference's golden outputs, validation messages,
the host-side helpers of the C-ABI library, and the product refuses CPU tensors."""

import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _golden as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same_sparse(S, z, prefix):
    if S.layout == torch.sparse_csr:
        assert np.array_equal(S.crow_indices().numpy(), z[prefix + "crow"])
        assert np.array_equal(S.col_indices().numpy(), z[prefix + "col"])
        assert np.array_equal(S.values().numpy(), z[prefix + "val"])
    else:
        assert np.array_equal(S._indices().numpy(), z[prefix + "idx"])
        assert np.array_equal(S._values().numpy(), z[prefix + "val"])


def test_convert_coo_to_csr_bit_exact():
    from torchsparsegradutils_amd.utils import convert_coo_to_csr

    z = G.load("utils_index.npz")
    A = G.sparse_from(z, "c2c_in_", (9, 7))
    _same_sparse(convert_coo_to_csr(A), z, "c2c_out_")
    Ab = G.sparse_from(z, "c2cb_in_", (3, 5, 4))
    _same_sparse(convert_coo_to_csr(Ab), z, "c2cb_out_")
    with pytest.raises(ValueError, match="Unsupported layout"):
        convert_coo_to_csr(torch.eye(3).to_sparse_csr())


@pytest.mark.parametrize("layout", ["coo", "csr"])
def test_block_diag_and_split_bit_exact(layout):
    from torchsparsegradutils_amd.utils import sparse_block_diag, sparse_block_diag_split

    z = G.load("utils_index.npz")
    shapes = [(3, 4), (2, 2), (4, 3)]
    blocks = [G.sparse_from(z, f"bd_{layout}_in{i}_", s) for i, s in enumerate(shapes)]
    D = sparse_block_diag(*blocks)
    assert D.shape == (9, 9)
    _same_sparse(D, z, f"bd_{layout}_out_")
    parts = sparse_block_diag_split(D, *shapes)
    for i, part in enumerate(parts):
        assert part.shape == shapes[i]
        _same_sparse(part, z, f"bd_{layout}_split{i}_")
    assert sparse_block_diag(blocks[0]) is blocks[0]  # single input returned unchanged (utils.py:566-567)
    with pytest.raises(ValueError, match="At least one sparse tensor must be provided."):
        sparse_block_diag()
    with pytest.raises(TypeError):
        sparse_block_diag(blocks[0], 3)
    with pytest.raises(ValueError, match="does not match"):
        sparse_block_diag_split(D, (3, 4), (2, 2))


def test_stack_csr_sparse_eye_and_row_helpers():
    from torchsparsegradutils_amd.utils import sparse_eye, stack_csr
    from torchsparsegradutils_amd.utils.utils import _compress_row_indices, _demcompress_crow_indices, _sort_coo_indices

    a = torch.tensor([[0.0, 1], [2, 0]]).to_sparse_csr()
    b = torch.tensor([[3.0, 0], [0, 4]]).to_sparse_csr()
    s = stack_csr([a, b])
    assert s.shape == (2, 2, 2) and torch.equal(s.to_dense(), torch.stack([a.to_dense(), b.to_dense()]))
    with pytest.raises(ValueError, match="Cannot stack empty list of tensors."):
        stack_csr([])
    with pytest.raises(TypeError):
        stack_csr(a)
    for layout in (torch.sparse_coo, torch.sparse_csr):
        for idt in (torch.int32, torch.int64):
            E = sparse_eye((3, 4, 4), layout=layout, values_dtype=torch.float32, indices_dtype=idt)
            assert torch.equal(E.to_dense(), torch.eye(4).expand(3, 4, 4))
    with pytest.raises(ValueError, match="square"):
        sparse_eye((3, 4))
    crow = torch.tensor([0, 2, 2, 5], dtype=torch.int32)
    rows = _demcompress_crow_indices(crow, 3)
    assert rows.dtype == torch.int32 and rows.tolist() == [0, 0, 2, 2, 2]
    assert torch.equal(_compress_row_indices(rows, 3), crow)
    idx = torch.tensor([[2, 0, 1, 0], [1, 3, 0, 1]])
    srt, perm = _sort_coo_indices(idx)
    ref = torch.sparse_coo_tensor(idx, torch.arange(4.0), (3, 4)).coalesce()
    assert torch.equal(srt, ref.indices()) and torch.equal(perm.float(), ref.values())


def test_validation_messages_match_reference():
    import torchsparsegradutils_amd as m

    E = G.errors()
    A = torch.eye(3).to_sparse_coo()
    B = torch.ones(3, 2)
    cases = {
        "mm_not_tensor": lambda: m.sparse_mm(A, 3),
        "mm_low_dim": lambda: m.sparse_mm(A, torch.ones(3)),
        "mm_dim_mismatch": lambda: m.sparse_mm(A, torch.ones(1, 3, 2)),
        "mm_csc": lambda: m.sparse_mm(torch.eye(3).to_sparse_csc(), B),
        "mm_dense_A": lambda: m.sparse_mm(torch.eye(3), B),
        "mm_sparse_B": lambda: m.sparse_mm(A, B.to_sparse_coo()),
        "mm_batch": lambda: m.sparse_mm(torch.stack([A, A]), torch.ones(3, 3, 2)),
        "mm_inner": lambda: m.sparse_mm(A, torch.ones(4, 2)),
        "tri_not_tensor": lambda: m.sparse_triangular_solve(A, None),
        "tri_low_dim": lambda: m.sparse_triangular_solve(A, torch.ones(3)),
        "tri_dim_mismatch": lambda: m.sparse_triangular_solve(A, torch.ones(1, 3, 2)),
        "tri_csc": lambda: m.sparse_triangular_solve(torch.eye(3).to_sparse_csc(), B),
        "tri_sparse_B": lambda: m.sparse_triangular_solve(A, B.to_sparse_coo()),
        "tri_not_square": lambda: m.sparse_triangular_solve(torch.ones(3, 4).to_sparse_coo(), B),
        "tri_inner": lambda: m.sparse_triangular_solve(A, torch.ones(4, 2)),
        "tri_batch": lambda: m.sparse_triangular_solve(torch.stack([A, A]), torch.ones(3, 3, 2)),
        "gs_not_tensor": lambda: m.sparse_generic_solve(A, 1.0),
        "gs_layout": lambda: m.sparse_generic_solve(torch.eye(3), B),
        "gs_dim": lambda: m.sparse_generic_solve(torch.stack([A, A]), B),
        "gs_square": lambda: m.sparse_generic_solve(torch.ones(3, 4).to_sparse_coo(), B),
        "gs_B_dim": lambda: m.sparse_generic_solve(A, torch.ones(3, 2, 2)),
        "gs_incompatible": lambda: m.sparse_generic_solve(A, torch.ones(4, 2)),
        "gs_B_sparse": lambda: m.sparse_generic_solve(A, B.to_sparse_coo()),
    }
    for name, fn in cases.items():
        want = E[name]
        assert want["type"] in ("ValueError", "TypeError"), name
        with pytest.raises(Exception) as e:
            fn()
        assert type(e.value).__name__ == want["type"], name
        assert str(e.value) == want["msg"], name
    # dtype mismatch only warns (reference sparse_solve.py:398-403); the solver's own product then raises torch's dtype error
    with pytest.warns(UserWarning) as w:
        with pytest.raises(RuntimeError, match="expected scalar type Float but found Double"):
            m.sparse_generic_solve(A, B.double())
    assert E["gs_dtype_warning"]["warnings"] == [str(w[0].message)]


def test_cpu_solvers_run_on_tensor_ops():
    """CPU operands of the Krylov entry points: the recurrences as tensor ops around the ATen product (the fused step kernels are
    the MI355X path and are never entered with a CPU tensor)."""
    from torchsparsegradutils_amd.utils import BICGSTABSettings, LinearCGSettings, MINRESSettings, bicgstab, linear_cg, minres

    A = (2 * torch.eye(3)).to_sparse_csr()
    B = torch.ones(3, 2)
    for fn in (lambda: linear_cg(A, B, settings=LinearCGSettings(cg_tolerance=1e-6)),
               lambda: bicgstab(A, B, settings=BICGSTABSettings()), lambda: minres(A, B, settings=MINRESSettings())):
        x = fn()
        assert not x.is_cuda and torch.allclose(x, torch.full((3, 2), 0.5))


def test_host_side_helpers_of_the_abi():
    """The entries that answer on the host (exports and signatures: tests/test_abi_conformance_cpu.py)."""
    from torchsparsegradutils_amd import _backend

    lib = _backend.load_library()  # loads without a GPU; no compute call is made here
    # row-pair geometry: (rows per workgroup, entry lanes) per (value type, p); unsupported shapes are refused
    r, e = ctypes.c_int(0), ctypes.c_int(0)
    for vt, p_, want in ((_backend.TSGU_F32, 32, (64, 1)), (_backend.TSGU_F32, 64, (32, 1)), (_backend.TSGU_F32, 16, (64, 2)),
                         (_backend.TSGU_F32, 8, (64, 4)), (_backend.TSGU_BF16, 16, (64, 4)), (_backend.TSGU_BF16, 128, (32, 1))):
        assert lib.tsgu_rowpack_geometry(vt, p_, ctypes.byref(r), ctypes.byref(e), None, None, None) == 0
        assert (r.value, e.value) == want, (vt, p_, r.value, e.value)
    assert lib.tsgu_rowpack_geometry(_backend.TSGU_F64, 32, None, None, None, None, None) != 0
    assert lib.tsgu_rowpack_geometry(_backend.TSGU_F32, 12, None, None, None, None, None) != 0
    assert lib.tsgu_status_string(-2).decode().startswith("bad argument")
    # pure host-side helpers of the ABI
    assert lib.tsgu_spmm_num_blocks(_backend.TSGU_F32, 10 ** 6, 27 * 10 ** 6, 32, 27) == 31250
    # 16-byte dense rows + short sparse rows: one lane per row, 256 rows per workgroup
    assert lib.tsgu_spmm_num_blocks(_backend.TSGU_F32, 2000376, 13907376, 4, 7) == 7814
    # the same operand with long rows keeps 8 entry lanes per row (32 rows per workgroup)
    assert lib.tsgu_spmm_num_blocks(_backend.TSGU_F32, 2000376, 40 * 2000376, 4, 0) == 62512
    # ragged: the same short-row operand with one very long row keeps 8 entry lanes per row as well
    assert lib.tsgu_spmm_num_blocks(_backend.TSGU_F32, 2000376, 13907376, 4, 5000) == 10419   # 32 rows x 6 runs per workgroup
    assert lib.tsgu_sptrsm_work_bytes(10, 1) >= 516


def test_launch_reports_the_symbol_it_called(monkeypatch):
    """`_backend.launch` raises under the name of the symbol it called.  tsgu_coldot refuses p = 0 with TSGU_ERR_BAD_ARG before
    it touches a device, so no kernel runs.  On a machine without a GPU torch cannot name a current device or stream: only there
    the two queries `launch` makes are answered with device 0 / the null stream; the library call itself is the real one."""
    from torchsparsegradutils_amd import _backend

    if not torch.cuda.is_available():
        monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
        monkeypatch.setattr(_backend, "_raw_stream", lambda dev: None)
    with pytest.raises(RuntimeError) as e:
        _backend.launch("tsgu_coldot", torch.device("cuda", 0), _backend.TSGU_F32, 8, 0, None, 0, None, 0, None, None)
    status = _backend.load_library().tsgu_status_string(-2).decode()
    assert "tsgu_coldot" in str(e.value) and status in str(e.value)


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "torchsparsegradutils_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, re.M), f
                assert "liboracle" not in src, f


def test_cpu_tensors_take_the_torch_op_path_and_mixed_devices_raise():
    """INTEGRATION.md, "CPU tensors": operands that live on the CPU are computed by the package's torch-op path (_cpu.py: the ATen
    calls the reference makes; tests/test_cpu_path.py pins it to the reference's golden vectors).  The switch is the operands'
    device only: the HIP bindings themselves refuse a CPU tensor, so nothing computed for a GPU caller can come from the CPU
    (test_product_never_imports_the_oracle keeps the oracle out of the package)."""
    import warnings

    import torchsparsegradutils_amd as m
    from torchsparsegradutils_amd import _backend

    A = (2 * torch.eye(4)).to_sparse_csr()
    B = torch.ones(4, 2)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for call in (lambda: m.sparse_mm(A, B),
                     lambda: m.sparse_mm((2 * torch.eye(4)).to_sparse_coo(), B),
                     lambda: 4 * m.sparse_triangular_solve(A, B, upper=False),
                     lambda: 4 * m.sparse_generic_solve(A, B, solve=m.utils.linear_cg),
                     lambda: 4 * m.linalg_solve_triangular_compat(A, B, upper=False)):
            out = call()
            assert not out.is_cuda and torch.allclose(out, torch.full((4, 2), 2.0))
    for fn in (_backend.csr_spmm, _backend.csr_sddmm):
        with pytest.raises(RuntimeError, match="gfx950 kernels"):
            fn(A.crow_indices(), A.col_indices(), A.values() if fn is _backend.csr_spmm else B, B, 4, 4)


def test_compat_dense_branch_is_the_reference_dispatch():
    """reference _compat.py:17-34: dense operands go to torch.linalg.solve_triangular, `transpose` as a transposed view with
    `upper` flipped — all eight flag combinations, and the keyword-only signature."""
    import inspect

    from torchsparsegradutils_amd import linalg_solve_triangular_compat

    sig = inspect.signature(linalg_solve_triangular_compat)
    assert [p.kind for p in sig.parameters.values()][2:] == [inspect.Parameter.KEYWORD_ONLY] * 3
    assert sig.parameters["unitriangular"].default is False and sig.parameters["transpose"].default is False
    g = torch.Generator().manual_seed(0)
    T = torch.randn(5, 5, generator=g, dtype=torch.float64) + 5 * torch.eye(5, dtype=torch.float64)
    B = torch.randn(5, 2, generator=g, dtype=torch.float64)
    for upper in (False, True):
        for unit in (False, True):
            for tr in (False, True):
                x = linalg_solve_triangular_compat(T, B, upper=upper, unitriangular=unit, transpose=tr)
                want = torch.linalg.solve_triangular(T.transpose(-2, -1) if tr else T, B, upper=(not upper) if tr else upper, unitriangular=unit)
                assert torch.equal(x, want)


def test_cpp_host_module_of_the_step_is_built_against_the_abi_library():
    """csrc/host/step.cpp (the steady-state sparse_mm step's host path as a torch C++ autograd function) is built by the same
    Makefile, links the C ABI library it launches through, and sparse_matmul picks it up; without a GPU nothing is launched."""
    import torchsparsegradutils_amd.sparse_matmul as sm
    from torchsparsegradutils_amd import _backend

    lib = _backend.load_library()
    assert sm._host is not None, "torchsparsegradutils_amd/_tsgu_host.so is missing: make -C torchsparsegradutils_amd/csrc"
    assert sm._host.abi_version() == lib.tsgu_abi_version()
    assert hasattr(sm._host, "StepPlan") and hasattr(sm._host, "step")
    # CPU tensors never reach it (the documented error of the package comes from the Python path)
    A = torch.eye(4).to_sparse_csr()
    assert sm._step_plan(A, torch.zeros(4, 16)) is None if torch.zeros(1).is_cuda else True
