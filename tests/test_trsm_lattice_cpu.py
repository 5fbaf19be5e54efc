"""Line-sweep triangular solve on the CPU: which lattice plans are eligible (`_lattice.trsm_tables`) and — by walking every row of
every eligible case the way csrc/sptrsm_lattice.hip does, lines in ticket order — that the tables lead to exactly the column and
value position the CSR arrays name, in the order the sync-free kernel visits them, and that every dependency the sweep uses is
solved before it is needed: on the same line at an earlier step, or on a line with a smaller ticket."""

import numpy as np
import pytest
import torch

import _lattice_ref as ref
from torchsparsegradutils_amd import _lattice as lt
from torchsparsegradutils_amd import _pattern as pt
from torchsparsegradutils_amd.utils import synthetic


def _block_diag(crow, col, n1, nb):
    crow, col = crow.long(), col.long()
    crows = [crow[:1]] + [crow[1:] + b * col.numel() for b in range(nb)]
    cols = [col + b * n1 for b in range(nb)]
    return torch.cat(crows).to(torch.int32), torch.cat(cols).to(torch.int32)


def _pattern(shape, points=27, part=None, periodic=False, nb=1):
    crow, col = synthetic.box_stencil(*shape, periodic=(periodic,) * 3, points=points, part=part)
    n1 = shape[0] * shape[1] * shape[2]
    if nb > 1:
        crow, col = _block_diag(crow, col, n1, nb)
    return crow, col, nb * n1


def _plans(crow, col, n, dims):
    """(stored-order plan, its RowGather, kind-1 plan of the transposed walk, the transposed RowGather)."""
    g = pt.RowGather(crow, col, n, n)
    plan = ref.build_lattice_plan(g, dims=dims)
    assert plan is not None and plan.kind == 0
    t = g.transposed
    tplan = ref.build_lattice_plan(t, value_crow=crow, dims=dims)
    assert tplan is not None and tplan.kind == 1
    return plan, g, tplan, t


def _emulate(plan, tables, lower, crow, col, perm, value_crow):
    """Walk the lines in ticket order and every row's records in the kernel's visiting order.  `crow` / `col` / `perm`: the
    row-gather arrays the sync-free kernel would walk for the same solve (perm None: stored order); `value_crow`: A's row pointer.
    Returns (entries checked, entries the sweep uses)."""
    nb, nx, ny, nz = plan.nb, plan.nx, plan.ny, plan.nz
    nlines = nb * nx * ny
    assert tables.struct.nlines == nlines and tables.struct.nz == nz and tables.struct.kind == plan.kind
    assert tables.struct.width == plan.recw and tables.struct.uniform_len == plan.uniform_len and tables.struct.ncls == plan.ncls
    assert 1 <= tables.front_lines <= nlines
    tab = tables.tab_host
    rcls = plan.rcls.numpy()
    lens = plan.lens.numpy()
    rstart = plan.rstart.numpy().astype(np.int64)
    crow, col = crow.numpy().astype(np.int64), col.numpy().astype(np.int64)
    value_crow = value_crow.numpy().astype(np.int64)
    used_bit = lt.TRSM_USED_LOWER if lower else lt.TRSM_USED_UPPER
    solved_at = np.full(plan.n_rows, -1, dtype=np.int64)      # (ticket, step) order in which rows are published
    clock = 0
    checked = used = 0
    for ticket in range(nlines):
        line = ticket if lower else nlines - 1 - ticket
        for step in range(nz):
            z = step if lower else nz - 1 - step
            row = line * nz + z
            cls = rcls[row]
            length = int(lens[cls])
            s, e = crow[row], crow[row + 1]
            assert e - s == length
            for k in range(length):
                off, info = int(tab[cls, k, 0]), int(tab[cls, k, 1])
                j = row + off
                at = s + k                                     # the k-th entry the sync-free kernel meets in this row
                assert j == col[at], (row, k, j, col[at])
                src = j if plan.kind == 1 else row
                start = src * plan.uniform_len if plan.uniform_len else rstart[src]
                vpos = start + (info & 0xFF)
                assert start == value_crow[src]
                assert vpos == (perm[at] if perm is not None else at), (row, k)
                assert bool(info & lt.TRSM_DIAG) == (j == row)
                want_used = j < row if lower else j > row
                assert bool(info & used_bit) == want_used
                if want_used:
                    used += 1
                    same_line = j // nz == line
                    assert bool(info & lt.TRSM_INLINE) == same_line
                    if same_line:
                        assert abs(off) in (1, 2) and solved_at[j] == clock - abs(off)      # one of the wave's last two solutions
                    else:
                        tj = j // nz if lower else nlines - 1 - j // nz
                        assert tj < ticket and solved_at[j] >= 0
                checked += 1
            solved_at[row] = clock
            clock += 1
    return checked, used


ELIGIBLE = [
    # (shape, points, part, nb, sweeps of the stored-order plan that must be eligible)
    ((5, 6, 7), 27, "lower", 1, (True,)),
    ((5, 6, 7), 27, "strict_lower", 1, (True,)),
    ((4, 5, 6), 7, "lower", 1, (True,)),
    ((4, 5, 6), 27, None, 1, (True, False)),           # the whole truncated box, asked for as lower and as upper
    ((5, 4, 6), 27, "upper", 1, (False,)),
    ((4, 5, 6), 27, "lower", 2, (True,)),              # block diagonal
]


@pytest.mark.parametrize("shape,points,part,nb,sweeps", ELIGIBLE)
def test_eligible_factors_and_the_kernel_addressing(shape, points, part, nb, sweeps):
    crow, col, n = _pattern(shape, points, part, nb=nb)
    plan, g, tplan, t = _plans(crow, col, n, (nb,) + shape)
    for lower in sweeps:
        tables = lt.trsm_tables(plan, lower)
        assert tables is not None and tables.lower == lower
        checked, used = _emulate(plan, tables, lower, crow, col, None, crow)
        assert checked == col.numel() and used > 0
        # both sweeps of the transposed walk: op(A) = Aᵀ flips the triangle
        ttables = lt.trsm_tables(tplan, not lower)
        assert ttables is not None
        checked, used_t = _emulate(tplan, ttables, not lower, t.crow, t.col, t.perm.numpy().astype(np.int64), crow)
        assert checked == col.numel() and used_t == used
    if part in ("lower", "strict_lower"):
        # a lower factor asked for as upper uses no entry at all: still a valid (diagonal) sweep
        up = lt.trsm_tables(plan, False)
        assert up is not None and _emulate(plan, up, False, crow, col, None, crow)[1] == 0


def test_front_lines_of_the_27_point_half():
    """The launch rule: about ny·nz / 4 lines of a 27-point half are in flight together (level = 4x + 2y + z); 7-point: x + y + z."""
    assert lt._front_lines(1, 64, 64, 64, 4, 2) == pytest.approx(64 * 64 / 4, rel=0.3)
    crow, col, n = _pattern((6, 6, 6), 27, "lower")
    plan = ref.build_lattice_plan(pt.RowGather(crow, col, n, n), dims=(1, 6, 6, 6))
    assert lt.trsm_tables(plan, True).front_lines == lt._front_lines(1, 6, 6, 6, 4, 2)
    crow, col, n = _pattern((6, 6, 6), 7, "lower")
    plan = ref.build_lattice_plan(pt.RowGather(crow, col, n, n), dims=(1, 6, 6, 6))
    assert lt.trsm_tables(plan, True).front_lines == lt._front_lines(1, 6, 6, 6, 1, 1)


def test_periodic_triangular_parts_are_not_eligible():
    # by displacement: the lower half of a periodic box wraps above the diagonal at the faces (and those rows' used entries wrap too)
    crow, col, n = _pattern((4, 5, 6), 27, "lower", periodic=True)
    plan, g, tplan, t = _plans(crow, col, n, (1, 4, 5, 6))
    assert lt.trsm_tables(plan, True) is None and lt.trsm_tables(plan, False) is None
    assert lt.trsm_tables(tplan, True) is None and lt.trsm_tables(tplan, False) is None
    # by position: tril of the periodic box — the used entries of the face rows wrap
    crow, col, n = _pattern((4, 5, 6), 27, None, periodic=True)
    rows = torch.repeat_interleave(torch.arange(n), (crow[1:] - crow[:-1]).long())
    keep = col.long() <= rows
    lcrow = torch.zeros(n + 1, dtype=torch.int32)
    lcrow[1:] = torch.cumsum(torch.bincount(rows[keep], minlength=n), 0)
    plan = ref.build_lattice_plan(pt.RowGather(lcrow, col[keep].contiguous(), n, n), dims=(1, 4, 5, 6))
    assert plan is not None
    assert lt.trsm_tables(plan, True) is None


def test_a_banded_random_factor_gets_no_lattice_plan():
    crow, col, _ = synthetic.banded_lower(4096, per_row=6, band=64)
    assert ref.build_lattice_plan(pt.RowGather(crow, col, 4096, 4096)) is None
    assert lt.trsm_tables(None, True) is None
