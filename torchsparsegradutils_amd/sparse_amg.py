"""``sparse_amg`` — a smoothed-aggregation algebraic multigrid preconditioner (Vaněk, Mandel and Brezina, 1996) whose aggregates
come from a distance-2 maximal independent set (MIS-2; Bell, Dalton and Olson, 2012).

The one-level preconditioners of the package (``sparse_ilu0`` / ``sparse_ic0``, ``sparse_fsai``) cannot reach the low-frequency error
that costs a Krylov loop its iterations on elliptic problems; a multigrid cycle attacks exactly that error.  ``M(R)`` is one
V(``sweeps``, ``sweeps``) cycle from a zero guess with a damped-Jacobi smoother: pre- and post-smoothing are the same symmetric,
convergent iteration, so ``M`` is symmetric positive definite and is what ``linear_cg(preconditioner=…)``,
``minres(preconditioner=…)``, ``BICGSTABSettings.precon`` and ``sparse_lobpcg(preconditioner=…, largest=False)`` take.  The
reference package has no counterpart.

Two primitives carry everything that is not a torch op or a ``sparse_spgemm`` (``csrc/amg_impl.h``, C ABI in
``csrc/tsgu_hip_amg.h``; for CPU operands the torch-op forms of ``_cpu.py``, the same Python code above them):

``hop``      ``out[i] = max(in[i], max_{j in row i} in[j])`` over unsigned 64-bit keys on a CSR pattern: the MIS-2 rounds and the
             assignment of the nodes to their roots.  A max is exact, so the aggregates are a pure function of the pattern: the
             same on every run, for every lane-group width and every grid.
``affine``   ``Out = C + alpha·w∘(B − A·X)``: the residual, the Jacobi sweep, the restriction and the in-place prolongation are
             each ONE launch of it, on every level — from the second level down the rows are few and launch time decides.

Setup, per level from ``A_0 = A``: the strength filter (``theta``), MIS-2 aggregates, the tentative prolongator ``T`` (one entry
``1/sqrt(|aggregate|)`` per row), the smoothed prolongator ``P = (I − 4/(3ρ̂)·D⁻¹·A_F)·T``, the Galerkin product ``Pᵀ·(A·P)`` (three
``sparse_spgemm`` calls; ``Pᵀ`` through the cached transpose) and the smoother weights ``w = 4/(3ρ̂(A))/diag(A)`` with
``ρ̂(B) = max_i Σ_j |b_ij| / b_ii``, a device scalar.  The coarsest level is solved with its pseudo-inverse when it has at most
4096 rows, else smoothed.

No gradient flows through the hierarchy: it is built under ``no_grad`` on the detached operand, for the reasons given in
``sparse_factor``'s docstring — a preconditioner changes how fast a Krylov loop reaches the solution, not the solution.
"""

from __future__ import annotations

import warnings

import torch

from . import _backend as _be
from . import _pattern as _pt
from .sparse_factor import _Factor, _operand
from .sparse_spgemm import _numeric, _Operand, _plan_for, sparse_spgemm

__all__ = ["sparse_amg", "SparseAMG"]

DENSE_COARSE_MAX = 4096      # the largest coarsest level that is solved with its pseudo-inverse
_POLL_ROUNDS = 4             # MIS-2 rounds between two reads of the "still undecided" word


def _primitives(t: torch.Tensor):
    """(hop, mis2_update, affine) for the device of `t`: the HIP launchers, or their torch-op forms for CPU operands."""
    if t.is_cuda:
        return _be.amg_hop, _be.amg_mis2_update, _be.csr_affine_spmm
    from . import _cpu

    return _cpu.amg_hop, _cpu.amg_mis2_update, _cpu.csr_affine_spmm


def _group_width(n: int, nnz: int, device) -> int:
    """Lanes per row of the hop: the narrowest accepted width that covers the average row (the torch-op form has none: 0)."""
    if device.type != "cuda":
        return 0
    widths = _be.amg_geometry()[0]
    for w in widths:
        if w * max(n, 1) >= nnz:
            return w
    return widths[-1]


def _rows_of(ptr: torch.Tensor, nnz: int) -> torch.Tensor:
    n = ptr.numel() - 1
    return torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=ptr.device), (ptr[1:] - ptr[:-1]).to(torch.int64),
                                   output_size=nnz)


def _mis2_aggregate(ptr: torch.Tensor, idx: torch.Tensor, n: int, group: int = None):
    """(aggregate of every node as int64, number of aggregates) of a CSR pattern: MIS-2 roots by rounds of two hops and a node
    update, then every node joins the root with the largest key within distance 1, else within distance 2; aggregates are
    numbered by their roots' ascending index.  `group`: lanes per row of the hop (None: from nnz / n; the result is the same)."""
    hop, update, _ = _primitives(idx)
    dev = idx.device
    group = _group_width(n, idx.numel(), dev) if group is None else int(group)
    key = update(_be.AMG_INIT, n, device=dev)
    t1, t2 = torch.empty_like(key), torch.empty_like(key)
    undecided = torch.zeros((), dtype=torch.int64, device=dev)
    rounds = 0
    while True:
        for _ in range(_POLL_ROUNDS):       # (a round with nothing undecided changes nothing: polling every few rounds is exact)
            hop(ptr, idx, key, n, group, out=t1)
            hop(ptr, idx, t1, n, group, out=t2)
            undecided.zero_()
            update(_be.AMG_ROUND, n, key=key, t=t2, out=key, undecided=undecided)
        rounds += _POLL_ROUNDS
        if not int(undecided.item()):
            break
        if rounds > n + _POLL_ROUNDS:       # (every round decides at least the undecided node with the largest key)
            raise RuntimeError("sparse_amg: the MIS-2 rounds did not finish")
    roots = update(_be.AMG_ROOTS, n, key=key, out=t1)
    a1 = hop(ptr, idx, roots, n, group, out=t2)
    a2 = hop(ptr, idx, a1, n, group)
    near = torch.where(a1 != 0, a1, a2) & 0xFFFFFFFF
    is_root = roots != 0
    rank = torch.cumsum(is_root, 0) - 1
    agg = rank.index_select(0, near).clamp_(min=0)
    return agg, int(is_root.sum().item())


class _Level:
    """One level of the hierarchy: the CSR arrays of ``A_l`` and, unless it is the coarsest, what leads to the next one."""

    def __init__(self, ptr, idx, val, n: int):
        self.ptr, self.idx, self.val, self.n = ptr, idx, val, n
        self.rows = _rows_of(ptr, idx.numel())
        self.diag_pos = torch.nonzero(self.rows == idx.to(torch.int64)).reshape(-1)
        self.theta = None
        self.n_c = 0
        self.agg = None
        self.solver = None
        self.w = self.inv = self.P = self.PT = None
        self._products = {}

    @property
    def nnz(self) -> int:
        return self.idx.numel()

    def tensor(self, val=None) -> torch.Tensor:
        return torch.sparse_csr_tensor(self.ptr, self.idx, self.val if val is None else val, (self.n, self.n))

    def row_sums(self, ptr, idx, val) -> torch.Tensor:
        """Σ_j val_ij per row of a pattern of this level, in entry order (the affine product with a column of ones)."""
        ones = torch.ones((self.n, 1), dtype=val.dtype, device=val.device)
        return _primitives(val)[2](ptr, idx, val, ones, self.n, self.n, alpha=-1.0).reshape(-1)

    # ---- symbolic: the strength pattern and the aggregates ----------------------------------------------------------------------
    def coarsen(self, theta: float) -> bool:
        """Choose the strength pattern at `theta` and aggregate it; False when the level does not coarsen by a factor of two."""
        self.theta = float(theta)
        if theta > 0:
            d = self.val.index_select(0, self.diag_pos)
            col = self.idx.to(torch.int64)
            bound = theta * torch.sqrt(torch.abs(d.index_select(0, self.rows) * d.index_select(0, col)))
            keep = (self.rows == col) | (torch.abs(self.val) >= bound)
            self.f_pos = torch.nonzero(keep).reshape(-1)
            self.f_rows = self.rows.index_select(0, self.f_pos)
            self.f_idx = self.idx.index_select(0, self.f_pos).contiguous()
            self.f_ptr = torch.zeros(self.n + 1, dtype=self.ptr.dtype, device=self.ptr.device)
            self.f_ptr[1:] = torch.cumsum(torch.bincount(self.f_rows, minlength=self.n), 0)
            self.f_diag_pos = torch.nonzero(self.f_rows == self.f_idx.to(torch.int64)).reshape(-1)
        else:
            self.f_pos = None
            self.f_rows, self.f_ptr, self.f_idx, self.f_diag_pos = self.rows, self.ptr, self.idx, self.diag_pos
        self.agg, self.n_c = _mis2_aggregate(self.f_ptr, self.f_idx, self.n)
        if 2 * self.n_c > self.n:
            return False
        self.t_ptr = torch.arange(self.n + 1, dtype=self.ptr.dtype, device=self.ptr.device)
        self.t_idx = self.agg.to(self.idx.dtype)
        self.t_count = torch.bincount(self.agg, minlength=self.n_c)
        return True

    # ---- numeric: everything that depends on the values -------------------------------------------------------------------------
    def filtered_values(self) -> torch.Tensor:
        if self.f_pos is None:
            return self.val
        dropped = self.val.clone()
        dropped[self.f_pos] = 0
        fval = self.val.index_select(0, self.f_pos)
        fval[self.f_diag_pos] += self.row_sums(self.ptr, self.idx, dropped)       # A_F keeps A's row sums
        return fval

    def _omega(self, ptr, idx, val, diag) -> torch.Tensor:
        """4 / (3·ρ̂) with ρ̂ = max_i Σ_j |b_ij| / b_ii: a device scalar."""
        rho = (self.row_sums(ptr, idx, torch.abs(val)) / diag).max()
        return 4.0 / (3.0 * rho)

    def smoother(self) -> None:
        d = self.val.index_select(0, self.diag_pos)
        self.w = self._omega(self.ptr, self.idx, self.val, d) / d

    def galerkin(self, keep=None) -> "_Level":
        """P_l and the next level A_{l+1} = P_lᵀ·(A_l·P_l).  `keep`: the next level of an earlier build on the same pattern, whose
        index tensors (and everything derived from them) are kept while its values are replaced."""
        fval = self.filtered_values()
        fd = fval.index_select(0, self.f_diag_pos)
        sval = -(self._omega(self.f_ptr, self.f_idx, fval, fd) / fd.index_select(0, self.f_rows)) * fval
        sval[self.f_diag_pos] += 1
        tval = torch.rsqrt(self.t_count.to(self.val.dtype)).index_select(0, self.agg)
        S = torch.sparse_csr_tensor(self.f_ptr, self.f_idx, sval, (self.n, self.n))
        T = torch.sparse_csr_tensor(self.t_ptr, self.t_idx, tval, (self.n, self.n_c))
        self.p_val, P = self._product("P", S, T)
        if P is not None and self.P is None:
            self.p_ptr, self.p_idx = P.crow_indices(), P.col_indices()
            self.p_t = _pt.from_csr(P).transposed
            self.p_perm = self.p_t.perm.to(torch.int64)
        self.pt_val = self.p_val.index_select(0, self.p_perm)                    # Pᵀ's values: one gather through the cached transpose
        self.P = torch.sparse_csr_tensor(self.p_ptr, self.p_idx, self.p_val, (self.n, self.n_c))
        self.PT = torch.sparse_csr_tensor(self.p_t.crow, self.p_t.col, self.pt_val, (self.n_c, self.n))
        ap_val, AP = self._product("AP", self.tensor(), self.P)
        if keep is None:
            self.ap_ptr, self.ap_idx = AP.crow_indices(), AP.col_indices()
        AP = torch.sparse_csr_tensor(self.ap_ptr, self.ap_idx, ap_val, (self.n, self.n_c))
        ac_val, Ac = self._product("PTAP", self.PT, AP)
        if keep is None:
            return _Level(Ac.crow_indices(), Ac.col_indices(), ac_val, self.n_c)
        keep.val = ac_val
        return keep

    def _product(self, slot: str, A: torch.Tensor, B: torch.Tensor):
        """(values of A·B, the product as a tensor or None).  The first call is `sparse_spgemm`.  On the GPU its symbolic plan and
        the operands' patterns are kept, and later calls — new values on the same index tensors — run the numeric kernel alone,
        without a look-up in the pattern cache: a hierarchy has five patterns per level, and a refresh that walked them through
        the cache would push every other pattern of the caller (A's own plans among them) out of it."""
        kept = self._products.get(slot)
        if kept is not None:
            plan, a, b = kept
            return _numeric(plan, a, A.values(), b, B.values()), None
        C = sparse_spgemm(A, B)
        if A.is_cuda:
            aop, bop = _Operand(A), _Operand(B)
            self._products[slot] = (_plan_for(aop, bop), aop.plan, bop.plan)
        return C.values(), C


class SparseAMG(_Factor):
    r"""``M ≈ A⁻¹``: one V(``sweeps``, ``sweeps``) cycle of the aggregation hierarchy of ``A`` from a zero guess.

    ``M(R)`` / ``M.solve(R, transpose=False)`` / ``M.matmul(R)``  the cycle for ``R`` of shape ``(n,)`` or ``(n, p)``.  ``M`` is
                symmetric: ``transpose`` changes nothing, and ``M.T`` is ``M``.  The result is detached.
    ``levels``  a tuple of dicts, one per level: ``n``, ``nnz``, ``theta`` (the value the level's aggregation really used; None
                on the coarsest level, which has none), ``aggregates`` (their number); the coarsest entry carries ``"solver"``:
                ``"dense"`` (the pseudo-inverse) or ``"smoother"``
    ``operator_complexity`` / ``grid_complexity``   ``Σ nnz_l / nnz_0`` and ``Σ n_l / n_0``
    ``A(l)`` / ``P(l)``   the CSR operator of level ``l`` and the prolongator from level ``l + 1`` to ``l``
    ``aggregates(l)``     the aggregate of every node of level ``l``
    ``refresh(A_new)``    new values on the same pattern: every aggregate and every index tensor is kept
    ``info``    0, or 1 + row + (level << 32) of the first non-positive diagonal entry (a device tensor until someone reads it)"""

    def __init__(self, plan: _pt.FactorPlan, layout, shape, values: torch.Tensor, theta: float, sweeps: int, max_levels: int,
                 coarse_size: int):
        self._plan, self._layout, self.shape = plan, layout, tuple(shape)
        self._theta, self._sweeps, self._max_levels, self._coarse_size = float(theta), int(sweeps), int(max_levels), int(coarse_size)
        self._buffers = {}
        g = plan.gather
        ptr = g.crow if g.crow.dtype == g.col.dtype else g.crow.to(g.col.dtype)
        self._levels = [_Level(ptr.contiguous(), g.col.contiguous(), values, g.n_rows)]
        self._build(first=True)

    # ---- setup ----------------------------------------------------------------------------------------------------------------------
    def _build(self, first: bool) -> None:
        levels = self._levels
        info = torch.zeros((), dtype=torch.int64, device=levels[0].val.device)
        l = 0
        while True:
            lv = levels[l]
            d = lv.val.index_select(0, lv.diag_pos)
            ar = torch.arange(lv.n, dtype=torch.int64, device=d.device)
            bad = torch.where(d > 0, lv.n, ar).min() if lv.n else info * 0 + lv.n
            info = torch.where((info == 0) & (bad < lv.n), bad + 1 + (l << 32), info)
            lv.smoother()
            if first:
                last = lv.n <= self._coarse_size or l == self._max_levels - 1
                if not last:
                    last = not lv.coarsen(self._theta)
                    if last and self._theta > 0:      # the retry rule: strength filtering left too many aggregates
                        last = not lv.coarsen(0.0)
                if last:
                    lv.theta, lv.agg, lv.n_c = None, None, 0
                    break
                levels.append(lv.galerkin())
            else:
                if l == len(levels) - 1:
                    break
                lv.galerkin(keep=levels[l + 1])
            l += 1
        self.info = info
        self._coarse_solver(first)
        self.values = levels[0].val

    def _coarse_solver(self, first: bool) -> None:
        lv = self._levels[-1]
        if lv.n <= DENSE_COARSE_MAX:
            lv.solver = "dense"
            dense = lv.tensor().to_dense().to(device="cpu", dtype=torch.float64)        # the one copy to the host: n_L² values
            if bool(torch.isfinite(dense).all()):
                inv = torch.linalg.pinv(dense, hermitian=True)
            else:
                inv = torch.full_like(dense, float("nan"))
            lv.inv = inv.to(dtype=lv.val.dtype).to(lv.val.device)
        else:
            lv.solver = "smoother"
            if first:
                warnings.warn(f"sparse_amg: the coarsest level has {lv.n} rows (more than {DENSE_COARSE_MAX}): it is smoothed, not "
                              "solved — the matrix does not coarsen", stacklevel=3)

    def refresh(self, A_new: torch.Tensor) -> "SparseAMG":
        """Replace the values by those of ``A_new``, a matrix on the SAME pattern (same layout, shape and number of stored
        entries, else ``ValueError``; the indices themselves are not compared).  Every aggregate and every index tensor is kept
        and only the numeric part is recomputed: filter values, weights, prolongators, Galerkin products, the coarse inverse —
        the symbolic ``sparse_spgemm`` plans belong to the unchanged index tensors and are kept with them.  With ``theta > 0`` the strength
        PATTERN stays the one chosen at construction (the values that were dropped then are the ones that are lumped now).
        The result equals a fresh build on ``A_new`` bit for bit whenever that build would choose the same strength pattern.
        Returns ``self``."""
        with torch.no_grad():
            g, values = _operand(A_new, "sparse_amg")
            if A_new.layout != self._layout or tuple(A_new.shape) != self.shape or values.numel() != self._levels[0].nnz:
                raise ValueError(f"sparse_amg: refresh needs a matrix on the pattern of the hierarchy (layout {self._layout}, shape "
                                 f"{self.shape}, {self._levels[0].nnz} stored entries), got {A_new.layout}, {tuple(A_new.shape)}, "
                                 f"{values.numel()}")
            if values.dtype != self.dtype or values.device != self.device:
                raise ValueError(f"sparse_amg: refresh needs values of {self.dtype} on {self.device}, got {values.dtype} on {values.device}")
            self._levels[0].val = self._plan.canonical_values(values).contiguous()
            self._build(first=False)
        return self

    # ---- what the hierarchy looks like --------------------------------------------------------------------------------------------
    @property
    def levels(self):
        out = []
        for l, lv in enumerate(self._levels):
            entry = {"n": lv.n, "nnz": lv.nnz, "theta": lv.theta, "aggregates": lv.n_c}
            if l == len(self._levels) - 1:
                entry["solver"] = lv.solver
            out.append(entry)
        return tuple(out)

    @property
    def operator_complexity(self) -> float:
        return sum(lv.nnz for lv in self._levels) / max(self._levels[0].nnz, 1)

    @property
    def grid_complexity(self) -> float:
        return sum(lv.n for lv in self._levels) / max(self._levels[0].n, 1)

    def A(self, l: int) -> torch.Tensor:
        return self._levels[l].tensor()

    def P(self, l: int) -> torch.Tensor:
        if self._levels[l].P is None:
            raise IndexError(f"sparse_amg: level {l} is the coarsest: it has no prolongator")
        return self._levels[l].P

    def aggregates(self, l: int) -> torch.Tensor:
        if self._levels[l].agg is None:
            raise IndexError(f"sparse_amg: level {l} is the coarsest: it has no aggregates")
        return self._levels[l].agg

    @property
    def T(self) -> "SparseAMG":
        return self

    # ---- the cycle ------------------------------------------------------------------------------------------------------------------
    def _work(self, p: int, dtype: torch.dtype):
        """Per level: two iterates, a residual, and the right-hand side of the level (the restricted residual of the one above)."""
        bufs = self._buffers.get((p, dtype))
        if bufs is None:
            dev = self.device
            bufs = self._buffers[(p, dtype)] = [
                tuple(torch.empty((lv.n, p), dtype=dtype, device=dev) for _ in range(4)) for lv in self._levels]
        return bufs

    def _smooth(self, lv: _Level, b, x, y, times: int, affine, last=None):
        """`times` sweeps x ← x + w∘(b − A·x), alternating between the two buffers (the last one into `last`); returns (x, y)."""
        for k in range(times):
            out = last if (last is not None and k == times - 1) else y
            affine(lv.ptr, lv.idx, lv.val, x, lv.n, lv.n, C=x, B=b, w=lv.w, out=out)
            x, y = out, (x if out is y else y)
        return x, y

    def _cycle(self, l: int, b: torch.Tensor, bufs, affine, out=None) -> torch.Tensor:
        lv = self._levels[l]
        xa, xb, r, _ = bufs[l]
        s = self._sweeps
        if l == len(self._levels) - 1:
            if lv.solver == "dense":
                return torch.mm(lv.inv, b, out=out if out is not None else xa)
            torch.mul(lv.w.unsqueeze(1), b, out=xa)
            return self._smooth(lv, b, xa, xb, 2 * s - 1, affine, last=out)[0]
        torch.mul(lv.w.unsqueeze(1), b, out=xa)                                                       # x = w∘b
        x, y = self._smooth(lv, b, xa, xb, s - 1, affine)
        affine(lv.ptr, lv.idx, lv.val, x, lv.n, lv.n, B=b, out=r)                                     # r = b − A·x
        rc = bufs[l + 1][3]
        affine(lv.p_t.crow, lv.p_t.col, lv.pt_val, r, lv.n_c, lv.n, alpha=-1.0, out=rc)                # r_c = Pᵀ·r
        e = self._cycle(l + 1, rc, bufs, affine)
        affine(lv.p_ptr, lv.p_idx, lv.p_val, e, lv.n, lv.n_c, C=x, alpha=-1.0, out=x)                 # x ← x + P·e, in place
        return self._smooth(lv, b, x, y, s, affine, last=out)[0]

    def solve(self, R: torch.Tensor, transpose: bool = False) -> torch.Tensor:
        def cycle(X):
            X = _be.rowmajor(X)
            out = torch.empty((X.size(0), X.size(1)), dtype=X.dtype, device=X.device)
            return self._cycle(0, X, self._work(X.size(1), X.dtype), _primitives(X)[2], out=out)

        return self._apply(R, (cycle,))

    matmul = solve


def sparse_amg(A: torch.Tensor, *, theta: float = 0.0, sweeps: int = 1, max_levels: int = 10, coarse_size: int = 512,
               check: bool = True) -> SparseAMG:
    r"""The aggregation multigrid preconditioner of a square sparse ``A`` (COO or CSR, float32 / float64, int32 / int64 indices),
    meant for symmetric positive definite ``A``; symmetry is not checked.  Every row must store its diagonal entry
    (``ValueError`` naming the first row that does not).

    ``theta``        strength threshold in ``[0, 1)``: the aggregation (and the prolongator smoother) see ``A_F``, which keeps the
                     diagonal and the off-diagonals with ``|a_ij| >= theta·sqrt(|a_ii·a_jj|)`` and lumps the rest onto the
                     diagonal.  0 keeps everything.  A level on which the filtered pattern leaves more than ``n/2`` aggregates
                     is aggregated again with ``theta = 0``; if that does not help either, it is the coarsest.
    ``sweeps``       damped-Jacobi sweeps before and after the coarse correction (>= 1)
    ``max_levels``   the most levels the hierarchy may have (>= 1)
    ``coarse_size``  a level with at most this many rows is the coarsest (>= 1)

    ``check=True`` reads the breakdown word and raises ``RuntimeError("sparse_amg: non-positive diagonal in row r of level l")``;
    ``check=False`` leaves ``.info`` on the device.  Two calls give the same hierarchy bit for bit: the aggregates are a pure
    function of the pattern and no sum depends on a launch geometry.  No gradient flows through the hierarchy (see the module's
    docstring).  The setup reads the device a few times per level (the MIS-2 poll, the number of aggregates, the sizes of the
    three products); the application never does."""
    if not 0.0 <= float(theta) < 1.0:
        raise ValueError(f"sparse_amg: theta must be in [0, 1), got {theta}")
    for name, v in (("sweeps", sweeps), ("max_levels", max_levels), ("coarse_size", coarse_size)):
        if int(v) < 1:
            raise ValueError(f"sparse_amg: {name} must be at least 1, got {v}")
    with torch.no_grad():
        g, values = _operand(A, "sparse_amg")
        try:
            plan = _pt.factor_plan(g)
        except ValueError as e:
            raise ValueError(str(e).replace("sparse factorisation", "sparse_amg")) from None
        M = SparseAMG(plan, A.layout, A.shape, plan.canonical_values(values).contiguous(), theta, sweeps, max_levels, coarse_size)
    if check:
        word = int(M.info.item())
        if word:
            raise RuntimeError(f"sparse_amg: non-positive diagonal in row {(word - 1) & 0xFFFFFFFF} of level {(word - 1) >> 32}")
    return M
