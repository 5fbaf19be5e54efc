"""``SparseMultivariateNormal`` — the real caller of the hot path (reference
``torchsparsegradutils/distributions/sparse_multivariate_normal.py:105-389``): a multivariate normal whose
covariance or precision is given by a sparse lower-triangular factor (``L Lᵀ`` or ``L D Lᵀ`` with unit ``L``), sampled
with the reparameterisation trick.

``rsample`` is two calls into the hot path:

* covariance factor:  ``x = L·ε``  (``+ η`` for the implicit unit diagonal of the LDLᵀ form)        → K1 ``sparse_mm``
* precision factor:   ``x = L⁻ᵀ·ε`` → K4 ``sparse_triangular_solve(upper=False, transpose=True[, unitriangular=True])``

The reference routes both through ``_batch_sparse_mv``, which hands the operators a TRANSPOSED VIEW of the noise
(``bvec.t()``, :96) and transposes the result back.  Here that view is consumed in place: K1 / K4 take a column stride,
so the sequence allocates the result and nothing else (the reference's backends copy the view to row-major first).
Constructor checks and messages follow the reference (:249-322).

The density is sparse throughout as well (the reference offers it in ``SparseMultivariateNormalNative`` only, through
``to_dense()``, :531-589).  With ``d = value − loc``, ``log_prob = −½ (n·log 2π + M) − ½·logdet Σ`` and
``entropy = ½ n (1 + log 2π) + ½·logdet Σ``:

=============================  ==============================  ===================  ==========================================
parameterisation               ``M``                           ``½ logdet Σ``       built on
=============================  ==============================  ===================  ==========================================
``scale_tril``                 ``Σ z²``, ``z = L⁻¹d``          ``Σ log L_ii``       K4 ``sparse_triangular_solve(upper=False)``
``scale_tril`` + ``diagonal``  ``Σ z²/D``, ``z = (L+I)⁻¹d``    ``½ Σ log D``        the same with ``unitriangular=True``
``precision_tril``             ``Σ y²``, ``y = Lᵀd``           ``−Σ log L_ii``      K2, the transposed product
``precision_tril`` + diagonal  ``Σ D y²``, ``y = Lᵀd + d``     ``−½ Σ log D``       K2
=============================  ==============================  ===================  ==========================================

The sums are the reductions of ``csrc/mvn.hip`` (two-stage, fixed order: bitwise reproducible), which read the solve's / product's
result in place; ``variance`` (covariance forms) is one pass over the factor's rows.  Value dtypes float32 and float64 (fp32 sums in
fp32); any other dtype raises ``TypeError`` before a kernel is launched.  Gradients reach ``loc``, ``value``, ``diagonal`` and the
factor's values; the factor's gradient is ONE sparse tensor with the factor's own layout, index tensors and index dtype.
"""

from __future__ import annotations

import math
import warnings

import torch
from torch.autograd.function import once_differentiable
from torch.distributions import constraints
from torch.distributions.distribution import Distribution
from torch.distributions.utils import _standard_normal

from .. import _backend as _be
from .. import _cpu
from ..sparse_matmul import _SparseTMatMul, sparse_mm
from ..sparse_solve import _TriOperand, sparse_triangular_solve


def _apply_to_samples(op, mat: torch.Tensor, vec: torch.Tensor, **kwargs) -> torch.Tensor:
    """``op(mat, ·)`` on every sample of ``vec``: samples are rows of ``vec``, the operators want them as columns
    (reference ``_batch_sparse_mv`` :91-102; same four rank combinations, no broadcasting of batch dimensions)."""
    if mat.dim() == 2 and vec.dim() == 1:
        return op(mat, vec.unsqueeze(-1), **kwargs).squeeze(-1)
    if mat.dim() == 2 and vec.dim() == 2:
        return op(mat, vec.t(), **kwargs).t()           # (n, k) transposed view in, transposed layout out: no copies
    if mat.dim() == 3 and vec.dim() == 2:
        return op(mat, vec.unsqueeze(-1), **kwargs).squeeze(-1)
    if mat.dim() == 3 and vec.dim() == 3:
        return op(mat, vec.permute(1, 2, 0), **kwargs).permute(2, 0, 1)
    raise ValueError("Invalid dimensions for bmat and bvec")


_batch_sparse_mv = _apply_to_samples  # the reference's name for the helper


def _factor(name: str, t: torch.Tensor) -> torch.Tensor:
    if t.layout == torch.sparse_coo:
        t = t if t.is_coalesced() else t.coalesce()
    elif t.layout != torch.sparse_csr:
        raise ValueError("{} must be sparse COO or CSR, instead of {}".format(name, t.layout))
    if t.dim() < 2:
        raise ValueError(f"{name} {'matrix ' if name == 'scale_tril' else ''}must be at least two-dimensional, "
                         f"with optional leading batch dimension{'' if name == 'scale_tril' else 's'}")
    if t.dim() > 3:
        raise ValueError("{} can only have 1 batch dimension, but has {}".format(name, t.dim() - 2))
    return t


# ---- the density: reductions over the solve's / product's result and the factor's diagonal -----------------------------------------
_STRICT = "First input should be strictly triangular (i.e. unit diagonals is implicit)"      # (the unit-triangular solve's message)
_LOG_2PI = math.log(2 * math.pi)


def _check_dtype(*tensors) -> None:
    """The density is offered in float32 and float64 (fp32 sums in fp32): anything else is refused before a kernel is launched."""
    for t in tensors:
        if t is not None and t.dtype not in _be.MVN_DTYPES:
            raise TypeError(f"log_prob, entropy and variance take float32 and float64 parameters, got {t.dtype}")


def _diag_positions(plan):
    """Where every row of the (flat, block-diagonal if batched) pattern keeps its diagonal entry, -1 where it stores none: index
    work done once per pattern (``tsgu_csr_diag_positions``) and cached with it."""
    own = plan.core.own
    pos = own.get("diag_pos")
    if pos is None:
        find = _be.csr_diag_positions if plan.crow.is_cuda else _cpu.csr_diag_positions
        pos = own["diag_pos"] = find(plan.crow, plan.col, plan.perm, plan.n_rows)
    return pos


class _LogDiag(torch.autograd.Function):
    """``A ↦ (A, Σ_i log A_ii)`` per batch item, the dense formula ``A.to_dense().diagonal().log().sum()`` on the stored entries: a
    row without a stored diagonal contributes ``log 0 = −inf``, a negative one NaN.

    The factor is handed on (a tensor over the same index tensors and values) so that what is built on it — the solve, the transposed
    product — sends its sparse gradient back through HERE: the log-determinant's share, ``g / A_ii``, is added to the diagonal
    entries of that gradient in place, and the factor receives one sparse gradient with its own index tensors instead of the sum of
    two.  Without a gradient from downstream the zero fill and the scatter are one pass."""

    @staticmethod
    def forward(ctx, A):
        op = _TriOperand(A.detach())
        plan = op.plan
        pos = _diag_positions(plan)
        rpi = plan.n_rows // (op.batch or 1)
        vals = op.values.reshape(-1)
        out = (_be.diag_logsum if vals.is_cuda else _cpu.diag_logsum)(pos, vals, plan.n_rows, rpi)
        ctx.op, ctx.pos, ctx.rpi = op, pos, rpi
        ctx.save_for_backward(op.values)
        ctx.set_materialize_grads(False)
        if op.csr:
            same = op.rebuild(op.values)
        else:
            same = torch.sparse_coo_tensor(op.coo_indices, op.values, op.shape, is_coalesced=True)
        return same, (out if op.batch is not None else out.view(()))

    @staticmethod
    @once_differentiable
    def backward(ctx, g_same, g_out):
        if g_out is None:
            return g_same
        (values,) = ctx.saved_tensors
        op, pos, rpi = ctx.op, ctx.pos, ctx.rpi
        plan = op.plan
        vals = values.reshape(-1)
        gv = None
        if g_same is not None:
            gv = (g_same.values() if op.csr else g_same._values()).reshape(-1)
            if gv.dtype != vals.dtype or not gv.is_contiguous():
                gv = gv.to(vals.dtype).contiguous()
        g = g_out.reshape(-1).to(vals.dtype)
        if vals.is_cuda:
            gv = _be.diag_logsum_backward(plan.crow, plan.perm, pos, vals, g, plan.n_rows, rpi, grad=gv)
        else:
            gv = _cpu.diag_logsum_backward(pos, vals, g, plan.n_rows, rpi, grad=gv)
        return op.rebuild(gv)


class _LogVec(torch.autograd.Function):
    """``D ↦ Σ_i log D_i`` over the last axis (the LDLᵀ forms' log-determinant): the same reduction as :class:`_LogDiag`."""

    @staticmethod
    def forward(ctx, D):
        D = D.detach().contiguous()
        n = D.size(-1)
        out = (_be.diag_logsum if D.is_cuda else _cpu.diag_logsum)(None, D.reshape(-1), D.numel(), n)
        ctx.save_for_backward(D)
        return out.view(D.shape[:-1])

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (D,) = ctx.saved_tensors
        n = D.size(-1)
        g = g.reshape(-1).to(D.dtype)
        if D.is_cuda:
            gD = _be.diag_logsum_backward(None, None, None, D.reshape(-1), g, D.numel(), n)
        else:
            gD = _cpu.diag_logsum_backward(None, D.reshape(-1), g, D.numel(), n)
        return gD.view(D.shape)


class _QuadForm(torch.autograd.Function):
    """``(Y, E, w) ↦ out[item, c] = Σ_i w_i^{±1} (Y[i,c] + E[i,c])²`` for 2-D ``Y`` / ``E`` ``(items·n, k)`` read through their
    strides (``tsgu_quadform``); ``mode``: 0 no weight, 1 multiply, 2 divide."""

    @staticmethod
    def forward(ctx, Y, E, w, mode, rpi):
        Y = Y.detach()
        E = None if E is None else E.detach()
        ctx.w_shape = None if w is None else w.shape
        w = None if w is None else w.detach().reshape(-1)
        out = (_be.quadform if Y.is_cuda else _cpu.quadform)(Y, E, w, mode, rpi)
        ctx.mode, ctx.rpi = mode, rpi
        ctx.save_for_backward(Y, E, w)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        Y, E, w = ctx.saved_tensors
        need_w = w is not None and ctx.needs_input_grad[2]
        back = _be.quadform_backward if Y.is_cuda else _cpu.quadform_backward
        gY, gw = back(Y, E, w, ctx.mode, ctx.rpi, g.to(Y.dtype), need_w)
        return (gY if ctx.needs_input_grad[0] else None, gY if E is not None and ctx.needs_input_grad[1] else None,
                gw.view(ctx.w_shape) if need_w else None, None, None)


class _RowSumSq(torch.autograd.Function):
    """``(A, w, add) ↦ add_i + Σ_k A_ik² w_k`` per row: the diagonal of ``A diag(w) Aᵀ + diag(add)`` (``tsgu_csr_row_sumsq``)."""

    @staticmethod
    def forward(ctx, A, w, add):
        op = _TriOperand(A.detach())
        plan = op.plan
        vals = op.values.reshape(-1)
        ctx.w_shape = None if w is None else w.shape
        w = None if w is None else w.detach().reshape(-1)
        add = None if add is None else add.detach().reshape(-1)
        if vals.is_cuda:
            out = _be.csr_row_sumsq(plan.crow, plan.col, plan.perm, vals, w, add, plan.n_rows)
        else:
            out = _cpu.csr_row_sumsq(plan, vals, w, add)
        ctx.op = op
        ctx.save_for_backward(vals, w)
        return out.view(A.shape[:-1])

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        vals, w = ctx.saved_tensors
        op = ctx.op
        plan = op.plan
        g = g.reshape(-1).to(vals.dtype)
        gA = gw = None
        if ctx.needs_input_grad[0]:
            if vals.is_cuda:
                gA = op.rebuild(_be.csr_row_sumsq_backward(plan.crow, plan.col, plan.perm, vals, w, g, plan.n_rows))
            else:
                gA = op.rebuild(_cpu.csr_row_sumsq_backward(plan, vals, w, g))
        if w is not None and ctx.needs_input_grad[1]:
            # off the training path: grad_w[j] = Σ_{k: col k = j} g[row k] val[k]²  by torch ops
            v = vals if plan.perm is None else vals[plan.perm.to(torch.int64)]
            rows = plan.row_indices().reshape(-1).to(torch.int64)
            gw = torch.zeros_like(w).index_add_(0, plan.col.reshape(-1).to(torch.int64), g[rows] * v * v).view(ctx.w_shape)
        return gA, gw, (g.view(ctx.w_shape) if ctx.needs_input_grad[2] else None)


def _sparse_tmm(A: torch.Tensor, D: torch.Tensor) -> torch.Tensor:
    return _SparseTMatMul.apply(A, D)


def _columns(x: torch.Tensor, batched: bool) -> torch.Tensor:
    """Samples ``(n,)``, ``(k, n)`` — batched: ``(B, n)``, ``(k, B, n)`` — as the 2-D array ``(items·n, k)`` the reductions read: a
    view whenever the batch and event axes are jointly contiguous (the solve's result and the products' transposed views are)."""
    if batched:
        return x.reshape(-1, 1) if x.dim() == 2 else x.reshape(x.size(0), -1).t()
    return x.unsqueeze(-1) if x.dim() == 1 else x.t()


def _half_logdet(factor, diagonal, covariance: bool, validate: bool):
    """(the factor to build the Mahalanobis term on, ½·logdet Σ of shape () or (B,))."""
    if diagonal is not None:
        if validate and _TriOperand(factor.detach()).plan.has_diagonal:      # (one host read per pattern, cached with it)
            raise ValueError(_STRICT)
        half = 0.5 * _LogVec.apply(diagonal)
    else:
        factor, half = _LogDiag.apply(factor)
    return factor, (half if covariance else -half)


def _mahalanobis(factor, diagonal, covariance: bool, d: torch.Tensor) -> torch.Tensor:
    """``M`` of shape ``d.shape[:-1]`` for ``d = value − loc`` (the table in the module docstring)."""
    n = d.size(-1)
    batched = factor.dim() == 3
    lead = d.shape[:-1]
    if batched:
        if d.dim() < 2 or d.size(-2) != factor.size(0):
            raise ValueError("Invalid dimensions for bmat and bvec")
        ds = d if d.dim() == 2 else d.reshape((-1,) + tuple(d.shape[-2:]))
    else:
        ds = d if d.dim() == 1 else d.reshape(-1, n)
    ldlt = diagonal is not None
    w = None
    if ldlt:
        if diagonal.dim() == 2 and not batched:
            raise ValueError("a diagonal with a batch dimension needs a batched factor")
        w = diagonal.expand(factor.size(0), n) if batched else diagonal
    if covariance:
        y = _apply_to_samples(sparse_triangular_solve, factor, ds, upper=False, unitriangular=ldlt)
        M = _QuadForm.apply(_columns(y, batched), None, w, 2 if ldlt else 0, n)
    else:
        y = _apply_to_samples(_sparse_tmm, factor, ds)
        M = _QuadForm.apply(_columns(y, batched), _columns(ds, batched) if ldlt else None, w, 1 if ldlt else 0, n)
    return M.t().reshape(lead)


def _log_prob(loc, factor, diagonal, covariance: bool, value, validate: bool) -> torch.Tensor:
    _check_dtype(loc, factor, diagonal, value)
    n = loc.size(-1)
    factor, half = _half_logdet(factor, diagonal, covariance, validate)
    M = _mahalanobis(factor, diagonal, covariance, value - loc)
    return -0.5 * (n * _LOG_2PI + M) - half


def _entropy(loc, factor, diagonal, covariance: bool, validate: bool, batch_shape) -> torch.Tensor:
    _check_dtype(loc, factor, diagonal)
    _, half = _half_logdet(factor, diagonal, covariance, validate)
    return (0.5 * loc.size(-1) * (1.0 + _LOG_2PI) + half).expand(batch_shape)


def _variance(factor, diagonal, validate: bool) -> torch.Tensor:
    """diag(L Lᵀ): ``Σ_k L_ik²``; diag((L+I) D (L+I)ᵀ): ``D_i + Σ_k L_ik² D_k``."""
    _check_dtype(factor, diagonal)
    if diagonal is None:
        return _RowSumSq.apply(factor, None, None)
    if validate and _TriOperand(factor.detach()).plan.has_diagonal:
        raise ValueError(_STRICT)
    D = diagonal.expand(factor.shape[:-1]).contiguous()
    return _RowSumSq.apply(factor, D, D)


class SparseMultivariateNormal(Distribution):
    r"""Multivariate normal :math:`\mathcal N(\mu, \Sigma)` with :math:`\Sigma = L L^\top`, :math:`L D L^\top` (``scale_tril``)
    or :math:`\Sigma^{-1} = L L^\top`, :math:`L D L^\top` (``precision_tril``); ``diagonal`` given ⇒ LDLᵀ with unit,
    strictly-lower-stored ``L``.  ``loc``: ``(n,)`` or ``(B, n)``; factors: sparse COO/CSR ``(n, n)`` or ``(B, n, n)``."""

    support = constraints.real_vector
    has_rsample = True
    arg_constraints = {}

    def __init__(self, loc, diagonal=None, scale_tril=None, precision_tril=None, validate_args=None):
        if loc.dim() < 1:
            raise ValueError("loc must be at least one-dimensional.")
        if loc.dim() > 2:
            raise ValueError(
                "loc must be at most two-dimensional as the current implementation only supports 1 batch dimension."
            )
        event_shape = loc.shape[-1:]
        self._loc = loc
        if diagonal is not None:
            if diagonal.dim() < 1:
                raise ValueError("diagonal must be at least one-dimensional.")
            if diagonal.dim() > 2:
                raise ValueError(
                    "diagonal must be at most two-dimensional as the current implementation only supports 1 batch dimension."
                )
            if diagonal.shape[-1:] != event_shape:
                raise ValueError("diagonal must be a batch of vectors with shape {}".format(event_shape))
        self._diagonal = diagonal
        if (scale_tril is not None) + (precision_tril is not None) != 1:
            raise ValueError("Exactly one of scale_tril or precision_tril may be specified.")
        if scale_tril is not None:
            factor = self._scale_tril = _factor("scale_tril", scale_tril)
        else:
            factor = self._precision_tril = _factor("precision_tril", precision_tril)
        shapes = [loc.shape[:-1], factor.shape[:-2]] + ([diagonal.shape[:-1]] if diagonal is not None else [])
        super().__init__(torch.broadcast_shapes(*shapes), event_shape, validate_args=validate_args)

    diagonal = property(lambda self: self._diagonal)
    scale_tril = property(lambda self: self._scale_tril)
    precision_tril = property(lambda self: self._precision_tril)
    loc = property(lambda self: self._loc)
    mean = property(lambda self: self._loc)
    mode = property(lambda self: self._loc)

    @property
    def is_ldlt_parameterization(self):
        return self._diagonal is not None

    def _transform(self, eps: torch.Tensor) -> torch.Tensor:
        """Standard-normal noise → sample (reference :358-389)."""
        ldlt = self._diagonal is not None
        if "_scale_tril" in self.__dict__:
            if ldlt:
                eta = self._diagonal.sqrt() * eps
                x = _apply_to_samples(sparse_mm, self._scale_tril, eta) + eta   # unit diagonal is implicit
            else:
                x = _apply_to_samples(sparse_mm, self._scale_tril, eps)
        else:
            rhs = eps / self._diagonal.sqrt() if ldlt else eps
            x = _apply_to_samples(sparse_triangular_solve, self._precision_tril, rhs,
                                  upper=False, unitriangular=ldlt, transpose=True)
        return self._loc + x

    def rsample(self, sample_shape=torch.Size()):
        shape = self._extended_shape(sample_shape)
        return self._transform(_standard_normal(shape, dtype=self._loc.dtype, device=self._loc.device))

    def _parameters(self):
        """(factor, diagonal, whether the factor is the covariance's)."""
        covariance = "_scale_tril" in self.__dict__
        return (self._scale_tril if covariance else self._precision_tril), self._diagonal, covariance

    def log_prob(self, value):
        r"""Log density at ``value`` of shape ``sample_shape + batch_shape + (n,)`` → ``value.shape[:-1]``, sparse throughout
        (module docstring).  A row of an LLᵀ factor without a stored diagonal entry gives ``∓inf`` as the dense formula does, a
        negative one NaN; an LDLᵀ factor must be strictly lower (checked under ``validate_args=True``)."""
        if self._validate_args:
            self._validate_sample(value)
        factor, diagonal, covariance = self._parameters()
        return _log_prob(self._loc, factor, diagonal, covariance, value, bool(self._validate_args))

    def entropy(self):
        r"""``½ n (1 + log 2π) + ½ logdet Σ`` of shape ``batch_shape``: one reduction over the stored diagonal (or ``D``)."""
        factor, diagonal, covariance = self._parameters()
        return _entropy(self._loc, factor, diagonal, covariance, bool(self._validate_args), self._batch_shape)

    @property
    def variance(self):
        r"""Diagonal of ``Σ`` for the covariance forms: ``Σ_k L_ik²`` (LLᵀ) or ``D_i + Σ_k L_ik² D_k`` (LDLᵀ)."""
        factor, diagonal, covariance = self._parameters()
        if not covariance:
            raise NotImplementedError("variance of a precision_tril parameterisation is the diagonal of an inverse, which is not a "
                                      "sparse operation; it is provided for scale_tril only")
        return _variance(factor, diagonal, bool(self._validate_args)).expand(self._batch_shape + self._event_shape)

class SparseMultivariateNormalNative(Distribution):
    r"""The reference's second sparse multivariate normal (``sparse_multivariate_normal.py:392-589``): ``Σ = L Lᵀ`` with an
    unbatched CSR factor ``L`` (stored positive diagonal) and ``loc`` of shape ``(n,)``.  Same constructor checks and messages.

    ``rsample`` is ``sparse_mm`` on the transposed view of the noise; ``log_prob`` and ``variance`` are the sparse density of
    :class:`SparseMultivariateNormal` — nothing is densified, so they emit none of the reference's memory warnings.
    ``covariance_matrix`` is dense by definition and warns as the reference does."""

    arg_constraints = {"loc": constraints.real_vector}
    support = constraints.real_vector
    has_rsample = True

    def __init__(self, loc, scale_tril, validate_args=None):
        if loc.dim() != 1:
            raise ValueError("loc must be one-dimensional for SparseMultivariateNormalNative.")
        if scale_tril.layout != torch.sparse_csr:
            raise ValueError("scale_tril must be sparse CSR for SparseMultivariateNormalNative.")
        if scale_tril.dim() != 2:
            raise ValueError("scale_tril must be two-dimensional (unbatched) for SparseMultivariateNormalNative.")
        if scale_tril.shape[0] != scale_tril.shape[1]:
            raise ValueError("scale_tril must be square.")
        if scale_tril.shape[0] != loc.shape[0]:
            raise ValueError("scale_tril must have the same size as loc.")
        self._loc = loc
        self._scale_tril = scale_tril
        super().__init__(torch.Size(), loc.shape, validate_args=validate_args)

    scale_tril = property(lambda self: self._scale_tril)
    loc = property(lambda self: self._loc)
    mean = property(lambda self: self._loc)
    mode = property(lambda self: self._loc)

    @property
    def covariance_matrix(self):
        r""":math:`\Sigma = L L^\top`, dense."""
        warnings.warn(
            "Computing covariance_matrix requires converting sparse matrix to dense format. "
            "This may cause memory issues for large sparse matrices. "
            "Consider using variance property for diagonal elements only.",
            UserWarning,
            stacklevel=2,
        )
        L = self._scale_tril.to_dense()
        return L @ L.T

    @property
    def variance(self):
        r""":math:`\operatorname{diag}(L L^\top)`, one pass over the factor's rows."""
        return _variance(self._scale_tril, None, False)

    def rsample(self, sample_shape=torch.Size()):
        shape = self._extended_shape(sample_shape)
        eps = _standard_normal(shape, dtype=self._loc.dtype, device=self._loc.device)
        flat = eps if eps.dim() <= 2 else eps.reshape(-1, eps.size(-1))
        return self._loc + _apply_to_samples(sparse_mm, self._scale_tril, flat).reshape(shape)

    def log_prob(self, value):
        if self._validate_args:
            self._validate_sample(value)
        return _log_prob(self._loc, self._scale_tril, None, True, value, bool(self._validate_args))

    def entropy(self):
        return _entropy(self._loc, self._scale_tril, None, True, bool(self._validate_args), self._batch_shape)
