"""MI355X-native (gfx950) implementation of torchsparsegradutils' sparse hot path.

Drop-in names for ``sparse_mm`` / ``gather_mm`` / ``segment_mm`` / ``sparse_triangular_solve`` / ``sparse_generic_solve`` /
``sparse_generic_lstsq`` / ``sparse_logsumexp`` / ``sparse_bidir_logsumexp`` (reference ``torchsparsegradutils/__init__.py:1-16``),
and ``sparse_softmax`` / ``sparse_log_softmax`` / ``sparse_attention`` / ``sparse_mm_reduce`` / ``sparse_spgemm`` / ``sparse_bsr_mm`` /
``sparse_bsr_attention`` / ``sparse_ilu0`` / ``sparse_ic0`` / ``sparse_fsai`` / ``sparse_amg`` / ``sparse_coloring`` / ``sparse_sgs`` /
``sparse_lobpcg`` / ``sparse_logdet`` / ``sparse_inv_quad_logdet`` / ``sparse_inv_sqrt_mm`` / ``sparse_sqrt_mm`` / ``sparse_expm_mm`` /
``sparse_topk_mm`` / ``sparse_semi_structured_mm`` / ``sparse_semi_structured_linear`` / ``sparse_semi_structured_prune`` /
``sparse_sinkhorn`` beside them;
the arithmetic runs in hand-written HIP kernels behind the C ABI in ``include/tsgu_hip.h``.  GPU only — there is no CPU fallback.
"""

from ._backend import poll_errors
from ._compat import linalg_solve_triangular_compat
from ._pattern import wait_for_plans
from .indexed_matmul import GatherMM, SegmentMM, gather_mm, segment_mm
from .sparse_amg import SparseAMG, sparse_amg
from .sparse_attention import SparseAttention, sparse_attention
from .sparse_bsr_attention import SparseBSRAttention, sparse_bsr_attention
from .sparse_bsr_mm import SparseBSRMatMul, sparse_bsr_mm
from .sparse_coloring import SparseColoredIC0, SparseColoredILU0, SparseColoring, SparseSGS, sparse_coloring, sparse_sgs
from .sparse_factor import SparseIC0, SparseILU0, sparse_ic0, sparse_ilu0
from .sparse_fsai import SparseFSAI, sparse_fsai
from .sparse_lobpcg import SparseLOBPCG, sparse_lobpcg
from .sparse_logdet import SparseLogDet, sparse_inv_quad_logdet, sparse_logdet
from .sparse_logsumexp import SparseLogSumExp, sparse_bidir_logsumexp, sparse_logsumexp
from .sparse_lstsq import SparseGenericLstsq, sparse_generic_lstsq
from .sparse_matmul import SparseMatMul, sparse_mm
from .sparse_mm_reduce import SparseMMReduce, sparse_mm_reduce
from .sparse_sinkhorn import SparseSinkhorn, sparse_sinkhorn
from .sparse_softmax import SparseSoftmax, sparse_log_softmax, sparse_softmax
from .sparse_spgemm import SparseSpGEMM, sparse_spgemm
from .sparse_sqrt import SparseInvSqrtMM, sparse_inv_sqrt_mm, sparse_sqrt_mm
from .sparse_expm import SparseExpmMM, sparse_expm_mm
from .sparse_topk import SparseTopkMM, sparse_topk_mm
from .sparse_semi_structured import (
    SemiStructured,
    sparse_semi_structured_linear,
    sparse_semi_structured_mm,
    sparse_semi_structured_prune,
)
from .sparse_solve import (
    SparseGenericSolve,
    SparseTriangularSolve,
    sparse_generic_solve,
    sparse_triangular_solve,
)

__all__ = [
    "sparse_mm",
    "sparse_mm_reduce",
    "sparse_spgemm",
    "sparse_bsr_mm",
    "sparse_bsr_attention",
    "sparse_ilu0",
    "sparse_ic0",
    "SparseILU0",
    "SparseIC0",
    "sparse_coloring",
    "SparseColoring",
    "sparse_sgs",
    "SparseSGS",
    "SparseColoredILU0",
    "SparseColoredIC0",
    "sparse_fsai",
    "SparseFSAI",
    "sparse_amg",
    "SparseAMG",
    "sparse_lobpcg",
    "SparseLOBPCG",
    "sparse_logdet",
    "sparse_inv_quad_logdet",
    "SparseLogDet",
    "sparse_inv_sqrt_mm",
    "sparse_sqrt_mm",
    "SparseInvSqrtMM",
    "sparse_expm_mm",
    "SparseExpmMM",
    "sparse_topk_mm",
    "SparseTopkMM",
    "SemiStructured",
    "sparse_semi_structured_prune",
    "sparse_semi_structured_mm",
    "sparse_semi_structured_linear",
    "gather_mm",
    "segment_mm",
    "sparse_triangular_solve",
    "sparse_generic_solve",
    "sparse_generic_lstsq",
    "sparse_logsumexp",
    "sparse_bidir_logsumexp",
    "sparse_softmax",
    "sparse_log_softmax",
    "sparse_sinkhorn",
    "SparseSinkhorn",
    "sparse_attention",
    "SparseGenericLstsq",
    "wait_for_plans",
    "poll_errors",
    "SparseMatMul",
    "SparseMMReduce",
    "SparseSpGEMM",
    "SparseBSRMatMul",
    "SparseBSRAttention",
    "SparseTriangularSolve",
    "SparseGenericSolve",
    "SparseLogSumExp",
    "SparseSoftmax",
    "SparseAttention",
    "SegmentMM",
    "GatherMM",
    "linalg_solve_triangular_compat",
]

__version__ = "0.1.0"


def _prefetch_lazy_torch_modules() -> None:
    """torch.autograd's Python front end imports torch.fx.experimental.symbolic_shapes (and with it sympy: 150-450 ms)
    the first time a backward pass is given explicit output gradients — inside the first training step of every process.
    Import it now, together with this package, where a start-up cost belongs (TSGU_PREFETCH_IMPORTS=0: off).  On the importing
    thread on purpose: a helper thread would save the time but can meet the main thread's own imports in a lock cycle, which
    Python resolves by handing one of them a half-initialised module."""
    import os

    if os.environ.get("TSGU_PREFETCH_IMPORTS", "1") != "1":
        return
    try:
        import importlib

        importlib.import_module("torch.fx.experimental.symbolic_shapes")
    except Exception:  # noqa: BLE001  (purely an optimisation)
        pass


_prefetch_lazy_torch_modules()
