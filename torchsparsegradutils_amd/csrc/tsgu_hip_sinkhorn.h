/*
 * tsgu_hip_sinkhorn.h — the half steps of a Sinkhorn iteration over a sparse pattern, their adjoints and the transport plan
 * (sparse_sinkhorn.py): entries of libtsgu_hip.so.
 *
 * STAGED: this header lives beside the sources and not under include/ ("Adding a header"); its entries are bound
 * from `_backend.STAGED_SINKHORN`.  An addition to the C ABI of tsgu_hip.h with the same conventions (device pointers, `device` +
 * `stream` last, status codes, tsgu_vtype / tsgu_itype, no synchronisation, no allocation, no global atomics).  The entries are
 * additive, so TSGU_ABI_VERSION stays as it is.  The reference has no counterpart.
 *
 * A direction of the pattern is (ptr, perm, idx): group g holds the entries k in [ptr[g], ptr[g + 1]), entry k is val[perm[k]]
 * (val[k] when perm is NULL) and lies in group idx[k] of the other direction.  The rows of a CSR matrix are (crow, NULL, col), its
 * columns those of the transposed pattern with the perm into the value array.  `val` has the value type; potentials, marginals,
 * cotangents and the gradient buffer have its ACCUMULATOR type: float for TSGU_F32 and TSGU_BF16, double for TSGU_F64.
 *
 * Every walk is the range walk of the segmented log-sum-exp (tsgu_segment_logsumexp): one wave per range of entries, partials of a
 * group that crosses ranges merged in a fixed order.  `workspace` (tsgu_sinkhorn_workspace bytes, 16-byte aligned) may be NULL with
 * workspace_bytes = 0 when the caller knows that no group crosses a range boundary; the merge launch is then omitted.
 */
#ifndef TSGU_HIP_SINKHORN_H
#define TSGU_HIP_SINKHORN_H

#include "../../include/tsgu_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host only: bytes of the workspace of the entries below for `nnz` entries of value type `vtype`. */
int tsgu_sinkhorn_workspace(int vtype, int64_t nnz, int64_t* bytes_host);

/* out[g] = (log_marg ? log_marg[g] : 0) - log sum_{k in group g} exp(val[perm ? perm[k] : k] + other[idx[k]]).
 * A val of -inf is an absent entry: its term is exp(-inf) whatever other[idx[k]] is (+inf included).  A group without entries (or
 * with nothing but -inf) gives +inf; a NaN gives NaN.  nnz = 0 still writes every group. */
int tsgu_sinkhorn_half(int vtype, int itype, int64_t n_groups, int64_t nnz, const void* ptr, const void* perm, const void* idx,
                       const void* val, const void* other, const void* log_marg, void* out, void* workspace, int64_t workspace_bytes,
                       int device, void* stream);

/* One pass in stored order: out[k] = val[k] + pot_group[group of k by ptr] + pot_other[idx[k]], rounded once to the value type;
 * a val of -inf stays -inf whatever the potentials (a stored -inf is an absent entry). */
int tsgu_sinkhorn_plan(int vtype, int itype, int64_t n_groups, int64_t nnz, const void* ptr, const void* idx, const void* val,
                       const void* pot_group, const void* pot_other, void* out, int device, void* stream);

/* The adjoint of the half step of the OTHER direction, walked in this one.  With k' = perm ? perm[k] : k, c = idx[k], g = grp[k]
 * (the group of entry k: ptr expanded, [nnz] of `itype`):
 *   term_k = g_other[c] * exp(((val[k'] + pot_group[g]) + pot_other[c]) - (log_marg_other ? log_marg_other[c] : 0))
 * in this order.  A caller that kept -lse of the other direction's half step passes it as pot_other with log_marg_other NULL:
 * val + pot_group is the value that half step staged, so the weights of one of its groups sum to one up to the rounding of the sum,
 * whatever the size of the potentials (a potential rounded after the subtraction of its log marginal does not give that).
 *   grad[k'] -= term_k                       (read-modify-write; the positions are distinct)
 *   g_out[g]  = (accumulate ? g_out[g] : 0) - sum_{k in group g} term_k
 * term_k is 0 where val[k'] is -inf (an absent entry), also beside an infinite potential.  nnz = 0 still writes every group. */
int tsgu_sinkhorn_half_backward(int vtype, int itype, int64_t n_groups, int64_t nnz, const void* ptr, const void* perm, const void* idx,
                                const void* grp, const void* val, const void* pot_group, const void* pot_other,
                                const void* log_marg_other, const void* g_other, void* grad, void* g_out, int accumulate,
                                void* workspace, int64_t workspace_bytes, int device, void* stream);

/* out[g] = (add ? add[g] : 0) + sum_{k in group g} val[perm ? perm[k] : k]; val, add and out of the accumulator type of `vtype`. */
int tsgu_segment_sum(int vtype, int itype, int64_t n_groups, int64_t nnz, const void* ptr, const void* perm, const void* val,
                     const void* add, void* out, void* workspace, int64_t workspace_bytes, int device, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TSGU_HIP_SINKHORN_H */
