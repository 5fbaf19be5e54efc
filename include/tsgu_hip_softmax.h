/*
 * tsgu_hip_softmax.h — the segmented softmax entries of libtsgu_hip.so.
 *
 * An addition to the C ABI of tsgu_hip.h with the same conventions (device pointers, `device` + `stream` last, status codes,
 * tsgu_vtype / tsgu_itype, no synchronisation, no allocation).  The entries are additive, so TSGU_ABI_VERSION stays as it is.
 * The reference has no counterpart: it offers the log-sum-exp (sparse_logsumexp.py) but not its normalising form, and
 * torch.sparse.softmax exists for COO only.
 */
#ifndef TSGU_HIP_SOFTMAX_H
#define TSGU_HIP_SOFTMAX_H

#include "tsgu_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Softmax (log_form = 0) or log-softmax (log_form = 1) over the stored entries of every group [ptr[g], ptr[g+1]):
 *   out[k'] = exp(val[k'] - m_g) / sum_{j in g} exp(val[j'] - m_g)        k' = perm ? perm[k] : k,  m_g the group's maximum
 *   out[k'] = (val[k'] - m_g) - log sum_{j in g} exp(val[j'] - m_g)       (log form)
 * Absent entries do not take part; an empty group writes nothing.  A group with a NaN or a +inf, or with nothing but -inf, is
 * NaN throughout (torch.softmax on the group's values).  bf16 values are computed in fp32 and rounded once when stored.
 * The row direction of a CSR pattern is (crow, no perm); the column direction its cached transpose (tptr, perm into A's values):
 * `out` is in A's stored order either way.  `out` must not overlap `val`.
 *
 * The entries are cut into ranges of 8192 / sizeof(accumulator) entries (2048 for fp32 and bf16, 1024 for fp64), one wave each;
 * a group inside one range is finished there (one read and one write per entry).  Groups that cross a range boundary take two
 * more short launches and the workspace: tsgu_segment_softmax_workspace(vtype, nnz) bytes, 16-byte aligned.  A caller that
 * knows from the pattern that NO non-empty group crosses a boundary (ptr[g] / range == (ptr[g+1] - 1) / range for all of them)
 * passes workspace = NULL and workspace_bytes = 0: the two launches are omitted.  (With that promise broken the entries of
 * crossing groups are left unnormalised; nothing is read or written out of bounds.)
 * Deterministic: partial sums are merged in a fixed order, no float atomics.
 */
int tsgu_segment_softmax_workspace(int vtype, int64_t nnz, int64_t* bytes_host);
int tsgu_segment_softmax(int vtype, int itype, int64_t n_groups, int64_t nnz, const void* ptr, const void* perm, const void* val,
                         int log_form, void* out, void* workspace, int64_t workspace_bytes, int device, void* stream);
/*
 * Gradient of the stored values from the forward's result y and its upstream gradient g (both in A's stored order, as gin):
 *   gin[k'] = y[k'] * (g[k'] - sum_{j in g} g[j'] * y[j'])                (softmax)
 *   gin[k'] = g[k'] - exp(y[k']) * sum_{j in g} g[j']                     (log form)
 * Same cutting, workspace and promise as the forward; the sums are two-stage in a fixed order.
 */
int tsgu_segment_softmax_backward(int vtype, int itype, int64_t n_groups, int64_t nnz, const void* ptr, const void* perm,
                                  const void* y, const void* g, int log_form, void* gin, void* workspace,
                                  int64_t workspace_bytes, int device, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TSGU_HIP_SOFTMAX_H */
