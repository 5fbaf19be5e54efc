/*
 * tsgu_hip_lsmr.h — the step kernels of LSMR (utils/lsmr.py; Fong & Saunders, SIAM J. Sci. Comput. 33(5), 2011): entries of
 * libtsgu_hip.so.
 *
 * An addition to the C ABI of tsgu_hip.h with the same conventions (device pointers, `device` + `stream`
 * last, status codes, tsgu_vtype, no synchronisation, no allocation).  The entries are additive, so TSGU_ABI_VERSION stays as it
 * is.
 *
 * Operands.  Values are TSGU_F32 or TSGU_F64 (TSGU_BF16 is TSGU_ERR_BAD_DTYPE).  A vector operand is a contiguous row-major [n][p]
 * array, 16-byte aligned: the p columns are independent least-squares problems that advance in lock-step.  Widths, workgroups
 * and partial rows are those of the Krylov step kernels of tsgu_hip.h (K7): a launch over n rows writes
 * tsgu_cg_num_blocks(vtype, n, p) partial rows of p values; `fold` (tsgu_cg_fold_rows() x p, may be NULL) is scratch for long
 * partial lists.
 *
 * The Golub-Kahan vectors are kept unnormalised, u~ = beta u ([m][p]) and v~ = alpha v ([n][p]); their norms are scalars.
 *
 * State, zeroed and then filled by the caller before the first call (utils/lsmr.py does it with tensor ops):
 *   scal   DOUBLE for both value types, tsgu_lsmr_scal_rows() = 28 rows of p values:
 *          0 alpha | 1 beta | 2 alphabar | 3 rho | 4 rhobar | 5 cbar | 6 sbar | 7 zeta | 8 zetabar | 9 betadd | 10 betad |
 *          11 rhodold | 12 tautildeold | 13 thetatilde | 14 d | 15 |A|^2 estimate | 16 maxrbar | 17 minrbar | 18 |b| |
 *          19 |r| estimate | 20 |A| estimate | 21 cond(A) estimate | 22 s_prod | 23 s_self | 24 c1 | 25 c2 | 26 c3 |
 *          27 the divisor of v~ in the update (alpha, or 1 where alpha = 0)
 *          (the names are those of the paper's algorithm and of utils/lsmr.py)
 *   flags  int32, 2 + 2 p words: [0] stop: every column is done | [1] iterations run | [2, 2 + p) done | [2 + p, 2 + 2 p) the
 *          iterations of the column: the last iteration that began while it was not done
 * Every launcher returns at once, writing nothing, when flags[0] != 0.
 *
 * Determinism: no atomics.  A partial row sums a workgroup's rows in an order that depends on (n, p) alone and
 * tsgu_lsmr_scalar sums partial rows in an order that depends on their count and p alone: two runs give the same bits.
 *
 * Every launcher refuses on the host, before any launch: NULL pointers, n <= 0, p <= 0, a phase or `which` out of range, operands
 * that are not 16-byte aligned (TSGU_ERR_BAD_ARG), unknown value types (TSGU_ERR_BAD_DTYPE), a p the lane geometry does not
 * cover (TSGU_ERR_TOO_LARGE).
 */
#ifndef TSGU_HIP_LSMR_H
#define TSGU_HIP_LSMR_H

#include "tsgu_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host only: rows of the scalar block. */
int tsgu_lsmr_scal_rows(void);

/* One phase of the per-column state on one workgroup.  partial: `n_partial` rows of p sums of squares in the value type, as the
 * phase's producer wrote them.
 *   phase 0, BETA     partial of the BIDIAG launch over u~: beta = sqrt(sum).  (s_prod, s_self) of the second half step:
 *            (1 / beta, beta / alpha), (1 / beta, 0) where alpha = 0, and (0, -1) where beta = 0 (v~ keeps its bits).
 *   phase 1, ROTATE   partial of the BIDIAG launch over v~: alpha = sqrt(sum), kept where beta = 0.  The rotation for `damp`, Q_k
 *            and Qbar_k, the estimates of |r|, |A| and cond(A); c1 = thetabar rho / (rhoold rhobarold), c2 = zeta / (rho rhobar)
 *            and 0 for a done column, c3 = thetanew / rho (each 0 where its divisor is 0); (s_prod, s_self) of the next first
 *            half step: (1 / alpha, alpha / beta), 0 where the divisor is 0.  iterations of a column that is not done =
 *            flags[1] + 1; then flags[1] += 1.
 *   phase 2, STOP     partial of the UPDATE launch: |x| = sqrt(sum).  The six stopping tests of the paper's section 6 with
 *            `atol`, `btol`, `ctol` = 1 / conlim and `eps` (the machine epsilon of the value type); done |= stop; flags[0] = every
 *            column is done. */
int tsgu_lsmr_scalar(int vtype, int phase, const void* partial, int64_t n_partial, void* fold, void* scal, int* flags, double damp,
                     double atol, double btol, double ctol, double eps, int64_t p, int device, void* stream);

/* which 0, BIDIAG: a0 = y [n][p] (u~ or v~), a1 = the product (A v~ or A' u~); a2, a3 unused (NULL).
 *            y <- s_prod * a1 - s_self * y (two products, one subtraction, coefficients rounded to the value type);
 *            partial[b][c] = the sum of y^2 over the rows of workgroup b.
 * which 1, UPDATE: a0 = x, a1 = v~ (read only), a2 = h, a3 = hbar, all [n][p].  vhat = v~ / scal[27]; hbar <- h - c1 * hbar;
 *            x <- x + c2 * hbar (x keeps its bits where c2 = 0); h <- vhat - c3 * h; partial[b][c] = the sum of x^2. */
int tsgu_lsmr_vector(int vtype, int which, int64_t n, int64_t p, void* a0, const void* a1, void* a2, void* a3, const void* scal,
                     const int* flags, void* partial, int device, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TSGU_HIP_LSMR_H */
