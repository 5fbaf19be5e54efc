// K8: fused LSMR recurrences on gfx950 (Fong & Saunders, SIAM J. Sci. Comput. 33(5), 2011), every right-hand side at once.
//
// The host-driven loop of utils/lsmr.py reads three norms back per iteration, runs the rotations in numpy and uploads the
// coefficients of a dozen tensor ops.  Here the Golub-Kahan vectors are kept UNNORMALISED, u~ = beta u and v~ = alpha v, with
// their norms in the scalar block, so that a half step of the bidiagonalisation is one pass with no normalisation pass after it:
//   u~ <- (1/alpha) (A v~) - (alpha/beta) u~        beta  <- |u~|
//   v~ <- (1/beta) (A' u~) - (beta/alpha) v~        alpha <- |v~|
// and one iteration is
//   A v~ -> vector(BIDIAG on u~) -> scalar(BETA) -> A' u~ -> vector(BIDIAG on v~) -> scalar(ROTATE) -> vector(UPDATE) -> scalar(STOP)
// All per-column scalars live on the device, in double precision for both value types (as the host loop keeps them); the host
// reads one word per chunk of iterations.  Reductions are two-stage in a fixed order.  Every kernel is a no-op once flags[0] != 0.
//
// scal, double [28][p]:
//    0 alpha | 1 beta | 2 alphabar | 3 rho | 4 rhobar | 5 cbar | 6 sbar | 7 zeta | 8 zetabar | 9 betadd | 10 betad | 11 rhodold |
//   12 tautildeold | 13 thetatilde | 14 d | 15 |A|^2 estimate | 16 maxrbar | 17 minrbar | 18 |b| | 19 |r| estimate |
//   20 |A| estimate | 21 cond(A) estimate | 22 s_prod, 23 s_self: what the next BIDIAG takes (y <- s_prod prod - s_self y) |
//   24 c1, 25 c2, 26 c3: what UPDATE takes | 27 what UPDATE divides v~ by (alpha, or 1 where alpha = 0)
// flags, int32 [2 + 2 p]: [0] stop: every column is done | [1] iterations run | [2, 2 + p) done | [2 + p, 2 + 2 p) iterations of
//   the column (the last iteration that began while it was live)
#include "krylov_common.h"
#include "../../include/tsgu_hip_lsmr.h"

namespace tsgu {

enum LsmrPhase { kLsBeta = 0, kLsRotate = 1, kLsStop = 2 };
enum LsmrVector { kLsBidiag = 0, kLsUpdate = 1 };
enum LsmrRow {
    kLsAlpha = 0, kLsBetaRow, kLsAlphabar, kLsRho, kLsRhobar, kLsCbar, kLsSbar, kLsZeta, kLsZetabar, kLsBetadd, kLsBetad, kLsRhodold,
    kLsTautildeold, kLsThetatilde, kLsD, kLsNormA2, kLsMaxrbar, kLsMinrbar, kLsNormb, kLsNormr, kLsNormA, kLsCondA, kLsSProd, kLsSSelf,
    kLsC1, kLsC2, kLsC3, kLsAlphaDiv, kLsRows
};

// Stable plane rotation: r = hypot(a, b), c = a / r, s = b / r; r == 0 gives c = s = 0.
__device__ __forceinline__ void lsmr_rotation(double a, double b, double& c, double& s, double& r) {
    r = hypot(a, b);
    const double safe = r > 0 ? r : 1.0;
    c = a / safe;
    s = b / safe;
}

__device__ __forceinline__ double lsmr_ratio(double num, double den) { return den != 0 ? num / den : 0.0; }

// One workgroup, one thread per column in windows of 64 columns.  partial: n_partial rows of p sums of squares in the value type.
template <typename V>
__global__ __launch_bounds__(kBlock) void lsmr_scalar_kernel(int phase, const V* __restrict__ partial, int64_t n_partial, int64_t p,
                                                             double* __restrict__ scal, int* __restrict__ flags, double damp,
                                                             double atol, double btol, double ctol, double eps) {
    __shared__ V red[kBlock];
    __shared__ int live_any;
    if (flags[0] != 0) return;
    const int t = threadIdx.x;
    const int itn = flags[1] + 1;  // the iteration this launch belongs to (read by every thread before thread 0 moves it on)
    if (t == 0) live_any = 0;
    int* done = flags + 2;
    int* its = flags + 2 + p;
    auto S = [&](int row, int64_t c) -> double& { return scal[(int64_t)row * p + c]; };
    for (int64_t c0 = 0; c0 < p; c0 += 64) {
        const int w = (int)(p - c0 < 64 ? p - c0 : 64);
        const double sum = (double)block_colsum<V>(partial, n_partial, p, c0, w, red);
        if (t >= w) continue;
        const int64_t c = c0 + t;
        if (phase == kLsBeta) {
            // beta = |u~|; the second half step keeps v~ where beta = 0 (u = 0, v and alpha kept: lsmr.py, the `pos` columns)
            const double beta = sqrt(sum > 0 ? sum : 0.0), alpha = S(kLsAlpha, c);
            S(kLsBetaRow, c) = beta;
            S(kLsSProd, c) = beta > 0 ? 1.0 / beta : 0.0;
            S(kLsSSelf, c) = beta > 0 ? lsmr_ratio(beta, alpha) : -1.0;
        } else if (phase == kLsRotate) {
            const double beta = S(kLsBetaRow, c);
            const double alpha = beta > 0 ? sqrt(sum > 0 ? sum : 0.0) : S(kLsAlpha, c);
            const bool live = done[c] == 0;
            // rotation for the damping term, then Q_k on the bidiagonal
            double chat, shat, alphahat, cr, sr, rho;
            lsmr_rotation(S(kLsAlphabar, c), damp, chat, shat, alphahat);
            const double rhoold = S(kLsRho, c);
            lsmr_rotation(alphahat, beta, cr, sr, rho);
            const double thetanew = sr * alpha;
            const double alphabar = cr * alpha;
            // Qbar_k on R_k'
            const double rhobarold = S(kLsRhobar, c), zetaold = S(kLsZeta, c), zetabar_in = S(kLsZetabar, c);
            const double thetabar = S(kLsSbar, c) * rho;
            const double rhotemp = S(kLsCbar, c) * rho;
            double cbar, sbar, rhobar;
            lsmr_rotation(rhotemp, thetanew, cbar, sbar, rhobar);
            const double zeta = cbar * zetabar_in;
            const double zetabar = -sbar * zetabar_in;
            // coefficients of hbar, x, h (a finished column keeps its x)
            S(kLsC1, c) = lsmr_ratio(thetabar * rho, rhoold * rhobarold);
            S(kLsC2, c) = live ? lsmr_ratio(zeta, rho * rhobar) : 0.0;
            S(kLsC3, c) = lsmr_ratio(thetanew, rho);
            S(kLsAlphaDiv, c) = alpha > 0 ? alpha : 1.0;
            // estimate of |r|: rotations Qhat_{k,2k+1}, Q_{k,k+1}, Qtilde_{k-1}
            const double betadd_in = S(kLsBetadd, c);
            const double betaacute = chat * betadd_in;
            const double betacheck = -shat * betadd_in;
            const double betahat = cr * betaacute;
            const double betadd = -sr * betaacute;
            const double thetatildeold = S(kLsThetatilde, c);
            double ctildeold, stildeold, rhotildeold;
            lsmr_rotation(S(kLsRhodold, c), thetabar, ctildeold, stildeold, rhotildeold);
            const double thetatilde = stildeold * rhobar;
            const double rhodold = ctildeold * rhobar;
            const double betad = -stildeold * S(kLsBetad, c) + ctildeold * betahat;
            const double tautildeold = (zetaold - thetatildeold * S(kLsTautildeold, c)) / (rhotildeold != 0 ? rhotildeold : 1.0);
            const double taud = (zeta - thetatilde * tautildeold) / (rhodold != 0 ? rhodold : 1.0);
            const double d = S(kLsD, c) + betacheck * betacheck;
            S(kLsNormr, c) = sqrt(d + (betad - taud) * (betad - taud) + betadd * betadd);
            // estimates of |A| and cond(A)
            double norm_a2 = S(kLsNormA2, c) + beta * beta;
            S(kLsNormA, c) = sqrt(norm_a2);
            norm_a2 += alpha * alpha;
            const double maxrbar = fmax(S(kLsMaxrbar, c), rhobarold);
            const double minrbar = itn > 1 ? fmin(S(kLsMinrbar, c), rhobarold) : S(kLsMinrbar, c);
            S(kLsCondA, c) = fmax(maxrbar, rhotemp) / fmin(minrbar, rhotemp);
            S(kLsAlpha, c) = alpha;
            S(kLsAlphabar, c) = alphabar;
            S(kLsRho, c) = rho;
            S(kLsRhobar, c) = rhobar;
            S(kLsCbar, c) = cbar;
            S(kLsSbar, c) = sbar;
            S(kLsZeta, c) = zeta;
            S(kLsZetabar, c) = zetabar;
            S(kLsBetadd, c) = betadd;
            S(kLsBetad, c) = betad;
            S(kLsRhodold, c) = rhodold;
            S(kLsTautildeold, c) = tautildeold;
            S(kLsThetatilde, c) = thetatilde;
            S(kLsD, c) = d;
            S(kLsNormA2, c) = norm_a2;
            S(kLsMaxrbar, c) = maxrbar;
            S(kLsMinrbar, c) = minrbar;
            // the next first half step: u~ <- (1/alpha) A v~ - (alpha/beta) u~ (u = 0 where beta = 0)
            S(kLsSProd, c) = alpha > 0 ? 1.0 / alpha : 0.0;
            S(kLsSSelf, c) = lsmr_ratio(alpha, beta);
            if (live) its[c] = itn;
        } else {
            // the stopping tests of the paper, section 6; the first three guard against tolerances below machine precision
            const double normx = sqrt(sum > 0 ? sum : 0.0);
            const double normb = S(kLsNormb, c), norm_a = S(kLsNormA, c), normr = S(kLsNormr, c);
            const double normb_safe = normb > 0 ? normb : 1.0;
            const double normar = fabs(S(kLsZetabar, c));
            const double test1 = normr / normb_safe;
            const double test2 = normar / (norm_a * normr + eps);
            const double test3 = 1.0 / (S(kLsCondA, c) + eps);
            const double t1 = test1 / (1.0 + norm_a * normx / normb_safe);
            const double rtol = btol + atol * norm_a * normx / normb_safe;
            const bool stop = (1.0 + test3 <= 1.0) || (1.0 + test2 <= 1.0) || (1.0 + t1 <= 1.0) || (test3 <= ctol) || (test2 <= atol) ||
                              (test1 <= rtol);
            if (stop) done[c] = 1;
            if (done[c] == 0) live_any = 1;  // (every writer stores the same value)
        }
    }
    __syncthreads();
    if (t == 0) {
        if (phase == kLsRotate) flags[1] = itn;
        if (phase == kLsStop && live_any == 0) flags[0] = 1;
    }
}

// y <- s_prod prod - s_self y in place over [n][p], coefficients per column from the scalar block; partial |y|^2 per workgroup.
template <typename V, int VEC>
__global__ __launch_bounds__(kBlock) void lsmr_bidiag_kernel(int64_t n, int64_t p, V* __restrict__ y, const V* __restrict__ prod,
                                                             const double* __restrict__ scal, const int* __restrict__ flags, int lpr,
                                                             int rpp, V* __restrict__ partial) {
    __shared__ V red[kBlock * VEC];
    if (flags[0] != 0) return;
    const Lanes L = lanes<VEC>(p, lpr, rpp);
    V sp[VEC], ss[VEC], acc[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        acc[k] = 0;
        sp[k] = L.on ? (V)scal[kLsSProd * p + L.c + k] : (V)0;
        ss[k] = L.on ? (V)scal[kLsSSelf * p + L.c + k] : (V)0;
    }
    for_rows(L, n, [&](int, int64_t row) {
        const int64_t o = row * p + L.c;
        V a[VEC], pr[VEC];
        load_vec<V, VEC>(y + o, a);
        load_vec<V, VEC>(prod + o, pr);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            a[k] = sp[k] * pr[k] - ss[k] * a[k];
            acc[k] = fma(a[k], a[k], acc[k]);
        }
        store_vec<V, VEC>(y + o, a);
    });
    fold_partial_row<V, VEC>(red, acc, L, p, partial + (int64_t)blockIdx.x * p);
}

// One pass over the [n][p] state: vhat = v~ / alpha in registers; hbar <- h - c1 hbar; x <- x + c2 hbar (x keeps its bits where
// c2 = 0: a finished column); h <- vhat - c3 h; partial |x|^2 per workgroup.
template <typename V, int VEC>
__global__ __launch_bounds__(kBlock) void lsmr_update_kernel(int64_t n, int64_t p, V* __restrict__ x, const V* __restrict__ v,
                                                             V* __restrict__ h, V* __restrict__ hbar, const double* __restrict__ scal,
                                                             const int* __restrict__ flags, int lpr, int rpp, V* __restrict__ partial) {
    __shared__ V red[kBlock * VEC];
    if (flags[0] != 0) return;
    const Lanes L = lanes<VEC>(p, lpr, rpp);
    V c1[VEC], c2[VEC], c3[VEC], ad[VEC], acc[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        acc[k] = 0;
        c1[k] = L.on ? (V)scal[kLsC1 * p + L.c + k] : (V)0;
        c2[k] = L.on ? (V)scal[kLsC2 * p + L.c + k] : (V)0;
        c3[k] = L.on ? (V)scal[kLsC3 * p + L.c + k] : (V)0;
        ad[k] = L.on ? (V)scal[kLsAlphaDiv * p + L.c + k] : (V)1;
    }
    for_rows(L, n, [&](int, int64_t row) {
        const int64_t o = row * p + L.c;
        V xv[VEC], vv[VEC], hv[VEC], hb[VEC];
        load_vec<V, VEC>(x + o, xv);
        load_vec<V, VEC>(v + o, vv);
        load_vec<V, VEC>(h + o, hv);
        load_vec<V, VEC>(hbar + o, hb);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            hb[k] = hv[k] - c1[k] * hb[k];
            if (c2[k] != (V)0) xv[k] = xv[k] + c2[k] * hb[k];
            hv[k] = vv[k] / ad[k] - c3[k] * hv[k];
            acc[k] = fma(xv[k], xv[k], acc[k]);
        }
        store_vec<V, VEC>(hbar + o, hb);
        store_vec<V, VEC>(x + o, xv);
        store_vec<V, VEC>(h + o, hv);
    });
    fold_partial_row<V, VEC>(red, acc, L, p, partial + (int64_t)blockIdx.x * p);
}

}  // namespace tsgu

using namespace tsgu;

extern "C" {

int tsgu_lsmr_scal_rows(void) { return kLsRows; }

int tsgu_lsmr_scalar(int vtype, int phase, const void* partial, int64_t n_partial, void* fold, void* scal, int* flags, double damp,
                     double atol, double btol, double ctol, double eps, int64_t p, int device, void* stream) {
    if (!scal || !flags || !partial || p <= 0 || p > 1024 || n_partial < 0 || phase < kLsBeta || phase > kLsStop) return TSGU_ERR_BAD_ARG;
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return with_value_type(vtype, [&](auto tag) -> int {
        using V = decltype(tag);
        const V* src;
        int64_t rows;
        if (const int rc = fold_partials<V>(partial, n_partial, p, fold, true, flags, s, src, rows)) return rc;
        return launch(lsmr_scalar_kernel<V>, 1, s, phase, src, rows, p, (double*)scal, flags, damp, atol, btol, ctol, eps);
    });
}

int tsgu_lsmr_vector(int vtype, int which, int64_t n, int64_t p, void* a0, const void* a1, void* a2, void* a3, const void* scal,
                     const int* flags, void* partial, int device, void* stream) {
    if (n <= 0 || p <= 0 || !a0 || !a1 || !scal || !flags || !partial || which < kLsBidiag || which > kLsUpdate) return TSGU_ERR_BAD_ARG;
    if (which == kLsUpdate && (!a2 || !a3)) return TSGU_ERR_BAD_ARG;
    if (!(aligned16(a0) && aligned16(a1) && aligned16(a2) && aligned16(a3))) return TSGU_ERR_BAD_ARG;
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return with_value_type(vtype, [&](auto tag) -> int {
        using V = decltype(tag);
        constexpr int wide = VT<V>::kWide;
        if (which == kLsBidiag)
            return launch_lanes<V>(n, p, lsmr_bidiag_kernel<V, 1>, lsmr_bidiag_kernel<V, wide>, [&](auto kern, const VecGeom& g) {
                return launch(kern, g.blocks, s, n, p, (V*)a0, (const V*)a1, (const double*)scal, flags, g.lpr, g.rpp, (V*)partial);
            });
        return launch_lanes<V>(n, p, lsmr_update_kernel<V, 1>, lsmr_update_kernel<V, wide>, [&](auto kern, const VecGeom& g) {
            return launch(kern, g.blocks, s, n, p, (V*)a0, (const V*)a1, (V*)a2, (V*)a3, (const double*)scal, flags, g.lpr, g.rpp,
                          (V*)partial);
        });
    });
}

}  // extern "C"
