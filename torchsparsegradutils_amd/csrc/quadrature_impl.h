// K10: Gauss quadrature of Lanczos tridiagonal matrices (contracts in tsgu_hip_quadrature.h) and the Rademacher probe block.
//
// tridiag_quadrature_kernel: one lane per column, workgroups of one wave.  A lane builds its own tridiagonal matrix from column c of
//          `coef` (CG coefficients or the entries themselves), finds where it ends, and runs the implicit QL iteration with Wilkinson
//          shifts on it, carrying only the first row of the eigenvector matrix (Golub-Welsch): the eigenvalues are the nodes, the
//          squares of that row the weights.  Everything is float64 whatever the value type.  The three length-r arrays of a lane
//          (diagonal, off-diagonal, first row) are [row][lane] in LDS — lane l of row i at word i * 64 + l, conflict-free for 8-byte
//          words — or, above kQuadLdsRows rows, [row][column] in the caller's work buffer.  No lane reads another lane's words, so
//          there is no barrier: lanes of different lengths and sweep counts simply diverge.
// rademacher_fill_kernel: out[i][c] = +-1 from the lowbias32 hash of (seed, i, c), one thread per element.
#pragma once

#include "amg_impl.h"          // amg_lowbias32
#include "tsgu_common.h"

namespace tsgu {

constexpr int kQuadCap = 128;          // the largest r (tsgu_quadrature_geometry)
constexpr int kQuadLdsRows = 100;      // r up to here: the arrays live in LDS (3 * 8 * 64 * r = 1536 r bytes <= 153 600)
constexpr int kQuadNoWorkRows = 64;    // the header's promise: `work` is not needed up to here (<= kQuadLdsRows)
constexpr int kQuadLanes = 64;         // columns per workgroup
constexpr int kQuadSweeps = 64;        // QL sweeps per eigenvalue before the block is deflated by force (never met in practice)
constexpr int kQuadMaxLds = 3 * 8 * kQuadLanes * kQuadLdsRows;
static_assert(kQuadNoWorkRows <= kQuadLdsRows && kQuadMaxLds <= 160 * 1024, "the LDS form must fit one CU");

enum QuadKind { kQuadCg = 0, kQuadEntries = 1 };
enum QuadFn { kQuadLog = 0, kQuadReciprocal = 1, kQuadIdentity = 2, kQuadOne = 3 };

struct QuadParams {
    int kind, fn, r;
    int64_t p;
    const void* coef;
    const void* scale;
    void* out;
    int* info;
    double* work;
};

// a lane's view of one of its arrays: element i at base[i * stride]
struct QuadArray {
    double* base;
    int64_t stride;
    __host__ __device__ __forceinline__ double& operator[](int i) const { return base[(int64_t)i * stride]; }
};

__host__ __device__ __forceinline__ bool quad_positive_finite(double v) { return v > 0.0 && v < __builtin_inf(); }

// The tridiagonal matrix of a column and its length (tsgu_hip_quadrature.h, "Column length"): d, e as the QL iteration takes them
// (e[i] = T[i, i + 1], e[len - 1] = 0), z = the first unit vector.
// (quad_build and quad_ql are also host functions: a CPU program can run the very arithmetic of the kernel, under a sanitizer too)
template <typename V>
__host__ __device__ __forceinline__ int quad_build(int kind, int r, int64_t p, const V* __restrict__ coef, const QuadArray d,
                                                   const QuadArray e, const QuadArray z) {
    int len = 0;
    double carry = 0.0;          // beta_{k-1} / alpha_{k-1}
    for (int k = 0; k < r; ++k) {
        const double a = (double)coef[((int64_t)2 * k) * p], b = (double)coef[((int64_t)2 * k + 1) * p];
        if (kind == kQuadCg) {
            if (!quad_positive_finite(a)) break;
            const double ia = 1.0 / a;
            d[k] = ia + carry;
            z[k] = k == 0 ? 1.0 : 0.0;
            len = k + 1;
            if (!quad_positive_finite(b)) break;
            e[k] = sqrt(b) * ia;
            carry = b * ia;
        } else {
            d[k] = a;
            z[k] = k == 0 ? 1.0 : 0.0;
            len = k + 1;
            if (b == 0.0 || !(fabs(b) < __builtin_inf())) break;
            e[k] = b;
        }
    }
    if (len > 0) e[len - 1] = 0.0;
    return len;
}

// Implicit QL with Wilkinson shifts on (d, e) of length n; z is rotated along (the first row of the eigenvector matrix).
__host__ __device__ __forceinline__ void quad_ql(int n, const QuadArray d, const QuadArray e, const QuadArray z) {
    for (int l = 0; l < n; ++l) {
        for (int sweep = 0;; ++sweep) {
            int m = l;
            for (; m < n - 1; ++m) {
                const double dd = fabs(d[m]) + fabs(d[m + 1]);
                if (fabs(e[m]) + dd == dd) break;
            }
            if (m == l) break;
            if (sweep == kQuadSweeps) {
                e[l] = 0.0;
                break;
            }
            const double el = e[l];
            double g = (d[l + 1] - d[l]) / (2.0 * el);
            double rr = hypot(g, 1.0);
            g = d[m] - d[l] + el / (g + copysign(rr, g));
            double s = 1.0, c = 1.0, pp = 0.0;
            int i = m - 1;
            for (; i >= l; --i) {
                const double ei = e[i];
                double f = s * ei;
                const double b = c * ei;
                rr = hypot(f, g);
                e[i + 1] = rr;
                if (rr == 0.0) {
                    d[i + 1] -= pp;
                    e[m] = 0.0;
                    break;
                }
                s = f / rr;
                c = g / rr;
                g = d[i + 1] - pp;
                rr = (d[i] - g) * s + 2.0 * c * b;
                pp = s * rr;
                d[i + 1] = g + pp;
                g = c * rr - b;
                f = z[i + 1];
                const double zi = z[i];
                z[i + 1] = s * zi + c * f;
                z[i] = c * zi - s * f;
            }
            if (rr == 0.0 && i >= l) continue;
            d[l] -= pp;
            e[l] = g;
            e[m] = 0.0;
        }
    }
}

template <typename V, bool LDS>
__global__ __launch_bounds__(kQuadLanes) void tridiag_quadrature_kernel(const QuadParams P) {
    extern __shared__ __attribute__((aligned(16))) double quad_lds[];
    const int lane = threadIdx.x;
    const int64_t c = (int64_t)blockIdx.x * kQuadLanes + lane;
    if (c >= P.p) return;
    QuadArray d, e, z;
    if constexpr (LDS) {
        d = {quad_lds + lane, kQuadLanes};
        e = {quad_lds + (int64_t)P.r * kQuadLanes + lane, kQuadLanes};
        z = {quad_lds + (int64_t)2 * P.r * kQuadLanes + lane, kQuadLanes};
    } else {
        d = {P.work + c, P.p};
        e = {P.work + (int64_t)P.r * P.p + c, P.p};
        z = {P.work + (int64_t)2 * P.r * P.p + c, P.p};
    }
    const int len = quad_build<V>(P.kind, P.r, P.p, (const V*)P.coef + c, d, e, z);
    quad_ql(len, d, e, z);
    double sum = 0.0;
    bool bad = false;
    for (int j = 0; j < len; ++j) {
        const double lam = d[j], w = z[j] * z[j];
        double f = 1.0;
        if (P.fn == kQuadLog || P.fn == kQuadReciprocal) {
            if (!(lam > 0.0)) bad = true;
            f = P.fn == kQuadLog ? log(lam) : 1.0 / lam;
        } else if (P.fn == kQuadIdentity) {
            f = lam;
        }
        sum += w * f;
    }
    const double sc = P.scale != nullptr ? (double)((const V*)P.scale)[c] : 1.0;
    ((V*)P.out)[c] = bad ? (V)__builtin_nan("") : (V)(sc * sum);
    P.info[c] = bad ? -len : len;
}

// out[i][c] = +-1: the sign bit of lowbias32(c + lowbias32(i + s)), s = lowbias32(lo(seed) ^ lowbias32(hi(seed))), 32-bit wrapping sums
template <typename V>
__global__ __launch_bounds__(kBlock) void rademacher_fill_kernel(int64_t n, int64_t p, unsigned s, V* __restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (idx >= n * p) return;
    const int64_t i = idx / p, c = idx - i * p;
    const unsigned h = amg_lowbias32((unsigned)c + amg_lowbias32((unsigned)i + s));
    out[idx] = (h >> 31) ? (V)-1 : (V)1;
}

inline unsigned rademacher_seed_word(int64_t seed) {
    auto mix = [](unsigned x) {
        x ^= x >> 16;
        x *= 0x7feb352du;
        x ^= x >> 15;
        x *= 0x846ca68bu;
        x ^= x >> 16;
        return x;
    };
    const uint64_t u = (uint64_t)seed;
    return mix((unsigned)(u & 0xffffffffu) ^ mix((unsigned)(u >> 32)));
}

}  // namespace tsgu
