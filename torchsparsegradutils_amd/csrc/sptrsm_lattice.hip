// K4 on stencil factors: the triangular solve as a LINE SWEEP over a row-major lattice.
//
// The sync-free sweep (csrc/sptrsm.hip) pays one ticket atomic and the dependent chain ptr -> idx -> poll per ROW.  When the
// factor's pattern is a stencil on a lattice (a tsgu_trsm_lattice_plan, derived from the lattice plan's class tables on the host:
// _lattice.trsm_tables) a wave owns a whole z-LINE — the nz consecutive rows (item, x, y, ·) — and solves its rows in z order:
//   * the dependencies on the same line (dz = -1, -2; +1, +2 for an upper sweep) never leave the wave: the last two solutions stay
//     in registers, no memory hop, no ticket;
//   * lines are drawn from ONE ticket counter in the order (item, x, y) ascending (descending for an upper sweep): one atomic per
//     line (per group of lines on lattices with very many short lines), not per row.  Forward progress is the argument of sptrsm.hip applied to lines: every dependency of a line lies on the
//     line itself or on a line with a smaller ticket (that is what makes a plan eligible), and a ticket is only ever taken by a wave
//     that is already running;
//   * neighbour rows, value positions and row lengths come from the class table in LDS (one record per class and visiting position),
//     not from crow / col / perm;
//   * values, right-hand sides and row classes do not depend on anything: a wave stages them in LDS one chunk of rows ahead of the
//     rows that wait for their dependencies;
//   * the cross-line hand-off is the measured mechanism of sptrsm.hip and nothing else: X pre-filled with the NaN tag, one
//     agent-scope store per published element, relaxed agent-scope polls with a sleep, every spin bounded by the wall clock and the
//     error word of TrsmWork.
// The arithmetic order is that of sptrsm_syncfree_kernel exactly (lane = column·EP + entry, rounds of EP stored entries, fma per
// lane, entry_sum tree, one division), so the solution is the same BITS whatever the schedule.
#include "sptrsm_common.h"

namespace tsgu {

// record of one (class, visiting position): `off` = neighbour row − own row (class-constant: a plan is only eligible when it is),
// `info` = value position (kind 0: inside the own row = the visiting position; kind 1: inside the SOURCE row, the plan's ksrc)
// | flags
constexpr int kTlUsedLower = 1 << 8;    // the entry lies strictly below the diagonal
constexpr int kTlUsedUpper = 1 << 9;    // … strictly above
constexpr int kTlDiag = 1 << 10;
constexpr int kTlInline = 1 << 11;      // neighbour on the own line (|off| = 1 or 2): read from the wave's registers

// what a lane keeps of one round of a row: the value, the neighbour's solution as far as it has arrived, its row, flags
constexpr int kTlPre = 4;               // rounds of the NEXT row that are requested ahead (rows of up to 4·EP entries: all of them)
constexpr int kTlFDiag = 1, kTlFNeed = 2, kTlFMem = 4, kTlFDist2 = 8;
template <typename A, typename Bits>
struct TlRound {
    A a;
    Bits xb;
    int64_t j;
    int f;
};
template <typename A, typename Bits>
struct TlRow {
    TlRound<A, Bits> rd[kTlPre];
    A rhs;
    int64_t row;
    int r, cls, len;
};

struct TrsmLatParams {
    tsgu_trsm_lattice_plan plan;
    int64_t n, nnz, p;
    const void* val;
    const void* B;
    int64_t ldb, bcs;
    void* X;
    int64_t ldx;
    TrsmWork* work;
    int lower, unit;
    int ch;                   // rows staged at a time
    int group;                // lines per ticket
    long long timeout_ticks;
};

template <typename V>
__host__ __device__ constexpr int tl_wave_bytes(int ch, int width, int cl) {
    // per wave: values [ch][width] | right-hand sides [ch][cl] | classes [ch] (padded to 16 bytes)
    return ch * width * (int)sizeof(V) + ch * cl * (int)sizeof(V) + (ch + 15) / 16 * 16;
}

__device__ __forceinline__ void tl_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <typename V, int CL>
__global__ __launch_bounds__(kBlock) void sptrsm_lattice_kernel(const TrsmLatParams P) {
    using S = Sentinel<V>;
    using Bits = typename S::Bits;
    using A = typename VT<V>::Acc;
    constexpr int EP = kWave / CL;
    extern __shared__ __attribute__((aligned(16))) unsigned char tl_smem[];

    const int lane = threadIdx.x & (kWave - 1);
    const int slot = threadIdx.x / kWave;
    const int cl = lane / EP;
    const int ep = lane % EP;
    const bool col_ok = cl < P.p;

    const int W = P.plan.width, ncls = P.plan.ncls, nz = P.plan.nz, CH = P.ch;
    const int uniform = P.plan.uniform_len;
    const bool kind1 = P.plan.kind != 0;
    const int used_bit = P.lower ? kTlUsedLower : kTlUsedUpper;

    // LDS: class records [ncls][W] int2 | class lengths [ncls] int | per-wave staging
    int2* const tab = reinterpret_cast<int2*>(tl_smem);
    int* const clen = reinterpret_cast<int*>(tab + ncls * W);
    unsigned char* const wave0 = tl_smem + ((ncls * W * 8 + ncls * 4 + 15) / 16 * 16) + slot * tl_wave_bytes<V>(CH, W, CL);
    V* const sval = reinterpret_cast<V*>(wave0);
    V* const srhs = sval + CH * W;
    unsigned char* const scls = reinterpret_cast<unsigned char*>(srhs + CH * CL);

    {
        const int2* __restrict__ gtab = static_cast<const int2*>(P.plan.tab);
        const unsigned char* __restrict__ glen = static_cast<const unsigned char*>(P.plan.lens);
        for (int i = threadIdx.x; i < ncls * W; i += kBlock) tab[i] = gtab[i];
        for (int i = threadIdx.x; i < ncls; i += kBlock) clen[i] = glen[i];
    }
    __syncthreads();      // the only workgroup barrier: from here on the four waves are independent

    const unsigned char* __restrict__ rcls = static_cast<const unsigned char*>(P.plan.rcls);
    const int32_t* __restrict__ rstart = static_cast<const int32_t*>(P.plan.rstart);
    const V* __restrict__ val = static_cast<const V*>(P.val);
    const V* __restrict__ B = static_cast<const V*>(P.B);
    Bits* X = static_cast<Bits*>(P.X);
    TrsmWork* work = P.work;
    unsigned long long* const counter = &work->class_ticket[0];
    const int64_t nlines = P.plan.nlines;

    // a ticket is a GROUP of `P.group` consecutive lines of the sweep order, solved one after the other by the wave that drew it
    // (group = 1 unless the lattice has very many short lines: one counter serves ~80 M atomics per second).  Progress as for
    // single lines: a dependency lies on an earlier line of the own group (finished) or in a group with a smaller ticket.
    int64_t gnext = 0, gend = 0;
    for (;;) {
        if (gnext >= gend) {
            unsigned long long t = 0;
            if (lane == 0) t = __hip_atomic_fetch_add(counter, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            t = __shfl(t, 0, kWave);
            if (t >= (unsigned long long)((nlines + P.group - 1) / P.group)) break;
            gnext = (int64_t)t * P.group;
            gend = gnext + P.group < nlines ? gnext + P.group : nlines;
        }
        const int64_t ticket = gnext++;
        const int64_t line = P.lower ? ticket : nlines - 1 - ticket;
        const int64_t row0 = line * nz;

        A xm1 = 0, xm2 = 0;      // the line's last two solutions of this lane's column
        bool dead = false;
        for (int s0 = 0; s0 < nz; s0 += CH) {
            const int rows = nz - s0 < CH ? nz - s0 : CH;
            // ---- stage the chunk: step s0 + r of the sweep is row z = s0 + r (lower) or nz - 1 - s0 - r (upper) ----
            // The staging area belongs to this wave alone; lanes write entries that OTHER lanes of the wave read.  What orders them:
            // a wave's LDS operations are executed in program order, and the wavefront-scope release / acquire fences below keep
            // the compiler from moving LDS accesses across the points where the roles change (the wave barrier alone is only a
            // scheduling barrier).  No workgroup barrier: the four waves never wait for each other.
            tl_wave_sync();
            for (int r = lane; r < rows; r += kWave) {
                const int z = P.lower ? s0 + r : nz - 1 - s0 - r;
                const int c = rcls[row0 + z];
                scls[r] = (unsigned char)(c < ncls ? c : ncls - 1);
            }
            for (int i = lane; i < rows * CL; i += kWave) {
                const int r = i / CL, c = i - r * CL;
                const int z = P.lower ? s0 + r : nz - 1 - s0 - r;
                V b{};
                if (c < P.p) b = B[(row0 + z) * P.ldb + c * P.bcs];
                srhs[i] = b;
            }
            tl_wave_sync();
            for (int i = lane; i < rows * W; i += kWave) {
                const int r = i / W, k = i - r * W;
                const int z = P.lower ? s0 + r : nz - 1 - s0 - r;
                const int cls = scls[r];
                V a{};
                if (k < clen[cls]) {
                    const int2 e = tab[cls * W + k];
                    const int64_t src = row0 + z + (kind1 ? e.x : 0);
                    if (src >= 0 && src < P.n) {       // (always, for the tables of an eligible plan: no access depends on it)
                        const int64_t at = (uniform ? src * uniform : (int64_t)rstart[src]) + (kind1 ? (e.y & 0xff) : k);
                        if (at >= 0 && at < P.nnz) a = val[at];
                    }
                }
                sval[i] = a;
            }
            tl_wave_sync();

            // One row ahead: the records, the value and the FIRST poll of every entry of the next row are requested before the
            // current row waits for its dependencies.  Entries of lines that are long finished (plane x - 1) arrive while the
            // current row is solved and are never polled again; only the entries that still hold the tag are re-polled.
            auto fetch_round = [&](int64_t row, int len, const int2* rec, const V* rv, int base) {
                TlRound<A, Bits> q;
                q.a = 0;
                q.xb = S::kTag;
                q.j = 0;
                q.f = 0;
                // rounds of EP stored entries, farthest dependency first: ascending positions for a lower sweep, descending for an
                // upper one (as sptrsm_syncfree_kernel)
                const int k = P.lower ? base + ep : (len - 1) - base - ep;
                if (k >= 0 && k < len) {
                    const int2 e = rec[k];
                    q.a = VT<V>::up(rv[k]);
                    if (e.y & kTlDiag) {
                        q.f = kTlFDiag;
                    } else {
                        const int64_t j = row + e.x;
                        if (col_ok && (e.y & used_bit) && j >= 0 && j < P.n) {
                            q.f = kTlFNeed;
                            if (!(e.y & kTlInline)) {
                                q.f |= kTlFMem;
                                q.j = j;
                                q.xb = __hip_atomic_load(X + j * P.ldx + cl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            } else if (e.x == 2 || e.x == -2) {
                                q.f |= kTlFDist2;
                            }
                        }
                    }
                }
                return q;
            };
            auto fetch_row = [&](int r) {
                TlRow<A, Bits> w;
                const int z = P.lower ? s0 + r : nz - 1 - s0 - r;
                w.r = r;
                w.row = row0 + z;
                w.cls = __builtin_amdgcn_readfirstlane((int)scls[r]);
                w.len = __builtin_amdgcn_readfirstlane(clen[w.cls]);
                w.rhs = VT<V>::up(srhs[r * CL + cl]);
#pragma unroll
                for (int ri = 0; ri < kTlPre; ++ri) {
                    if (ri * EP < w.len) {
                        w.rd[ri] = fetch_round(w.row, w.len, tab + w.cls * W, sval + r * W, ri * EP);
                    } else {
                        w.rd[ri].a = 0;
                        w.rd[ri].xb = S::kTag;
                        w.rd[ri].j = 0;
                        w.rd[ri].f = 0;
                    }
                }
                return w;
            };

            TlRow<A, Bits> cur = fetch_row(0);
            for (int r = 0; r < rows; ++r) {
                TlRow<A, Bits> nxt = cur;
                if (r + 1 < rows) nxt = fetch_row(r + 1);
                const int64_t row = cur.row;
                const int len = cur.len;

                A acc = 0;
                A diag = 0;
                A dsum = 1;
                auto finish_round = [&](TlRound<A, Bits>& q) {
                    if (q.f & kTlFDiag) diag += q.a;
                    const bool mem = (q.f & kTlFMem) != 0;
                    long long t0 = 0;
                    for (unsigned spin = 0;; ++spin) {
                        if (!__any(mem && q.xb == S::kTag)) break;
                        if (spin) __builtin_amdgcn_s_sleep(1);
                        if (mem && q.xb == S::kTag) {
                            q.xb = __hip_atomic_load(X + q.j * P.ldx + cl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        }
                        if ((spin & 255u) == 255u) {
                            const long long now = wall_clock64();
                            if (t0 == 0) t0 = now;
                            if (now - t0 > P.timeout_ticks ||
                                __hip_atomic_load(&work->error, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) {
                                dead = true;
                                break;
                            }
                        }
                    }
                    if (!dead && (q.f & kTlFNeed)) {
                        const A x = mem ? S::val(q.xb) : ((q.f & kTlFDist2) ? xm2 : xm1);
                        acc = fma(q.a, x, acc);
                    }
                };
#pragma unroll
                for (int ri = 0; ri < kTlPre; ++ri) {
                    if (!dead && ri * EP < len) finish_round(cur.rd[ri]);
                }
                for (int base = kTlPre * EP; base < len && !dead; base += EP) {
                    TlRound<A, Bits> q = fetch_round(row, len, tab + cur.cls * W, sval + cur.r * W, base);
                    finish_round(q);
                }
                if (__any(dead)) {
                    dead = true;
                    break;
                }
                if (!P.unit) dsum = len > 0 ? entry_sum<A, EP>(diag) : A(0);     // (an empty row of a non-unit solve divides by zero)
                acc = entry_sum<A, EP>(acc);
                // every entry lane of the column holds the same sums: all of them keep the solution for the next rows of the line
                const A x = (cur.rhs - acc) / dsum;
                Bits xb = S::bits(x);
                if (x != x) xb = S::kCanon;
                if (ep == 0 && col_ok) __hip_atomic_store(X + row * P.ldx + cl, xb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                xm2 = xm1;
                xm1 = S::val(xb);
                cur = nxt;
            }
            if (dead) break;
        }
        if (dead) {
            if (lane == 0) __hip_atomic_store(&work->error, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            break;
        }
    }
}

template <typename V>
int sptrsm_lattice_launch(TrsmLatParams P, int n_cu, int workgroups, hipStream_t stream) {
    const int64_t n = (int64_t)P.plan.nlines * P.plan.nz;
    {
        int64_t nb = (n * P.p + kBlock - 1) / kBlock;
        if (nb > 4096) nb = 4096;
        hipLaunchKernelGGL((sptrsm_fill_kernel<V>), dim3((unsigned)nb), dim3(kBlock), 0, stream, P.X, P.ldx, n, P.p, P.work);
        if (const int rc = check_launch()) return rc;
    }
    const int cl = next_pow2(P.p);
    // rows staged at a time: 32, fewer when the workgroup's LDS would pass 64 KiB
    const int fixed = (P.plan.ncls * P.plan.width * 8 + P.plan.ncls * 4 + 15) / 16 * 16;
    int ch = 32;
    while (ch > 1 && fixed + kTrsmWaves * tl_wave_bytes<V>(ch, P.plan.width, cl) > 64 * 1024) ch /= 2;
    const int lds = fixed + kTrsmWaves * tl_wave_bytes<V>(ch, P.plan.width, cl);
    if (lds > 64 * 1024) return TSGU_ERR_TOO_LARGE;
    P.ch = ch;
    // lines per ticket: at most ~16 K tickets on the one counter (0.2 ms of same-address atomics, spread over the sweep)
    P.group = (int)((P.plan.nlines + 16383) / 16384);
    if (P.group < 1) P.group = 1;
    // persistent grid of 4-wave workgroups; 0 = the fixed rule: a wave for every line a hyperplane front crosses (about
    // ny·nz / 4 per item for the half of a 27-point box), at least one workgroup per compute unit.  Never more than 8 per CU
    // (what stays resident) nor more waves than lines.  Speed only: the ticket order alone guarantees progress.
    int64_t blocks = workgroups;
    if (blocks < 1) {
        blocks = ((int64_t)P.plan.front_lines + kTrsmWaves - 1) / kTrsmWaves;
        if (blocks < n_cu) blocks = n_cu;
    }
    if (blocks > (int64_t)n_cu * 8) blocks = (int64_t)n_cu * 8;
    const int64_t need = (((int64_t)P.plan.nlines + P.group - 1) / P.group + kTrsmWaves - 1) / kTrsmWaves;
    if (blocks > need) blocks = need;
    const dim3 grid((unsigned)blocks, 1, 1);
    dispatch_pow2<1, 64>(cl, [&](auto n) {
        hipLaunchKernelGGL((sptrsm_lattice_kernel<V, decltype(n)::value>), grid, dim3(kBlock), (size_t)lds, stream, P);
    });
    return check_launch();
}

}  // namespace tsgu

using namespace tsgu;

extern "C" {

int tsgu_csr_sptrsm_lattice(int vtype, const tsgu_trsm_lattice_plan* plan, int64_t nnz, const void* val,
                            int lower, int unit,
                            const void* B, int64_t ldb, int64_t b_col_stride, void* X, int64_t ldx, int64_t p,
                            void* work, int workgroups, int device, void* stream) {
    if (!plan || nnz < 0 || p < 0) return TSGU_ERR_BAD_ARG;
    if (plan->nlines < 0 || plan->nz < 1 || plan->ncls < 1 || plan->ncls > 255 || plan->width < 1 || plan->width > 32 ||
        plan->uniform_len < 0 || plan->uniform_len > 32)
        return TSGU_ERR_BAD_ARG;
    const int64_t n = (int64_t)plan->nlines * plan->nz;
    if (n == 0 || p == 0) return TSGU_OK;
    if (p > 64) return TSGU_ERR_TOO_LARGE;       // one column tile: wider operands stay on tsgu_csr_sptrsm
    if (!plan->tab || !plan->lens || !plan->rcls || (!plan->uniform_len && !plan->rstart) || !val || !B || !X || !work)
        return TSGU_ERR_BAD_ARG;
    if (plan->uniform_len && n * plan->uniform_len > nnz) return TSGU_ERR_BAD_ARG;
    if (b_col_stride < 1 || ldb < 1 || (b_col_stride == 1 && ldb < p) || ldx < p || B == X) return TSGU_ERR_BAD_ARG;
    if (const int rc = set_device(device)) return rc;
    const int n_cu = device_cu_count(device);
    if (n_cu == 0) return TSGU_ERR_RUNTIME;
    TrsmLatParams P{};
    P.plan = *plan;
    P.n = n;
    P.nnz = nnz;
    P.p = p;
    P.val = val;
    P.B = B;
    P.ldb = ldb;
    P.bcs = b_col_stride;
    P.X = X;
    P.ldx = ldx;
    P.work = static_cast<TrsmWork*>(work);
    P.lower = lower;
    P.unit = unit;
    P.timeout_ticks = 400000000LL;  // 4 s at the 100 MHz wall clock
    hipStream_t s = static_cast<hipStream_t>(stream);
    return with_value_type(vtype, [&](auto v) { return sptrsm_lattice_launch<decltype(v)>(P, n_cu, workgroups, s); });
}

}  // extern "C"
