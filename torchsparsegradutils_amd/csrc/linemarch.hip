// Whole-line plane march (linemarch_impl.h): bf16 instantiations and the launcher the march entry points (march.hip) call.
#include "linemarch_impl.h"

namespace tsgu {

// fills P from the plan (geometry, tile) and validates it; returns the dynamic LDS bytes or a negative status
int linemarch_fill(LineParams& P, const tsgu_march_plan* pl, int mode, int64_t p, int64_t n_rows, int64_t nnz) {
    if (!pl || p != 16) return TSGU_ERR_BAD_DTYPE;
    if (pl->ntap != 9 || pl->ry != 1 || pl->rz != 1 || pl->mask != (1u << 27) - 1u || (pl->periodic & 7) != 7 || pl->uniform_len != 27) return TSGU_ERR_BAD_ARG;
    if (pl->nb <= 0 || pl->nx < 3 || pl->ny < 3 || pl->nz < 3 || pl->nseg <= 0 || pl->nseg > pl->nx || pl->tz != pl->nz) return TSGU_ERR_BAD_ARG;
    if (n_rows >= 0 && (!lattice_has_rows(*pl, n_rows) || 27 * n_rows != nnz)) return TSGU_ERR_BAD_ARG;
    if (nnz > 0x7fffffffLL || nnz * 2 + 16 > 0xffffffffLL) return TSGU_ERR_TOO_LARGE;
    P.nb = pl->nb, P.nx = pl->nx, P.ny = pl->ny, P.nz = pl->nz;
    P.ty = pl->ty;
    P.tiles_y = pl->ny / (pl->ty > 0 ? pl->ty : 1);
    if (!split_x(P, *pl)) return TSGU_ERR_BAD_ARG;
    const int lds = linemarch_layout(P, pl->threads, mode);
    if (lds < 0) return lds;
    if (const int rc = set_workgroups(P, (int64_t)P.nb * P.nseg * P.tiles_y)) return rc;
    return lds;
}

int linemarch_run(int mode, const LineParams& P, int threads, hipStream_t stream) {
    int rc = TSGU_ERR_BAD_ARG;      // a mode, workgroup size or line length without a kernel
    auto run = [&](auto m) {
        dispatch_pow2<256, 1024>(threads, [&](auto nt) {
            dispatch_pow2<8, 64>(P.nz, [&](auto nz) { rc = linemarch_launch_t<decltype(nt)::value, decltype(nz)::value, decltype(m)::value>(P, stream); });
        });
    };
    if (mode == kLatSpmmT) run(std::integral_constant<int, kLatSpmmT>{});
    else if (mode == kLatSpmm) run(std::integral_constant<int, kLatSpmm>{});
    else if (mode == kLatSddmm) run(std::integral_constant<int, kLatSddmm>{});
    return rc;
}

}  // namespace tsgu
