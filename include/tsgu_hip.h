/*
 * tsgu_hip.h — C ABI of the MI355X (gfx950) sparse hot path.
 *
 * This is the drop-in boundary of the build: every entry point replaces one ATen
 * call site of the reference (cai4cai/torchsparsegradutils).  The reference has no
 * native code, so there is no FFI to mirror; the functions below are what a binding
 * for its hot path would call.  For every entry the replaced reference line is cited
 * (paths relative to the reference checkout).
 *
 * Conventions
 *   - plain pointers + sizes; no torch / C++ types; nothing throws across the ABI.
 *   - all pointers are DEVICE pointers unless the name ends in `_host`.
 *   - every launcher returns TSGU_OK (0) or a negative tsgu_status; it never syncs
 *     the stream and never allocates device memory (workspaces and plans are passed in).
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream);
 *     `device` is the HIP ordinal the pointers live on.
 *   - dense operands are row-major with an explicit leading dimension (elements).
 *   - value dtype / index dtype are run-time enums (tsgu_vtype / tsgu_itype).
 *   - CSR column indices inside a row need NOT be sorted or unique.
 *   - batched CSR (torch layout): crow [batch][n_rows+1], col/val [batch][nnz_per_item];
 *     every item's crow starts at 0.  batch == 1 for plain 2-D matrices.
 */
#ifndef TSGU_HIP_H
#define TSGU_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TSGU_ABI_VERSION 7

typedef enum {
    TSGU_OK = 0,
    TSGU_ERR_BAD_DTYPE = -1,     /* unsupported vtype/itype combination        */
    TSGU_ERR_BAD_ARG = -2,       /* null pointer, negative size, bad leading dimension */
    TSGU_ERR_TOO_LARGE = -3,     /* n_cols >= 2^31 or grid limit exceeded     */
    TSGU_ERR_LAUNCH = -4,        /* hipLaunchKernel / hipGetLastError failed  */
    TSGU_ERR_RUNTIME = -5,       /* other HIP runtime failure                 */
    TSGU_ERR_RESERVED_6 = -6,    /* (unused; kept so that the numbering of -7 is stable) */
    TSGU_ERR_TIMEOUT = -7        /* bounded device spin expired (sptrsm)       */
} tsgu_status;

typedef enum { TSGU_F32 = 0, TSGU_F64 = 1, TSGU_BF16 = 2 } tsgu_vtype;
typedef enum { TSGU_I32 = 0, TSGU_I64 = 1 } tsgu_itype;

/* Library / device introspection (no reference counterpart). */
int tsgu_abi_version(void);
const char* tsgu_status_string(int status);
/* Fills name (<= cap bytes), compute-unit count and wavefront size of `device`. */
int tsgu_device_info(int device, char* name, int cap, int* n_cu, int* wave_size);
/* The compute-unit count alone, by attribute query (microseconds; tsgu_device_info reads the whole property structure: ~0.1 s on first use). */
int tsgu_device_cu_count(int device, int* n_cu);
/* Streaming device copy (16 bytes per lane, non-temporal): the HBM ceiling the measurements are compared with. */
int tsgu_device_copy(const void* src, void* dst, int64_t bytes, int device, void* stream);

/*
 * 128-bit content fingerprint of an index array x[n] (itype) into out2[2] (uint64, device): two position-weighted sums in wrapping
 * 64-bit arithmetic, the same words whatever the launch geometry.  No reference counterpart: the reference keeps no per-pattern
 * state (sparse_matmul.py:141-163 re-derives everything per call), so it has no cliff when a caller rebuilds its index tensors
 * every step; the pattern cache here recognises such tensors by content (one pass over the indices) and adopts the existing plans.
 * accumulate = 0: out2 is zeroed first (one more device operation on the stream); 1: the sums are ADDED to what out2 holds (a caller
 * fingerprinting several arrays zeroes all their words with one fill).
 */
int tsgu_index_fingerprint(int itype, int64_t n, const void* x, void* out2, int accumulate, int device, void* stream);
/*
 * The same pass with an EXACT comparison and / or a copy: out3[0..1] += the fingerprint of x; when `ref` is given, out3[2] += a
 * count that is non-zero iff x[k] != ref[k] for some k; when `copy` is given, copy[k] = x[k].  The fingerprint only selects which
 * cached pattern a fresh index tensor is compared with — plans are adopted on out3[2] == 0, never on equal fingerprints alone
 * (a collision would silently compute with another matrix' pattern); `copy` is how the cache keeps the content it compares with
 * (it never holds the caller's tensors).  accumulate bit 0 as above (0: the three words are zeroed first); bit 1 (with ref, without copy):
 * COMPARE ONLY — the fingerprint words are left alone (equal tensors have their reference's fingerprint; the hashing is a third of the pass).
 */
int tsgu_index_fingerprint_match(int itype, int64_t n, const void* x, const void* ref, void* copy, void* out3, int accumulate,
                                 int device, void* stream);

/*
 * K1  C = A · B            (CSR × dense, optional fused column-dot epilogue)
 * replaces: torch.sparse.mm(A, B)            torchsparsegradutils/sparse_matmul.py:155
 *           A.matmul(p) in the Krylov loops  torchsparsegradutils/utils/linear_cg.py:322,
 *                                            utils/bicgstab.py:196,221
 *
 * perm (optional, itype, [nnz]): value indirection — entry k uses val[perm[k]].  This is
 * how Aᵀ·G (K2) runs on the cached transposed pattern without materialising Aᵀ's values:
 * replaces: torch.sparse.mm(A.t(), grad)     torchsparsegradutils/sparse_matmul.py:229
 *
 * b_col_stride / c_col_stride: element (i, c) of B / C sits at i·ld + c·col_stride.  1 = row-major.  Other values
 * serve the TRANSPOSED VIEWS the reference's sparse multivariate normal passes (`bvec.t()` / `permute`,
 * distributions/sparse_multivariate_normal.py:96,100: ld = 1, col_stride = n) without a copy: the kernel then takes
 * one column per grid.z slice with lanes along the rows.
 *
 * max_row_nnz: length of the longest row (0 = unknown).  Only a hint: with 16-byte dense rows and short sparse rows the
 * kernel gives every row ONE lane, unless this says that some row is far longer than the average (ragged patterns).
 *
 * dot_w / dot_partial (optional): when non-NULL the kernel also writes, per thread block,
 * partial[block][c] = sum_rows C[row,c] * W[row,c]  (fp32/fp64 accumulate), block-major,
 * ld = p.  W has leading dimension ldw.  `tsgu_spmm_num_blocks` gives the row count of
 * `dot_partial`.  Used for pᵀ(Ap) in CG (linear_cg.py:64-65).
 */
int tsgu_csr_spmm(int vtype, int itype,
                  int64_t n_rows, int64_t n_cols, int64_t nnz_per_item,
                  const void* crow, const void* col, const void* val, const void* perm,
                  const void* B, int64_t ldb, int64_t b_col_stride, int64_t b_batch_stride,
                  void* C, int64_t ldc, int64_t c_col_stride, int64_t c_batch_stride,
                  int64_t p, int64_t batch, int64_t max_row_nnz,
                  const void* dot_w, int64_t ldw, void* dot_partial,
                  int device, void* stream);

/* Number of thread blocks (per batch item) tsgu_csr_spmm uses for (n_rows, nnz_per_item, p, vtype). */
int64_t tsgu_spmm_num_blocks(int vtype, int64_t n_rows, int64_t nnz_per_item, int64_t p, int64_t max_row_nnz);

/*
 * Lane geometry of the plan-free kernels, answered on the host by the launchers' own rules (no device is touched; no reference
 * counterpart).  kernel: 0 = K1 / K2 (CSR SpMM), 1 = K3 (CSR SDDMM), 2 = the COO flavour of K3, 3 = the fused backward K2+K3
 * (n_rows = rows of the walked pattern: the columns of A).  wide_ok: every dense operand's base address, leading dimension and
 * batch stride allows 16-byte lanes.  col_strided (kernel 0 only): B / C have a column stride other than 1.
 * Out: vec elements per lane (1 or 16 bytes' worth), column_lanes x entry_lanes lanes per row (per entry for the COO flavour, where
 * entry_lanes is 1), column_tiles tiles of vec * column_lanes columns, row_runs runs of 256 / (column_lanes * entry_lanes) rows per
 * workgroup (kernel 0; 1 otherwise) and stage_entries, the stored entries a workgroup stages per pass.
 * TSGU_ERR_BAD_DTYPE: unknown vtype, F64 with kernel 3.  TSGU_ERR_BAD_ARG: unknown kernel, a negative size, a NULL output, and for
 * kernel 3 a width the launcher refuses (column_tiles != 1).
 */
int tsgu_csr_geometry(int kernel, int vtype, int64_t n_rows, int64_t nnz_per_item, int64_t p, int64_t max_row_nnz,
                      int wide_ok, int col_strided,
                      int* vec, int* column_lanes, int* entry_lanes, int64_t* column_tiles, int* row_runs, int* stage_entries);

/*
 * K3  out[k] = alpha * < G[row(k), :], B[col(k), :] >   for every stored entry k of A
 * (sparsity-masked SDDMM; no row-index expansion, no nnz×p temporaries)
 * replaces: repeat_interleave + 2×index_select + mul + sum
 *           torchsparsegradutils/sparse_matmul.py:186-205      (alpha = +1)
 *           torchsparsegradutils/sparse_solve.py:216-235       (alpha = -1, role swap when
 *                                                               transpose: pass G/B swapped
 *                                                               via `swap_roles`)
 *           torchsparsegradutils/sparse_solve.py:487-504       (alpha = -1)
 * swap_roles != 0 computes  alpha * < G[col(k), :], B[row(k), :] >  (sparse_solve.py:223-225).
 * out has vtype, [batch][nnz_per_item].
 */
int tsgu_csr_sddmm(int vtype, int itype,
                   int64_t n_rows, int64_t n_cols, int64_t nnz_per_item,
                   const void* crow, const void* col,
                   const void* G, int64_t ldg, int64_t g_batch_stride,
                   const void* B, int64_t ldb, int64_t b_batch_stride,
                   void* out, double alpha, int swap_roles,
                   int64_t p, int64_t batch,
                   int device, void* stream);

/*
 * COO flavour of K3 for un-coalesced COO inputs (explicit row indices, any order):
 * out[k] = alpha * < G[row[k], :], B[col[k], :] >
 * replaces: torchsparsegradutils/sparse_matmul.py:185,201-205 (COO branch)
 */
int tsgu_coo_sddmm(int vtype, int itype, int64_t nnz,
                   const void* row, const void* col,
                   const void* G, int64_t ldg, const void* B, int64_t ldb,
                   void* out, double alpha, int64_t p,
                   int device, void* stream);

/*
 * K2+K3 fused: the whole backward of C = A·B in one pass over the cached transposed pattern
 * (t_ptr[n_cols+1], t_idx[nnz] = row in A, t_perm[nnz] = position in A's value array):
 *   gradB[j,:]          = Σ_k∈col j  val[t_perm[k]] · G[t_idx[k],:]          (sparse_matmul.py:229)
 *   gradA_vals[t_perm[k]] = < G[t_idx[k],:], B[j,:] >                          (sparse_matmul.py:186-205)
 * Every upstream row G[i,:] is gathered once and used for both gradients (K2 and K3 run separately
 * gather 2·nnz dense rows).  fp32 / bf16, p <= 64·(16 bytes / element size); batched like K1.
 * Results are identical to K2 (same order) and to K3 up to the order-independent per-entry dot.
 */
int tsgu_csr_mm_backward(int vtype, int itype, int64_t n_rows, int64_t n_cols, int64_t nnz_per_item,
                         const void* t_ptr, const void* t_idx, const void* t_perm, const void* val,
                         const void* G, int64_t ldg, int64_t g_batch_stride,
                         const void* B, int64_t ldb, int64_t b_batch_stride,
                         void* gradA_vals, void* gradB, int64_t ldgb, int64_t gb_batch_stride,
                         int64_t p, int64_t batch, int device, void* stream);

/*
 * Row-pair gather kernels ("rowpack"): same reference lines as tsgu_csr_spmm (sparse_matmul.py:155,229) and
 * tsgu_csr_mm_backward (sparse_matmul.py:186-205,229).  One lane group owns rows 2q and 2q+1 and walks the sorted
 * UNION of their column sets, so a dense row both rows reference is gathered once (27-point stencil: 36 gathers
 * per pair instead of 54).  A workgroup of 256 threads = G lane groups (G = rows_per_block/2 from
 * tsgu_rowpack_geometry) owns G row pairs.  The plan is built once per sparsity pattern by the caller with index ops
 * and handed over as a struct of device pointers (all int32 / uint32 arrays):
 *
 * STREAM FORM (nclasses == 0) — one record per union entry / stored entry of the whole matrix
 *   uptr [nblocks·G+1]   union-entry offsets per lane-group slot (slot s of workgroup b = b·G + s)
 *   ucol [nu]            dense-row index of each union entry (ascending inside a pair when there is no upos; plans
 *                        with upos may list a pair's entries in any order — only the order of summation inside a row
 *                        follows it).  Without upos, bits 30 / 31
 *                        say whether row 2q / 2q+1 owns the column (n_cols < 2^30) and the value slots of a row are
 *                        consecutive in the workgroup's staged value slice.
 *   upos [nu]            optional: two 16-bit halves (low: row 2q, high: row 2q+1) = slot of that row's value in the
 *                        workgroup's staged value slice; bit 15 set = the row has no entry in this column.  Required
 *                        with sperm and whenever entry_lanes > 1.
 *   sperm[nnz]           optional (the walked pattern addresses the values through a permutation, e.g. the transposed
 *                        pattern): positions in the value array, ascending inside each workgroup's entry range; the
 *                        slots of upos index that order.  NULL: values are read in walked order.
 *   vpair[nblocks·G]     optional, with eptr[nblocks+1] and sperm: the row pair each lane-group slot owns (-1 = none),
 *                        so that a workgroup can own any set of pairs — e.g. a 3-D brick of a lattice, whose entries
 *                        form long runs in the value array — instead of G consecutive ones; eptr gives each
 *                        workgroup's range in sperm.  NULL = consecutive pairs.
 * CLASS-DICTIONARY FORM (nclasses > 0) — workgroups whose records are translations of each other share one copy.
 *   wcls [nblocks]       class of each workgroup
 *   wbase[nblocks][3]    {base pair, base column, base value position} added to the class's relative records
 *   uptr [nclasses][G+1] relative union offsets (first = 0, last = union entries of the class)
 *   ucol / upos [nclasses][ucap], sperm [nclasses][ecap], vpair [nclasses][G] (relative, -1 = none), cne[nclasses] =
 *                        stored entries per workgroup (with sperm).  eptr is unused.
 *   On lattice stencils (dozens of classes for millions of rows) the index streams — a third of the HBM traffic of
 *   the stream form — shrink to a few KB that stay in L2; results are bit-identical to the stream form.
 * ROW QUADS (rows_per_group = 4): a lane group owns FOUR consecutive rows (workgroup = 4·G rows); records as in the
 *                        form without upos, the four ownership bits in bits 28..31 of ucol (n_cols < 2^28); ecap up to twice
 *                        max_entries.  27-point stencil: 54 union columns per quad = 13.5 gathers per row instead of 18.  Only
 *                        for stored-order walks with one entry lane (forward SpMM, SDDMM).
 * order[nblocks]         optional (NULL = natural): workgroup b processes block order[b]; any permutation is valid.
 * ecap / ucap = capacity of the staged value slice / union records per workgroup (multiples of 256, within the limits
 * of tsgu_rowpack_geometry; ucap·(upos ? 8 : 4) + ecap·4 <= lds_budget_bytes).
 * fp32 and bf16 values (bf16: fp32 accumulation); p·sizeof(value)/16 in {2, 4, 8, 16} column lanes; 16-byte aligned
 * dense operands with 16-byte aligned rows; 2-D operands (batched problems are passed as their block-diagonal 2-D
 * form).  n_cols (n_cols_t) = rows of the gathered dense operand; below 2^24 rows and 4 GiB the kernels use 32-bit
 * gather offsets.  With entry_lanes == 1 each row's sum runs over its own entries in ascending stored order
 * (bit-identical to the one-group-per-row kernels when the records are listed in ascending order); with entry_lanes > 1 (narrow dense rows) the entries of a pair
 * are dealt round-robin to the entry lanes and combined by a fixed xor tree.  A row never touches a dense row it does
 * not reference (predicated update, no multiply by zero).
 */
typedef struct tsgu_rowpack_plan {
    int64_t nblocks;          /* workgroups */
    int32_t ecap, ucap;       /* LDS capacities (entries) */
    int32_t nclasses;         /* 0 = stream form */
    int32_t rows_per_group;   /* 0 or 2: row pairs; 4: row QUADS (stored-order walks without upos only) */
    const void* uptr;
    const void* ucol;
    const void* upos;
    const void* sperm;
    const void* order;
    const void* vpair;
    const void* eptr;
    const void* wcls;
    const void* wbase;
    const void* cne;
    const void* srcstart;     /* dictionary form with sperm, optional: int32 [rows of the value array's owner] first value position of
                                 every SOURCE row.  Then a record of sperm is (source row - the workgroup's first source row) << 8 |
                                 offset inside the row, and wbase[b][2] is the workgroup's first source row: positions relative to
                                 the source row are the same in translated workgroups even when rows of another length lie between
                                 them (a mesh with shorter rows at its faces), positions relative to the workgroup's first are not. */
} tsgu_rowpack_plan;

/* Geometry for (vtype, p): rows per workgroup, entry lanes per pair (> 1: plans need upos), plan limits. */
int tsgu_rowpack_geometry(int vtype, int64_t p, int* rows_per_block, int* entry_lanes, int* max_entries, int* max_union,
                          int* lds_budget_bytes);
int tsgu_csr_spmm_rowpack(int vtype, int itype, int64_t n_rows, int64_t n_cols, int64_t nnz, const void* ptr,
                          const tsgu_rowpack_plan* plan, const void* val, const void* B, int64_t ldb, void* C, int64_t ldc,
                          int64_t p, int device, void* stream);
/* (gradA values in A's order, gradB) in one walk over the transposed pattern's plan (needs sperm). */
int tsgu_csr_mm_backward_rowpack(int vtype, int itype, int64_t n_rows_t, int64_t n_cols_t, int64_t nnz, const void* t_ptr,
                                 const tsgu_rowpack_plan* plan, const void* val, const void* G, int64_t ldg, const void* B,
                                 int64_t ldb, void* gradA_vals, void* gradB, int64_t ldgb, int64_t p, int device, void* stream);
/* Row-pair SDDMM (plan of a pattern walked in stored order, without upos; replaces tsgu_csr_sddmm, reference
 * sparse_matmul.py:186-205, sparse_solve.py:223-235): out_vals[k] = alpha·<R[row k,:], Cm[col k,:]>.  The dense
 * rows of Cm that both rows of a pair reference are gathered once; the gradients leave in stored order with one
 * coalesced write per workgroup.  The G/B role swap of the solves is expressed by exchanging R and Cm. */
int tsgu_csr_sddmm_rowpack(int vtype, int itype, int64_t n_rows, int64_t n_cols, int64_t nnz, const void* ptr,
                           const tsgu_rowpack_plan* plan, const void* R, int64_t ldr, const void* Cm, int64_t ldc,
                           void* out_vals, double alpha, int64_t p, int device, void* stream);

/*
 * Row-block TILE kernels (general CSR patterns whose neighbouring rows share columns, no lattice needed: mesh orderings, banded
 * factors, FEM matrices — what the reference itself benchmarks, benchmarks/results/sparse_mm_suite_results.csv:5-6).
 * replaces: torch.sparse.mm(A, B) / torch.sparse.mm(A.t(), G)   torchsparsegradutils/sparse_matmul.py:155, :229
 *           the gather·mul·sum chain                            torchsparsegradutils/sparse_matmul.py:186-205
 * A persistent workgroup walks a run of row blocks (rows_per_block consecutive rows each).  The DISTINCT dense rows a block
 * references — its tile — are copied to LDS by 16-byte LDS-DMA one block ahead of the walk (double buffer), next to the block's
 * slice of the value array and ONE BYTE per entry naming the entry's dense row inside the tile; the walk reads a byte, a value and
 * 16 bytes of LDS per entry and keeps the accumulators in registers.  Plan (value independent, built once per pattern):
 *   desc [n_blocks + 4][8] int32 {u0, U, e0, E, c0, NC, x0, X}: block b's tile is ucol[u0 .. u0 + U) (ascending distinct columns, padded to
 *                          a multiple of 8 by repeating the last one; u0 a multiple of 8), its entries are e0 .. e0 + E of the walked
 *                          pattern, its value chunks (below) c0 .. c0 + NC; four trailing all-zero descriptors (the pipeline reads ahead)
 *   ucol                   int32 column numbers, U <= max_union per block
 *   lidx [nnz + 16]        uint8: position of entry k's column inside its block's tile (the SDDMM's walk)
 *   ent, xrow              the same as RECORDS for the forward / Aᵀ·G walk: a row's entries as whole rounds of eight uint16 = position in
 *                          the tile · 128 (the byte offset of the tile row), the last round padded with max_union · 128 (a row of zeros
 *                          the kernel keeps behind the tile); ent is 16-byte aligned, block b's records are ent[x0 .. x0 + X) (16 bytes
 *                          each, descriptor words 6, 7), row r's first record is x0 + xrow[r] (uint16; xrow is padded to whole blocks).
 *                          One aligned 16-byte LDS read and eight half-word adds per round where the byte stream costs three reads,
 *                          two byte shifts, eight extractions and eight shift-adds
 *   rptr [n_rows + 1]      int32 row pointer of the walked pattern
 *   cpos, cslot            optional (both or neither; NULL: values in walked order) — the plan of the TRANSPOSED pattern walks A's own
 *                          values (Aᵀ·G, sparse_matmul.py:229).  A block's values are fetched as CHUNKS of four consecutive values of
 *                          the value array, in ascending order of position: cpos[q] int32 = position of the chunk's first value
 *                          (cpos[q] + 4 <= nnz), cslot[q][0..3] uint16 = the entry of the block (0 .. E - 1) each of the four values
 *                          belongs to, 0xffff = none.  At most 1024 chunks per block.  The kernel loads a chunk with one 16-byte
 *                          load per lane (neighbouring lanes on neighbouring chunks) and scatters its values into the block's value
 *                          buffer in LDS.
 * fp32 values, p a multiple of 32 up to 1024 — ONE launch whatever the width: the pipeline's steps are (block, tile of 32 columns = 128
 * bytes of a dense row) pairs, a block's values / entry bytes / row pointers are staged once, and the SDDMM adds up the dots of a
 * block's column tiles on chip.  16-byte aligned dense operands, 2-D operands below 4 GiB.  Sums run in ascending
 * entry order of the walked pattern: the same bits as tsgu_csr_spmm / tsgu_csr_sddmm.  A row never touches a dense row it does not
 * reference.  tsgu_tile_geometry gives the limits a plan has to meet (or a negative status for an unsupported (vtype, p)).
 */
typedef struct tsgu_tile_plan {
    int64_t n_rows, n_cols, nnz;   /* of the walked pattern */
    int64_t n_blocks;
    int32_t rows_per_block, max_union, max_entries, reserved;
    const void* desc;
    const void* ucol;
    const void* lidx;
    const void* rptr;
    const void* cpos;
    const void* cslot;
    const void* ent;
    const void* xrow;
} tsgu_tile_plan;

int tsgu_tile_geometry(int vtype, int64_t p, int* rows_per_block, int* max_union, int* max_entries);
int tsgu_csr_spmm_tile(int vtype, const tsgu_tile_plan* plan, const void* val, const void* B, int64_t ldb, void* C, int64_t ldc,
                       int64_t p, int device, void* stream);
/* out_vals[k] = alpha·<R[row k,:], Cm[col k,:]> in the walked (stored) order; plan without perm. */
int tsgu_csr_sddmm_tile(int vtype, const tsgu_tile_plan* plan, const void* R, int64_t ldr, const void* Cm, int64_t ldc, void* out_vals,
                        double alpha, int64_t p, int device, void* stream);

/*
 * Lattice plane-sweep kernels ("lattice"): same reference lines as tsgu_csr_spmm (sparse_matmul.py:155,229) and
 * tsgu_csr_sddmm (sparse_matmul.py:186-205, sparse_solve.py:216-235,487-504), for patterns that are stencils on a
 * row-major lattice:  row = ((item·nx + x)·ny + y)·nz + z,  every stored entry (row, col) has col = the lattice point at
 * a displacement (dx, dy, dz) of row with |dx| <= 1, |dy| <= ry, |dz| <= rz (periodic wrap allowed in every direction,
 * x wraps inside an item).  2-D lattices are passed with ny = 1, batched problems as their block-diagonal form (nb items).
 * A workgroup of `threads` threads owns a ty × tz tile of the (y, z) plane and marches along x through `nseg` segments
 * per item, keeping four halo planes of the gathered dense operand in LDS (filled by 16-byte LDS-DMA one plane ahead):
 * every gather is an LDS read and the dense operand crosses L2 → CU (ty+2ry)(tz+2rz)/(ty·tz) times instead of once per
 * stored entry.  Up to 160 KiB of LDS per workgroup (tsgu_lattice_lds_bytes tells how much a configuration needs).
 *
 * The plan is built once per sparsity pattern by the caller (index ops; torchsparsegradutils_amd/_lattice.py):
 *   rcls  [rows]            uint8   class of each row: rows with the same displacement sequence share a class
 *   lens  [ncls]            uint8   stored entries per row of the class (<= recw <= 32, recw a multiple of 4)
 *   rstart[rows+1]          int32   first value position of each row of the VALUE-OWNING pattern (A's crow as int32);
 *                                   not read when uniform_len > 0 (every row has uniform_len entries)
 *   rec   kind 0 (walk in stored order: SpMM with the values of the walked rows, SDDMM):
 *         [ring][ncls][recw] int32  entry k of a row of class c gathers the LDS row at rec[x_ring % ring][c][k] BYTES from
 *                                   the row's own position in the halo tile, where a halo plane is (ty+2ry)·(tz+2rz) rows of
 *                                   p·sizeof(value) bytes, z fastest, and ring slot s holds plane bytes [s·plane, (s+1)·plane):
 *                                   rec = ((x_ring+dx) % ring)·plane + (dy·(tz+2rz) + dz)·rowbytes   (x_ring = 1 for the first
 *                                   plane of a segment)
 *         kind 1 (transposed walk: Aᵀ·G reads entry k' of SOURCE row i = row + displacement):
 *         [ring][ncls][recw][2] int32  {the same for the dense rows, the same displacement in the value ring (rows of
 *                                   `slot` = recw·4 rounded to 16 bytes) + 4·k'};  when a dense row is a multiple of 128 bytes
 *                                   the value ring takes the pitch of the dense ring and the table is [ring][ncls][recw] int32:
 *                                   dense-row offset (a multiple of 128) + 4·k' in the low 7 bits
 *   padded entries (k >= lens[c]) hold 0x7ff00: reads that far beyond the row's own position are beyond the LDS allocation and
 *   return zero on gfx950, so padded entries contribute exactly 0 and no dense row is touched that the sparse row does not reference.
 * Sums run in ascending entry order of the walked pattern (the order of the plan-free kernels).  fp32, fp64 and bf16 values
 * for both kinds (bf16: fp32 accumulation; the SpMM / Aᵀ·G walks add entries in pairs (2k, 2k+1) with v_dot2_f32_bf16 — exact
 * products, one fp32 addition per pair — within one bf16 ulp of the exact result like the one-entry-at-a-time kernels, not
 * bit-identical to them); p·sizeof(value)/16 in {2, 4, 8, 16} (SpMM, fp32: also 1); 16-byte aligned dense rows.
 */
typedef struct tsgu_lattice_plan {
    int32_t kind;             /* 0: stored-order walk (SpMM / SDDMM); 1: transposed walk (Aᵀ·G) */
    int32_t nb, nx, ny, nz;   /* items, planes per item, lines per plane, points per line */
    int32_t ry, rz;           /* halo radii */
    int32_t ncls, recw;       /* row classes of the pattern (<= 255), record width */
    int32_t nloc;             /* classes per workgroup list */
    int32_t uniform_len;      /* > 0: every row of the value-owning pattern has this many entries */
    int32_t ty, tz;           /* tile the records were built for */
    int32_t nseg;             /* x segments per item */
    int32_t threads;          /* workgroup size: 256, 512 or 1024 */
    int32_t ring;             /* halo planes resident in LDS (4..8): 3 in use + ring-3 in flight ahead of the computation */
    int32_t chunks_per_lane;  /* 16-byte chunks of a dense row per lane: 1, or 2 (dense rows of >= 128 bytes, recw == 28): half the
                                 lanes per row, twice the rows per wave */
    const void* rec;
    const void* lens;
    const void* rcls;
    const void* rstart;
    const void* wlist;        /* [workgroups][nloc] uint8: the classes of each workgroup's rows (0xff = unused); workgroup
                                 ((item·nseg + seg)·tiles_y + tile_y)·tiles_z + tile_z keeps only their records in LDS */
} tsgu_lattice_plan;

/* Dynamic LDS bytes of a configuration (mode: 0 SpMM, 1 SDDMM, 2 transposed SpMM), or a negative tsgu_status when it
 * does not fit the kernels' limits (160 KiB of LDS, DMA pieces and row passes per thread). */
int tsgu_lattice_lds_bytes(int mode, int vtype, int64_t p, int ty, int tz, int ry, int rz, int nloc, int recw, int threads, int ring,
                           int chunks_per_lane);
/* C = A·B (plan kind 0, the pattern of A) or gradB = Aᵀ·G (plan kind 1, the transposed pattern; `val` is A's value array
 * in A's own order, `B` is G).  n_rows = nb·nx·ny·nz. */
int tsgu_csr_spmm_lattice(int vtype, const tsgu_lattice_plan* plan, int64_t n_rows, int64_t nnz, const void* val,
                          const void* B, int64_t ldb, void* C, int64_t ldc, int64_t p, int device, void* stream);
/* C = A·B (plan kind 0, fp32 or fp64; partial sums in the value type) with the Krylov loops' dot epilogue: dot_partial[w][c] = Σ over the rows of workgroup w of
 * C[row, c]·B[row, c] (the own row of B is the centre of the halo plane in LDS; deterministic).  dot_rows must be the number of
 * workgroups of the configuration, nb·nseg·⌈ny/ty⌉·⌈nz/tz⌉; one chunk per lane.  This entry also takes 16-byte dense rows
 * (p = 4: one lane per row) — replaces tsgu_csr_spmm(..., dot_w = B, ...) inside utils/linear_cg.py:322 + :64-65 on lattice
 * stencils, without reading a column index.  `skip` (optional, device memory): when *skip != 0 the launch does nothing — the
 * done word of a solver loop whose iterations are queued ahead of the host's polls.  `dot_w` (optional): a second operand W [rows][p] with
 * C's leading dimension — the partial sums are then of C[row, c]·W[row, c] (BiCGSTAB's <r0, A q>, reference utils/bicgstab.py:196-199). */
int tsgu_csr_spmm_lattice_dot(int vtype, const tsgu_lattice_plan* plan, int64_t n_rows, int64_t nnz, const void* val,
                              const void* B, int64_t ldb, void* C, int64_t ldc, int64_t p, void* dot_partial, int64_t dot_rows,
                              const int* skip, const void* dot_w, int device, void* stream);
/* out_vals[k] = alpha·<R[row k,:], Cm[col k,:]> in stored order (plan kind 0). */
int tsgu_csr_sddmm_lattice(int vtype, const tsgu_lattice_plan* plan, int64_t n_rows, int64_t nnz, const void* R, int64_t ldr,
                           const void* Cm, int64_t ldc, void* out_vals, double alpha, int64_t p, int device, void* stream);

/*
 * Plane-march kernels (csrc/march_impl.h): the plane sweep for BOX stencils — every stored entry couples a lattice point with a
 * neighbour at (dx, dy, dz), |dx|, |dy|, |dz| <= 1, and every row holds exactly the displacements of ONE set `mask` (the whole
 * 27-point box, the 7-point cross, the lower / upper triangular half of either …) that lead to an existing neighbour: all of
 * them on a periodic lattice, the ones that stay inside on a lattice truncated at its faces (what the reference's
 * PairwiseEncoder emits, encoders/pairwise_encoder.py:562-849), per dimension (`periodic`).  Same call sites as the lattice
 * kernels above.  The sums are taken source plane by source plane: the dense rows of a halo plane are read from LDS once per
 * in-plane displacement and serve the three output planes x-1, x, x+1 (accumulators in registers), so a row costs at most ntap
 * LDS row reads instead of 3·ntap, there are no record tables, and two halo planes are resident instead of four.
 *   mask         bit (dx+1)·ntap + tap: the displacement occurs in the pattern (tsgu_march_supported tells which sets have kernels)
 *   periodic     bit 0 / 1 / 2: the lattice wraps in x / y / z.  In a truncated dimension the halo rows beyond a face are zero
 *                in LDS and halo planes beyond an x face are skipped: no row touches a dense row it does not reference
 *   ident        the class whose rows store ALL displacements of `mask` in ascending (dx, dy, dz) — the CANONICAL order (interior rows)
 *   tap_dy/dz    the in-plane displacements in that order
 *   kidx         [ncls][32] uint8: stored position of canonical slot (dx+1)·ntap + tap in a row of the class, 0xff when the row
 *                has no such entry (a face of a truncated lattice; a displacement outside `mask`); byte 31: entries of the row
 *   rcls         [rows (+ padding)] uint8 class of each row (the lattice plan's)
 *   uniform_len  > 0: every row stores this many entries (periodic lattices) and row r starts at r·uniform_len; 0: rows start at
 *   rstart       [rows + 1] int32 (A's row pointer)
 * Values are staged in canonical order (16-byte LDS-DMA for waves of `ident` rows of a full box, 4-byte LDS-DMA gathers through
 * kidx for the others); gradA is written in A's stored order.  Sums run in canonical order: bit-identical to the plan-free
 * kernels for rows that store their entries in ascending (dx, dy, dz) — all rows of a truncated lattice with sorted columns —
 * equal to rounding for rows that wrap around a face.  The transposed product needs no transposed pattern and no second plan:
 * entry (i -> j) is read from canonical slot (dx+1)·ntap + tap(dy, dz) of source row i's staged values.
 * fp32; p in {16, 32, 64} per call (wider operands: column tiles of 64 by the caller, the SDDMM with `accumulate`).
 *
 * bf16 (csrc/linemarch_impl.h, "whole-line march"): the products of a PERIODIC 27-point box stencil (mask = all 27 bits, periodic = 7,
 * uniform_len = 27) at p = 16 whose tile is `ty` whole z-lines (tz = nz, nz in {8, 16, 32, 64}, threads = ty·nz·2 in {256, 512, 1024},
 * ny a multiple of ty).  The value rows are staged raw (stored order) and the stored position of a displacement is computed —
 * 9·rank_x + 3·rank_y + rank_z, the rank of the wrapped neighbour coordinate among the three of its dimension: rows with sorted
 * columns — instead of read from kidx / rcls: the CALLER guarantees that this arithmetic describes every row (the Python side checks
 * it against the plan's class tables once per pattern, _lattice.linemarch_ok).  fp32 accumulation, one rounding.
 */
typedef struct tsgu_march_plan {
    int32_t nb, nx, ny, nz;   /* items, planes per item, lines per plane, points per line (each of nx, ny, nz >= 3) */
    int32_t ry, rz;           /* halo radii: 1, 1 */
    int32_t ntap;             /* in-plane displacements: 9 */
    int32_t tap_dy[9], tap_dz[9];
    int32_t ncls, ident;      /* row classes (<= 64), the canonical one */
    int32_t ty, tz;           /* tile */
    int32_t nseg;             /* x segments per item */
    int32_t threads;          /* workgroup size: 256 or 512 */
    uint32_t mask;            /* displacement set (27 bits) */
    int32_t periodic;         /* bit 0: x, bit 1: y, bit 2: z;  bit 3 (fp32, all three periodic, the whole box, uniform_len = 27): the caller has
                                 checked that every row stores (dx, dy, dz) at 9·rank_x + 3·rank_y + rank_z (sorted columns) — SpMM / SpMMT then
                                 stage value rows raw (plain 16-byte copies in every wave) and resolve the (y, z) order where values are read */
    int32_t uniform_len;      /* entries per row when all rows have the same number, else 0 */
    const void* kidx;
    const void* rcls;
    const void* rstart;       /* read when uniform_len == 0 */
} tsgu_march_plan;

/* 1 when there is a plane-march kernel for (mode: 0 SpMM, 1 SDDMM, 2 transposed SpMM; displacement set `mask`; rows of one length
 * or not; workgroup size): the whole box — all three products, 256 / 512 threads; the triangular halves of the box and of the
 * 7-point cross (by displacement, with / without the centre) on truncated lattices — the SDDMM, 256 threads.  Everything else
 * is faster on the general plane sweep (tsgu_csr_*_lattice) and has no plane-march kernel. */
int tsgu_march_supported(int mode, int mask, int uniform_len, int threads);
/* Dynamic LDS bytes of a configuration (mode: 0 SpMM, 1 SDDMM, 2 transposed SpMM) or a negative tsgu_status. */
int tsgu_march_lds_bytes(int mode, int vtype, int64_t p, int ty, int tz, int ry, int rz, int ncls, int threads);
/* C = A·B (transposed == 0) or gradB = Aᵀ·G (transposed != 0; `val` is A's value array in A's own order, `B` is G). */
int tsgu_csr_spmm_march(int vtype, const tsgu_march_plan* plan, int transposed, int64_t n_rows, int64_t nnz, const void* val,
                        const void* B, int64_t ldb, void* C, int64_t ldc, int64_t p, int device, void* stream);
/* out_vals[k] = alpha·<R[row k,:], Cm[col k,:]> in A's stored order (accumulate != 0: added to out_vals — the later column
 * tiles of operands wider than 64 columns).  bf16 (whole-line march, above): accumulate == 0. */
int tsgu_csr_sddmm_march(int vtype, const tsgu_march_plan* plan, int64_t n_rows, int64_t nnz, const void* R, int64_t ldr,
                         const void* Cm, int64_t ldc, void* out_vals, double alpha, int accumulate, int64_t p, int device,
                         void* stream);

/*
 * Row analysis for lattice plans (plan building, once per sparsity pattern; no reference counterpart — the reference
 * re-derives structure per call, sparse_matmul.py:186-192,229).  One thread per row; nothing is sorted.
 *   tsgu_lattice_rows       displacement code ((dx+1)·5 + dy+2)·5 + dz+2 of every entry of every row (nd == 0), or — nd > 0 —
 *                           of every entry of every row of the TRANSPOSED pattern without building it: the entries (i, j) of
 *                           transposed row j are found by searching the rows i = j − d for every displacement d of `disp[nd]`
 *                           (the codes that occur in the pattern), ordered by i, element = code(j→i)·32 + position of j in row i.
 *                           Pass 1 (ctable == NULL): the 64-bit hash of the row's sequence goes into an open-addressing table
 *                             (thash[tsgu_lattice_slots()] pre-set to 0x8000000000000000, trep[...] pre-set to INT_MAX: smallest
 *                             row of the slot); slot[row] (uint16) names the row's slot.  Rows with equal hashes are class candidates.
 *                           Pass 2 (ctable [ncls][32] int32, -1 beyond the class length; remap[slots] uint8; lens[ncls] uint8):
 *                             rcls[row] = remap[slot[row]] and every row is compared with its class exactly.
 *   tsgu_lattice_row_codes  sequences of `nrows` given rows (the class representatives) -> out [nrows][32] int32.
 *   tsgu_lattice_block_classes  mask[block][4] (uint64, zeroed by the caller): the set of classes among the rows of each
 *                           workgroup of a launch configuration (the lists a tsgu_lattice_plan carries in `wlist`).
 * status (device int32[8], zeroed by the caller): [0] rows that are not lattice rows (or differ from their class, or store a
 * column twice, or more than tsgu_lattice_slots() distinct rows), [1] max |dy|, [2] max |dz|, [3] longest row, [4] (pass 2 of the
 * stored-order walk with box_mask != 0) non-zero when some row is NOT "the displacements of box_mask — 27 bits, bit
 * (dx+1)·9 + (dy+1)·3 + dz+1 — whose neighbour exists", existence per dimension by `periodic` (bit 0 / 1 / 2: x / y / z wrap;
 * a truncated dimension has no neighbours beyond its faces): the condition of the plane-march kernels (tsgu_march_plan).
 * Rows longer than 32 entries are not-lattice.
 */
int tsgu_lattice_slots(void);
int tsgu_lattice_rows(int itype, int64_t n_rows, const void* crow, const void* col, int nb, int nx, int ny, int nz, const void* disp, int nd,
                      void* slot, void* thash, void* trep, const void* remap, const void* ctable, const void* lens, void* rcls, void* status,
                      int box_mask, int periodic, int device, void* stream);
int tsgu_lattice_row_codes(int itype, int64_t n_rows, const void* crow, const void* col, int nb, int nx, int ny, int nz, const void* disp,
                           int nd, const void* rows, int nrows, void* out, int device, void* stream);
int tsgu_lattice_block_classes(int64_t n_rows, const void* rcls, int nb, int nx, int ny, int nz, int ty, int tz, int nseg, void* mask,
                               int device, void* stream);

/*
 * K4  X = op(A)^{-1} B   sparse triangular solve, sync-free (dependency-driven) CSR sweep.
 * replaces: torch.triangular_solve(B, A, upper, transpose, unitriangular).solution
 *           torchsparsegradutils/_compat.py:42-48  (from sparse_solve.py:181-183 and :202-204)
 *
 * The kernel walks a row-gather structure (ptr, idx, [perm], val) of the matrix M whose rows
 * are solved in dependency order:  transpose == 0 → M = A (its CSR arrays, perm = NULL);
 * transpose != 0 → the caller passes the cached transposed pattern of A (CSC arrays of A viewed
 * as CSR of Aᵀ) with `perm` mapping into A's values, and `lower` already flipped.
 * Entries on the wrong side of the diagonal are ignored; with unit != 0 stored diagonal entries
 * are ignored too (same as the reference's backend).  X must NOT alias B.  B(i, c) = B[i·ldb + c·b_col_stride]
 * (b_col_stride = 1: row-major; transposed views are read in place), X is row-major.
 * fp32, fp64 and bf16 (bf16 elements, fp32 arithmetic, x rounded once when it is published).
 * `work` : device scratch, tsgu_sptrsm_work_bytes() bytes, contents irrelevant on entry.
 * `workgroups_per_cu` : persistent workgroups (4 waves each) per compute unit, 1 … 8 (0 = 1).  Speed only — every row sums its own
 *          entries in a fixed order, the solution does not depend on it: deep dependency chains want few polling waves (1), shallow
 *          wide patterns want many rows in flight (8).  (ABI 5: new argument.)
 */
int tsgu_csr_sptrsm(int vtype, int itype,
                    int64_t n, int64_t nnz,
                    const void* ptr, const void* idx, const void* perm, const void* val,
                    int lower, int unit,
                    const void* B, int64_t ldb, int64_t b_col_stride, void* X, int64_t ldx, int64_t p,
                    void* work, int workgroups_per_cu, int device, void* stream);
int64_t tsgu_sptrsm_work_bytes(int64_t n, int64_t p);

/*
 * K4 on stencil factors: the same solve as a line sweep over a row-major lattice (csrc/sptrsm_lattice.hip).
 * replaces: torch.triangular_solve(B, A, upper, transpose, unitriangular).solution
 *           torchsparsegradutils/_compat.py:42-48  (from sparse_solve.py:181-183 and :202-204)
 *
 * For a matrix M (A, or Aᵀ walked through A's own arrays) whose rows are the points of a lattice,
 * row = ((item·nx + x)·ny + y)·nz + z, and whose used entries (strictly below the diagonal for lower != 0, above otherwise) all
 * point to a row of the same z-line or of a line (item, x, y) that comes EARLIER in the sweep (lexicographically smaller for a lower
 * sweep, larger for an upper one) without wrapping around a lattice face.  One wave owns one z-line and solves its rows in z order;
 * lines are handed out by one ticket counter in sweep order; dependencies between lines use the hand-off of tsgu_csr_sptrsm (X
 * pre-filled with a NaN tag, one agent-scope store per element, bounded polls, the error word of `work`).  Every row sums its stored
 * entries in the order and lane geometry of tsgu_csr_sptrsm: the solution is the same bits.  The index arrays are not read.
 *
 * The plan structure tsgu_trsm_lattice_plan lives on the host, its pointers are device pointers:
 *   kind        0: M = A in stored order; 1: M = Aᵀ (values in the source rows of A's value array)
 *   nlines, nz  z-lines (items·nx·ny) and rows per line; n = nlines·nz
 *   ncls, width row classes (<= 255) and records per class (<= 32)
 *   uniform_len > 0: row r of A starts at r·uniform_len in `val`; 0: at rstart[r]
 *   front_lines lines a dependency front crosses (sizes the persistent grid when `workgroups` is 0; speed only)
 *   tab         [ncls][width] records of two int32 in VISITING order (kind 0: stored order; kind 1: ascending source row):
 *               word 0 = neighbour row − own row; word 1 = value position (kind 0: position in the own row; kind 1: position in
 *               the source row) | 1<<8 used by a lower sweep | 1<<9 used by an upper sweep | 1<<10 diagonal | 1<<11 same line
 *   lens        [ncls] uint8 stored entries per class;  rcls [n] uint8 class of every row;  rstart [n] int32 (uniform_len == 0)
 * fp32 and fp64, p <= 64 (TSGU_ERR_TOO_LARGE beyond: the caller keeps tsgu_csr_sptrsm).  B(i, c) = B[i·ldb + c·b_col_stride], X row-major,
 * X must not alias B.  `work`: tsgu_sptrsm_work_bytes() bytes.  `workgroups`: persistent 4-wave workgroups, 0 = chosen from
 * front_lines (capped at 8 per compute unit and at the number of lines); the solution does not depend on it.
 */
typedef struct {
    int32_t kind, nlines, nz, ncls, width, uniform_len, front_lines, reserved;
    const void* tab;
    const void* lens;
    const void* rcls;
    const void* rstart;
} tsgu_trsm_lattice_plan;
int tsgu_csr_sptrsm_lattice(int vtype, const tsgu_trsm_lattice_plan* plan, int64_t nnz, const void* val,
                            int lower, int unit,
                            const void* B, int64_t ldb, int64_t b_col_stride, void* X, int64_t ldx, int64_t p,
                            void* work, int workgroups, int device, void* stream);

/*
 * K5  fused CG vector updates (no preconditioner), all per-column scalars stay on the device.
 * replaces the ≈15-op chain  torchsparsegradutils/utils/linear_cg.py:64-95 (+ :27-47, :372-382)
 *
 * state layout (value type T = f32 or f64), all [p] unless noted:
 *   scal + 0*p : rr        (residual_inner_prod, rᵀr of the current residual)
 *   scal + 1*p : alpha
 *   scal + 2*p : beta
 *   scal + 3*p : rnorm     (‖r‖₂ per column, masked to 0 where rhs_is_zero)
 *   flags (int32): [0] done (tolerance reached), [1] iterations executed, [2..2+p) has_converged,
 *                  [2+p..2+2p) rhs_is_zero
 *
 * step 1  tsgu_cg_alpha:   alpha = safe(rr / Σ_blocks pAp_partial), 0 for converged columns
 * step 2  tsgu_cg_update1: r -= alpha·Ap ; x += alpha·p ; partial rr_new per block
 * step 3  tsgu_cg_beta:    rr_new = Σ partial ; beta = safe(rr_new / rr) ; rr = rr_new ;
 *                          rnorm = sqrt(rr_new) (masked) ; has_converged ; done flag
 * step 4  tsgu_cg_update2: pvec = r + beta·pvec
 * Every step is a no-op once flags[0] != 0, so a host may enqueue iterations ahead and poll.
 */
/* `fold` (optional): scratch of tsgu_cg_fold_rows() * p elements; when given and n_partial is large the
 * partial rows are first folded (deterministically) to that many rows by a wide launch. */
int64_t tsgu_cg_fold_rows(void);
int tsgu_cg_alpha(int vtype, const void* pap_partial, int64_t n_partial, void* fold, void* scal, int* flags,
                  double eps, int64_t p, int device, void* stream);
int tsgu_cg_update1(int vtype, int64_t n, int64_t p,
                    void* r, const void* Ap, void* x, const void* pvec,
                    const void* scal, const int* flags, void* rr_partial,
                    int device, void* stream);
/* steps 1 + 2 in ONE launch for n_partial <= 1024 partial rows (what K1 on the plane sweep leaves) and p <= 256: every
 * workgroup sums the partial rows itself, in row order — all workgroups hold the same alpha, bit for bit the alpha of
 * tsgu_cg_alpha.  Same operands as the two calls it replaces; returns TSGU_ERR_TOO_LARGE beyond the limits. */
int tsgu_cg_update1_alpha(int vtype, int64_t n, int64_t p, void* r, const void* Ap, void* x, const void* pvec, const void* pap_partial,
                          int64_t n_partial, void* scal, const int* flags, double eps, void* rr_partial, int device, void* stream);
/* The two-launch form of an iteration after K1 (same recurrences, reference utils/linear_cg.py:27-95, :319-382; for
 * n_partial <= 1024 partial rows of p'Ap and p <= 256, no preconditioner).  The single-workgroup step 3 disappears: every
 * workgroup of the direction update sums the |r|^2 partial rows itself.  For that the values an iteration READS live in half
 * `parity` (= iteration index & 1) of the state and the values it PRODUCES go to half `parity ^ 1`:
 *   scal2  [5][p]: rr half 0 | rr half 1 | alpha | beta | rnorm
 *   flags2 (int32): [0],[1] done by half, [2] iterations executed, [3] unused, [4..4+p) has_converged half 0, [4+p..4+2p) half 1,
 *                   [4+2p..4+3p) rhs_is_zero
 * tsgu_cg2_residual:  alpha = safe(rr / sum pAp_partial) (0 for converged columns) ; r -= alpha*Ap ; |r|^2 partials
 *                     (tsgu_cg2_num_blocks() rows, <= 1024)
 * tsgu_cg2_direction: beta = safe(rr_new / rr) ; x += alpha*p ; p = r + beta*p ; rr, rnorm, has_converged, the stop rule and the
 *                     iteration counter into half parity ^ 1
 * `hist` (optional, [n_hist][2][p] values): alpha and beta of the first n_hist iterations, what the Lanczos tridiagonal matrices
 * of linear_cg(n_tridiag > 0) are built from (reference :385-406).
 * The caller starts with rr, has_converged in half 0, parity 0, and alternates; both are no-ops once done[parity] != 0 (the
 * flag is carried to the other half), so a host may enqueue iterations ahead and poll flags2[0] | flags2[1]. */
int64_t tsgu_cg2_num_blocks(int vtype, int64_t n, int64_t p);
int tsgu_cg2_residual(int vtype, int64_t n, int64_t p, void* r, const void* Ap, const void* pap_partial, int64_t n_partial, void* scal2,
                      const int* flags2, int parity, double eps, void* rr_partial, int device, void* stream);
int tsgu_cg2_direction(int vtype, int64_t n, int64_t p, const void* r, void* pvec, void* x, const void* rr_partial, int64_t n_partial,
                       void* scal2, int* flags2, int parity, double eps, double stop_updating_after, double tolerance,
                       int min_iter_index, void* hist, int n_hist, int device, void* stream);
/* rows of rr_partial written by tsgu_cg_update1; r/Ap/x/pvec must be contiguous [n][p], 16-byte aligned */
int64_t tsgu_cg_num_blocks(int vtype, int64_t n, int64_t p);
int tsgu_cg_beta(int vtype, const void* rr_partial, int64_t n_partial, void* scal, int* flags,
                 double eps, double stop_updating_after, double tolerance, int iter_index,
                 int min_iter_index, int64_t p, int device, void* stream);
/* Preconditioned CG (reference utils/linear_cg.py:80-84, :319-382 with `preconditioner`): scal + 0*p holds <r, z>, z = M r
 * applied by the caller after step 2; step 3 takes the <r, z> partials next to the |r|^2 partials (beta and the next alpha
 * from <r, z>, residual norm / has_converged / stop test from |r|^2), step 4 is tsgu_cg_update2 with z in the place of r. */
int tsgu_cg_beta_precond(int vtype, const void* rr_partial, int64_t n_partial, const void* rz_partial, int64_t n_rz, void* scal,
                         int* flags, double eps, double stop_updating_after, double tolerance, int iter_index,
                         int min_iter_index, int64_t p, int device, void* stream);
int tsgu_cg_update2(int vtype, int64_t n, int64_t p, const void* r, void* pvec,
                    const void* scal, const int* flags, int device, void* stream);

/*
 * K6  fused BiCGSTAB recurrences (no preconditioner), all right-hand sides in lock-step, scalars on the device.
 * replaces the per-column Python loop and its ~12 ATen ops + 2 host reads per iteration
 *           torchsparsegradutils/utils/bicgstab.py:113-124, 163-241
 * scal  [8][p]: rho | alpha | omega | rho_next | threshold | beta | resid | resid0
 * flags int32 : [0] all columns finished, [1] iterations, [2..2+p) finished, [2+p..2+2p) finishing after the half
 *               step, [2+2p..2+3p) matvecs used.
 * tsgu_bicg_scalar(phase): 0 init (partial = <r0,r0>) | 1 beta | 2 alpha (partial = <r0,v>) | 3 half (|s|^2)
 *                          | 4 omega (partial = 3 sets <t,s>,<t,t>,<r0,t>, `set_stride` apart) | 5 end (|r|^2)
 * tsgu_bicg_vector(which): 0 p=(p*beta-(beta*omega)*v)+r (a0=p,a1=r,a2=v) | 1 s=r-alpha*v (a0=s,a1=r,a2=v)
 *                          | 2 three dot partials (a0=t,a1=s,a2=r0) | 3 x/r update (a0=x,a1=r,a2=s,a3=t,a4=p)
 * Vector operands are contiguous [n][p], 16-byte aligned; partial buffers have tsgu_cg_num_blocks() rows per set.
 * Every step is a no-op once flags[0] != 0.
 * Widths as for K7 below.  The library's own driver (utils/bicgstab.py) calls these entries with at most 256 columns: wider
 * right-hand sides are solved 256 columns at a time, since the columns are independent problems and a column's sums (hence its
 * iterates, in their last bits) depend on the width of the array it sits in.  The instances above 256 columns are kept for
 * callers of the C ABI and are covered by the step tests only.
 */
int tsgu_bicg_scalar(int vtype, int phase, const void* partial, int64_t n_partial, int64_t set_stride, void* fold,
                     void* scal, int* flags, double abstol, double reltol, int matvec_max, int nmv0, int64_t p,
                     int device, void* stream);
int tsgu_bicg_vector(int vtype, int which, int64_t n, int64_t p, void* a0, void* a1, const void* a2, const void* a3,
                     const void* a4, const void* scal, const int* flags, void* partial, int64_t set_stride,
                     int device, void* stream);
/* The x / r update of a right-preconditioned iteration (settings.precon, reference utils/bicgstab.py:191-194, 216-219,
 * 227-233): r = s - omega·t; x = (x + omega·z) + alpha·q with q = M p, z = M s applied by the caller between the steps
 * (v = A q, t = A z); columns finishing after the half step take x += alpha·q; |r|^2 partials.  Replaces
 * tsgu_bicg_vector(which = 3) in the step sequence above; everything else is unchanged. */
int tsgu_bicg_update_x_precond(int vtype, int64_t n, int64_t p, void* x, void* r, const void* s, const void* t,
                               const void* q, const void* z, const void* scal, const int* flags, void* partial,
                               int device, void* stream);

/*
 * K7: fused MINRES recurrences (one shift, no preconditioner; the general form follows), all right-hand sides at once — replaces the per-iteration
 * ATen op chain of reference utils/minres.py:259-296 (Lanczos step, Givens QR, solution update) and its
 * every-10-iterations stopping test (:299-305).  One iteration = tsgu_csr_spmm(+ <z, A z> partials) ->
 * tsgu_minres_scalar(0: alpha) -> tsgu_minres_vector(0: z_c = (A z - alpha z) - beta z_prev2 over z_prev2, |z_c|^2
 * partials) -> tsgu_minres_scalar(1: beta_c and the rotations) -> tsgu_minres_vector(1: z_c /= beta_c, w_c over w_prev2,
 * sol += w_c·scale, optionally |update|^2 and |sol|^2 partials) [-> tsgu_minres_scalar(2: stop test into flags[0])].
 * scal: [12][p] values — 0 alpha | 1 beta | 2,3 c,s two steps back | 4,5 c,s one step back | 6 scale | 7 sub | 8 subsub |
 * 9 diag | 10 scale of this update | 11 beta of the previous step; flags: int32 [0] stop, [1] iterations.  The caller
 * initialises rows 1, 6, 11 with the initial beta and rows 2, 4 with ones.  Arrays are contiguous [n][p], 16-byte
 * aligned; partial sets are `set_stride` elements apart with tsgu_cg_num_blocks(vtype, n, p) rows each; `fold`
 * (tsgu_cg_fold_rows() x p) is scratch for long partial lists.  fp32 / fp64.  Widths (the same for the K5 and K6 vector
 * steps): any p <= 256; above that p must be a multiple of the 16-byte lane width (4 fp32 / 2 fp64 columns) and at most 256
 * lanes wide, i.e. p <= 1024 in fp32 and p <= 512 in fp64.  Other widths return TSGU_ERR_TOO_LARGE and
 * tsgu_cg_num_blocks() returns -1 for them.
 */
int tsgu_minres_scalar(int vtype, int phase, const void* partial, int64_t n_partial, int64_t set_stride, void* fold,
                       void* scal, int* flags, double eps, double tol, double shift, int64_t p, int device, void* stream);
int tsgu_minres_vector(int vtype, int which, int64_t n, int64_t p, void* a0, const void* a1, void* a2, const void* a3,
                       void* a4, const void* scal, const int* flags, void* partial, int64_t set_stride, int with_norms,
                       int device, void* stream);
/* The same steps for (value·A + shift_s·I) x_s = b with several shifts at once and, optionally, a preconditioner
 * (reference utils/minres.py:140-311: `shifts`, `value`, `preconditioner`).  The Lanczos vectors and alpha / beta are
 * shared by the shifts; rotations, w vectors and solutions are per shift: scal is [n_shift][12][p] (rows 0, 1, 11 of
 * block 0 serve every shift; the caller initialises rows 2, 4, 6 of every block), w_prev2 / w_prev / sol are n_shift
 * planes [n][p], `shift_stride` elements apart (>= n·p, a multiple of 16 bytes), the stopping test reads 2·n_shift partial sets
 * (|update_s|^2 at set 2s, |sol_s|^2 at 2s+1) and averages over shifts and columns.  `shifts`: n_shift device values of
 * the value type.  scalar(0) stores alpha = value·<q, A q>, vector(0) forms z_c = (value·(A q) − alpha z) − beta z_prev2
 * from the unscaled product.  Preconditioned: the caller computes q_c = M z_c after vector(0), passes <z_c, q_c>
 * partials to scalar(1) (instead of |z_c|^2), and vector(1) gets a1 = q_prev and qc = q_c (normalised in place next
 * to z_c); without a preconditioner a1 = z_prev and qc = NULL. */
int tsgu_minres_scalar_ms(int vtype, int phase, const void* partial, int64_t n_partial, int64_t set_stride, void* fold,
                          void* scal, int* flags, double eps, double tol, const void* shifts, int n_shift, double value,
                          int64_t p, int device, void* stream);
int tsgu_minres_vector_ms(int vtype, int which, int64_t n, int64_t p, void* a0, const void* a1, void* a2, const void* a3,
                          void* a4, void* qc, const void* scal, const int* flags, void* partial, int64_t set_stride,
                          int with_norms, int n_shift, int64_t shift_stride, double value, int device, void* stream);

/* Column-wise dot products  out[c] = Σ_i X[i,c]·Y[i,c]  (two-stage, deterministic).
 * replaces: torch.dot / mul+sum in utils/bicgstab.py:168,199,222-224 and linear_cg.py:294 */
/* `partial` needs tsgu_coldot_max_blocks(n, p) * p elements. */
int64_t tsgu_coldot_max_blocks(int64_t n, int64_t p);
int tsgu_coldot(int vtype, int64_t n, int64_t p, const void* X, int64_t ldx,
                const void* Y, int64_t ldy, void* partial, void* out,
                int device, void* stream);

/*
 * Segmented log-sum-exp (sparse_logsumexp / sparse_bidir_logsumexp).
 * replaces: the scatter amax / exp / scatter sum / log of  torchsparsegradutils/sparse_logsumexp.py:10-73 (_scatter_logsumexp),
 *           its callers per axis                             sparse_logsumexp.py:105-138 (_logsumexp_2d),
 *           per batch item                                   sparse_logsumexp.py:141-172 (_logsumexp_batched),
 *           both axes into one padded buffer                 sparse_logsumexp.py:175-243 (_bidir_2d / _bidir_batched)
 *
 * out[group g] = log( sum_{k in [ptr[g], ptr[g+1])} exp(val[perm ? perm[k] : k])  +  zeros_g ),
 * zeros_g = axis_len - (ptr[g+1] - ptr[g]) when include_zeros (every stored entry counts, duplicates too), else 0.
 * NaN in a group -> NaN; +inf -> +inf; no values and no zeros -> -inf.  bf16 values accumulate in fp32 (one rounding at the end).
 * The row direction of a CSR pattern is (crow, no perm); the column direction its cached transpose (tptr, perm into A's values);
 * a whole matrix / batch item is one group (ptr = item boundaries, axis_len = rows * cols).
 * Output: group g is written at out[(g / groups_per_item) * item_stride + g % groups_per_item]; positions
 * [groups_per_item, item_stride) of every item are set to -inf (the padded buffer of the bidirectional call, no separate fill).
 * Balanced by entries, not by groups; deterministic (no float atomics: partials of groups that span several entry ranges are
 * merged in a fixed order).  `workspace` (16-byte aligned) holds tsgu_segment_logsumexp_workspace(vtype, nnz) bytes.
 */
int tsgu_segment_logsumexp_workspace(int vtype, int64_t nnz, int64_t* bytes_host);
int tsgu_segment_logsumexp(int vtype, int itype, int64_t n_groups, int64_t nnz, const void* ptr, const void* perm,
                           const void* val, int include_zeros, int64_t axis_len, void* out, int64_t groups_per_item,
                           int64_t item_stride, void* workspace, int64_t workspace_bytes, int device, void* stream);
/*
 * Gradient of the stored values, in their stored order (the backward of sparse_logsumexp.py:10-73 through autograd):
 *   grad[k] = g_grp[grp(k)] * exp(val[k] - lse_grp[grp(k)])  +  g_idx[idx[k]] * exp(val[k] - lse_idx[idx[k]])
 * grp(k): the group of [ptr[g], ptr[g+1]) holding k (found from ptr inside the kernel; n_groups = len(ptr) - 1);
 * either direction may be absent (ptr = NULL / idx = NULL).  One streaming pass, no atomics.
 */
int tsgu_segment_logsumexp_backward(int vtype, int itype, int64_t nnz, const void* val, const void* ptr, int64_t n_groups,
                                    const void* g_grp, const void* lse_grp, const void* idx, const void* g_idx,
                                    const void* lse_idx, void* grad, int device, void* stream);

/*
 * Segmented and gathered dense products (segment_mm / gather_mm and their gradients).
 * replaces: the tensor_split / nested-tensor matmul / cat of     torchsparsegradutils/indexed_matmul.py:95-105 (segment_mm),
 *           the R boolean masks / nested matmul / scatter of     indexed_matmul.py:203-217 (gather_mm),
 *           and the nested-tensor backward autograd takes through both.
 *
 * Rows are grouped by a plan of n_seg + 3 words each (built with device ops, indexed_matmul.py):
 *   offsets:  0 = offsets[0] <= offsets[1] <= ... <= offsets[n_seg + 1] <= offsets[n_seg + 2] = n.  Rows (positions in
 *             perm order) [offsets[r + 1], offsets[r + 2]) use b[r]; rows before offsets[1] and from offsets[n_seg + 1] on
 *             had an index outside [0, n_seg) and are written as zeros.
 *   tile_ptr: tile_ptr[e] = sum over e' < e of ceil((offsets[e' + 1] - offsets[e']) / tsgu_segment_mm_tile_rows()).
 * perm (itype, may be NULL = identity) maps a position to its row of a and out.  One workgroup per row tile: the launch takes
 * max_tiles >= ceil(n / BM) + min(n_seg, n) + 2 workgroups (a bound of tile_ptr[n_seg + 2]; no read-back), surplus ones exit.
 *
 * Forward (and grad_a, with b given as a transposed view):  out[perm[i]][:] = a[perm[i]][:] @ b[r]   (i in segment r)
 *   a: (n, d1), row stride lda;  b[r][k][j] at b + r*b_stride0 + k*b_stride1 + j*b_stride2, b_stride1 or b_stride2 == 1;
 *   out: (n, d2), row stride ldo.  MFMA (f32 16x16x4, f64 16x16x4, bf16 16x16x32 with fp32 accumulation and one rounding).
 *   f32 / f64 results are the k-ordered fma chain a[i][0]*b[0][j] + ... over k = 0 .. d1 - 1.
 */
int tsgu_segment_mm_tile_rows(void);
int tsgu_segment_mm(int vtype, int itype, int64_t n, int64_t d1, int64_t d2, int64_t n_seg, const void* offsets,
                    const void* tile_ptr, int64_t max_tiles, const void* perm, const void* a, int64_t lda, const void* b,
                    int64_t b_stride0, int64_t b_stride1, int64_t b_stride2, void* out, int64_t ldo, int device, void* stream);
/*
 * grad_b[r] = sum over the rows i of segment r of a[perm[i]]ᵀ g[perm[i]]   (the b-gradient of both products, replacing the
 * nested-tensor backward of indexed_matmul.py:95-105 / :203-217).  grad_b: (n_seg, d1, d2) contiguous, in b's dtype.
 * Split-K: each segment's rows are cut into chunks of chunk_rows (a function of the shapes only); one workgroup per
 * (chunk, 64 x 64 output tile) sums its rows in order.  A segment of one chunk is written directly; longer ones leave fp32
 * (fp64 for fp64) partials that a second kernel sums in chunk order; empty segments get zeros.  No atomics: bit-identical
 * from call to call.  chunk_ptr[n_seg + 1] is the chunk prefix of the real segments (sum of ceil(len_r / chunk_rows)) and
 * part_ptr[n_seg + 1] the prefix of the partial slots (chunk counts of segments with two or more chunks).
 * tsgu_segment_mm_grad_b_workspace gives chunk_rows, the launch bound max_chunks and the workspace bytes (16-byte aligned).
 */
int tsgu_segment_mm_grad_b_workspace(int vtype, int64_t n, int64_t n_seg, int64_t d1, int64_t d2, int64_t* chunk_rows,
                                     int64_t* max_chunks, int64_t* bytes);
int tsgu_segment_mm_grad_b(int vtype, int itype, int64_t n, int64_t d1, int64_t d2, int64_t n_seg, const void* offsets,
                           const void* chunk_ptr, const void* part_ptr, int64_t chunk_rows, int64_t max_chunks, const void* perm,
                           const void* a, int64_t lda, const void* g, int64_t ldg, void* grad_b, void* workspace,
                           int64_t workspace_bytes, int device, void* stream);

/*
 * Density of the sparse multivariate normal (SparseMultivariateNormal / SparseMultivariateNormalNative: log_prob, entropy,
 * variance) without densifying the factor.
 * replaces: L.to_dense(), its diagonal().log().sum() and the (z**2).sum(-1) behind a dense solve_triangular
 *                                           torchsparsegradutils/distributions/sparse_multivariate_normal.py:576-589 (log_prob),
 *           L.to_dense() and (L_dense**2).sum(-1)                      sparse_multivariate_normal.py:531-545 (variance),
 *           and the dense backward autograd takes through both.
 *
 * Value types fp32 and fp64 (fp32 sums in fp32, fp64 in fp64; bf16 is refused with TSGU_ERR_BAD_DTYPE).  Every sum over rows is
 * two-stage in a fixed order: one workgroup per chunk of rows of a batch item leaves one partial per output, a second kernel adds
 * an output's partials in order.  No float atomics, no host synchronisation: the same operands give the same bits, and every
 * launch can be captured.  `partial` holds (number of outputs) * tsgu_mvn_reduce_blocks(rows_per_item) accumulator elements
 * (4 bytes for fp32, 8 for fp64); `partial_elems` is its size in elements.  A batched operand is its block-diagonal 2-D pattern:
 * n_rows = items * rows_per_item.
 */
int64_t tsgu_mvn_reduce_blocks(int64_t rows_per_item);
/* Once per pattern: pos[i] = position in the owner's value array of the first entry of row i with col == i (through `perm`
 * when the pattern carries one, NULL = identity), -1 when the row stores no diagonal entry.  pos has the index type. */
int tsgu_csr_diag_positions(int itype, int64_t n_rows, int64_t nnz, const void* crow, const void* col, const void* perm,
                            void* pos, int device, void* stream);
/* out[item] = sum_i log(val[pos[i]]) over the item's rows; pos[i] < 0 counts as log 0 = -inf and a negative entry gives NaN, as
 * the dense formula does.  pos == NULL: val is a dense vector of n_rows elements and out[item] = sum_i log(val[i]) (the
 * log-determinant of the LDL^T forms: both share this reduction).  n_val = elements of val. */
int tsgu_diag_logsum(int vtype, int itype, int64_t n_rows, int64_t rows_per_item, int64_t n_val, const void* pos,
                     const void* val, void* out, void* partial, int64_t partial_elems, int device, void* stream);
/* Its gradient in the value array (nnz elements): g[item] / val[pos[i]] at the diagonal positions.  fill != 0: every entry of
 * every row is written, zero off the diagonal (the zero fill and the scatter are one pass over crow / perm; rows own disjoint
 * entries).  fill == 0: the diagonal entries of `grad` are updated in place on top of the gradient that is already there (the
 * solve's or the product's).  pos == NULL (dense vector, crow and perm unused): grad[i] = g[item] / val[i]. */
int tsgu_diag_logsum_backward(int vtype, int itype, int64_t n_rows, int64_t rows_per_item, int64_t nnz, const void* crow,
                              const void* perm, const void* pos, const void* val, const void* g, void* grad, int fill,
                              int device, void* stream);
/* The Mahalanobis term  out[item * k + c] = sum_i w_i^{+-1} (Y[i,c] + E[i,c])^2  over the item's rows.  Element (i, c) of Y at
 * Y[i * ldy + c * y_col_stride] (the solve's row-major result and the products' transposed views are both read in place), E
 * likewise with its own strides (NULL: absent; the implicit unit diagonal's share of L^T d + d).  w_mode: 0 no weight, 1 multiply
 * by w[i], 2 divide by w[i] (w: n contiguous elements). */
int tsgu_quadform(int vtype, int64_t n, int64_t k, const void* Y, int64_t ldy, int64_t y_col_stride, const void* E,
                  int64_t lde, int64_t e_col_stride, const void* w, int w_mode, int64_t rows_per_item, void* out,
                  void* partial, int64_t partial_elems, int device, void* stream);
/* One pass: grad_Y[i,c] = 2 g[item * k + c] w_i^{+-1} (Y + E)[i,c] (at grad_Y[i * ldg + c * g_col_stride]; also the gradient of
 * E) and, when grad_w is given, grad_w[i] = sum_c g[item * k + c] (Y + E)[i,c]^2 (multiply) or its negative over w_i^2 (divide). */
int tsgu_quadform_backward(int vtype, int64_t n, int64_t k, const void* Y, int64_t ldy, int64_t y_col_stride, const void* E,
                           int64_t lde, int64_t e_col_stride, const void* w, int w_mode, int64_t rows_per_item, const void* g,
                           void* grad_Y, int64_t ldg, int64_t g_col_stride, void* grad_w, int device, void* stream);
/* The variance of the covariance forms: out[i] = add[i] + sum over the entries k of row i of val[k]^2 * w[col[k]]  (w, add
 * optional; w has n_w elements).  Eight lanes per row, summed in a fixed order. */
int tsgu_csr_row_sumsq(int vtype, int itype, int64_t n_rows, int64_t nnz, int64_t n_w, const void* crow, const void* col,
                       const void* perm, const void* val, const void* w, const void* add, void* out, int device,
                       void* stream);
/* grad_val[k] = 2 g[row(k)] val[k] w[col[k]] in the value array's own order (every stored entry is written once). */
int tsgu_csr_row_sumsq_backward(int vtype, int itype, int64_t n_rows, int64_t nnz, int64_t n_w, const void* crow,
                                const void* col, const void* perm, const void* val, const void* w, const void* g, void* grad_val,
                                int device, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TSGU_HIP_H */
