"""A numpy restatement of the sparse × sparse product in float64, for the tests of ``sparse_spgemm``.

Operands are (mask, dense values): the mask is the stored pattern, the values matter only where the mask is set (a stored
entry may be 0.0).  The product's pattern is the STRUCTURAL product of the masks, sorted; its values and both masked gradients are
dense float64 products sampled at the patterns; next to each, the sum of the absolute values of its terms ``Σ|a||b|``, which is
what the elementwise bound ``8·ε·Σ|terms|`` of the project's tests is taken of.
"""

import functools

import numpy as np

EPS = {"float32": 2.0 ** -24, "float64": 2.0 ** -53, "bfloat16": 2.0 ** -24}      # unit roundoff of the accumulator type
BF16_ULP = 2.0 ** -8           # one bf16 ulp of a value, relative (8 significand bits), as tests/test_gpu_round4.py words it


def bf16_round(x):
    """float64 values rounded to the nearest bfloat16 (ties to even): exactly representable in all three value dtypes."""
    u = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).astype(np.float64)


def csr_of(mask):
    """(crow, col) of a boolean matrix, columns ascending in every row."""
    mask = np.asarray(mask, dtype=bool)
    crow = np.concatenate(([0], np.cumsum(mask.sum(1)))).astype(np.int64)
    return crow, np.nonzero(mask)[1].astype(np.int64)


def pattern(a_mask, b_mask):
    """The structural product: the boolean matrix and its sorted (crow, col)."""
    S = (a_mask.astype(np.int64) @ b_mask.astype(np.int64)) > 0
    return (S,) + csr_of(S)


def product(A, a_mask, B, b_mask):
    """(S, C, Σ|terms|) as dense float64 arrays, meaningful where S is set."""
    S, _, _ = pattern(a_mask, b_mask)
    Am, Bm = np.where(a_mask, A, 0.0), np.where(b_mask, B, 0.0)
    return S, Am @ Bm, np.abs(Am) @ np.abs(Bm)


def gradients(A, a_mask, B, b_mask, G):
    """(gradA, Σ|terms|, gradB, Σ|terms|) for the dense upstream gradient G, which counts on the product's pattern only; the
    gradients are meaningful on the operands' masks."""
    S, _, _ = pattern(a_mask, b_mask)
    Am, Bm, Gm = np.where(a_mask, A, 0.0), np.where(b_mask, B, 0.0), np.where(S, G, 0.0)
    return Gm @ Bm.T, np.abs(Gm) @ np.abs(Bm).T, Am.T @ Gm, np.abs(Am).T @ np.abs(Gm)


# ---- the cases -----------------------------------------------------------------------------------------------------------------
def _values(shape, seed):
    return bf16_round(np.random.default_rng(seed).standard_normal(shape))


def random_small(seed=0):
    """37×29 · 29×41 at about 15 % density, with: empty rows of A (3, 20), rows of A that meet only empty rows of B (5, 11 → rows
    7, 8 of B), a row of C with a single entry (row 9), and the rest random."""
    rng = np.random.default_rng(seed)
    a = rng.random((37, 29)) < 0.15
    b = rng.random((29, 41)) < 0.15
    b[[7, 8]] = False
    a[[3, 20]] = False
    a[5] = False
    a[5, 7] = True
    a[11] = False
    a[11, [7, 8]] = True
    b[13] = False
    b[13, 30] = True
    a[9] = False
    a[9, 13] = True
    return a, b


def all_empty():
    """Operands with entries whose product has none: A only meets empty rows of B."""
    a = np.zeros((6, 5), dtype=bool)
    b = np.zeros((5, 7), dtype=bool)
    a[:, :2] = True
    b[2:, ::2] = True
    return a, b


def bound_one_long_row(L):
    """3-row A whose rows' upper bounds are L-1, L, L+1: row r meets one long row of B (L-3+r entries at random columns) and one
    row of two entries."""
    rng = np.random.default_rng(L)
    m = L + 9
    a = np.zeros((3, 4), dtype=bool)
    b = np.zeros((4, m), dtype=bool)
    b[3, [1, m - 2]] = True
    for r in range(3):
        b[r, rng.choice(m, L - 3 + r, replace=False)] = True
        a[r, [r, 3]] = True
    return a, b


def bound_overlapping_rows(L, rows=8):
    """The same three upper bounds from `rows` rows of B per row of A that cover nearly the same columns: ub ≫ distinct count."""
    a = np.zeros((3, 3 * rows), dtype=bool)
    width = (L + 1) // rows + 4
    b = np.zeros((3 * rows, width + 3), dtype=bool)
    for r in range(3):
        target = L - 1 + r
        for q in range(rows):
            length = target // rows + (1 if q < target % rows else 0)
            start = q % 3
            b[r * rows + q, start:start + length] = True
            a[r, r * rows + q] = True
    return a, b


def long_row(distinct=6000):
    """One row of C with more distinct columns than the largest LDS bin holds (even columns from one row of B, odd ones from
    another, a few again from a third), next to a short row."""
    a = np.zeros((2, 3), dtype=bool)
    b = np.zeros((3, distinct), dtype=bool)
    b[0, 0::2] = True
    b[1, 1::2] = True
    b[2, 5:distinct:997] = True
    a[0] = True
    a[1, 2] = True
    return a, b


def clustered(capacity=512):
    """Columns that are all multiples of `capacity`, plus capacity-1 consecutive ones, met by one row of A (what would chain in
    a hash table of that capacity; the kernels sort instead, this is one more pattern for them)."""
    m = capacity * 40
    a = np.zeros((2, 3), dtype=bool)
    b = np.zeros((3, m), dtype=bool)
    b[0, ::capacity] = True
    b[1, 7:7 + capacity - 1] = True
    b[2, :capacity:3] = True
    a[0, :2] = True
    a[1] = True
    return a, b


def stencil27(n=8):
    """The 27-point periodic stencil on n³ (its square has 125 entries per row)."""
    idx = np.arange(n ** 3)
    x, y, z = idx // (n * n), (idx // n) % n, idx % n
    a = np.zeros((n ** 3, n ** 3), dtype=bool)
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                a[idx, ((x + dx) % n) * n * n + ((y + dy) % n) * n + (z + dz) % n] = True
    return a, a.copy()


CASES = {
    "random_small": random_small,
    "all_empty": all_empty,
    "long_row": long_row,
    "clustered": clustered,
    "stencil27": stencil27,
}


@functools.lru_cache(maxsize=None)
def case(name, limit=None):
    """(a_mask, A, b_mask, B, G) of a named case — values rounded to bfloat16, so that one float64 reference serves every value
    dtype — and its reference, computed once: a dict with S, crow, col, C, C_terms, gA, gA_terms, gB, gB_terms.  The arrays are
    shared between tests: read only."""
    if name in ("bound_one_long_row", "bound_overlapping_rows"):
        a, b = globals()[name](limit)
    else:
        a, b = CASES[name]()
    seed = sum(map(ord, name)) + (limit or 0)
    A, B = _values(a.shape, seed), _values(b.shape, seed + 1)
    G = _values((a.shape[0], b.shape[1]), seed + 2)
    S, crow, col = pattern(a, b)
    _, C, Ct = product(A, a, B, b)
    gA, gAt, gB, gBt = gradients(A, a, B, b, G)
    ref = dict(S=S, crow=crow, col=col, C=C, C_terms=Ct, gA=gA, gA_terms=gAt, gB=gB, gB_terms=gBt)
    for arr in (a, A, b, B, G, *ref.values()):
        arr.setflags(write=False)
    return a, A, b, B, G, ref


def to_torch(mask, values, layout, dtype, index_dtype=None, device="cpu"):
    """The operand as a torch sparse tensor: `layout` "csr" (index_dtype int32 or int64) or "coo" (coalesced, int64)."""
    import torch

    crow, col = csr_of(mask)
    v = torch.tensor(values[mask]).to(dtype).to(device)
    if layout == "csr":
        idt = index_dtype or torch.int64
        return torch.sparse_csr_tensor(torch.from_numpy(crow).to(idt).to(device), torch.from_numpy(col).to(idt).to(device), v,
                                       mask.shape)
    idx = torch.from_numpy(np.stack((np.nonzero(mask)[0], col))).to(device)
    return torch.sparse_coo_tensor(idx, v, mask.shape, is_coalesced=True)


def arrays_of(T):
    """(crow, col, values) of a torch CSR or coalesced COO tensor as numpy arrays (values as float64)."""
    import torch

    T = T.detach()
    if T.layout == torch.sparse_csr:
        crow, col, val = T.crow_indices(), T.col_indices(), T.values()
    else:
        assert T.is_coalesced()
        idx = T._indices()
        crow, col, val = torch._convert_indices_from_coo_to_csr(idx[0].contiguous(), T.size(0)), idx[1], T._values()
    return crow.cpu().numpy().astype(np.int64), col.cpu().numpy().astype(np.int64), val.double().cpu().numpy()


def assert_on_pattern(T, crow, col, exact, terms, dtype_name, what):
    """The sparse tensor T has exactly the pattern (crow, col), and every stored value lies within 8·ε·Σ|terms| of `exact` (dense
    float64; bfloat16: plus one bf16 ulp of the exact value for the single rounding of the fp32-accumulated sum)."""
    got_crow, got_col, val = arrays_of(T)
    assert np.array_equal(got_crow, crow), (what, "crow")
    assert np.array_equal(got_col, col), (what, "col")
    rows = np.repeat(np.arange(len(crow) - 1), np.diff(crow))
    want, mag = exact[rows, col], terms[rows, col]
    bound = 8 * EPS[dtype_name] * mag
    if dtype_name == "bfloat16":
        bound = bound + BF16_ULP * np.abs(want)
    err = np.abs(val - want)
    worst = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print(f"{what} [{dtype_name}]: {err.size} entries, worst error / bound = {worst:.3g}")
    assert np.all(err <= bound), (what, dtype_name, worst)
