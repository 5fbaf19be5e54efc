"""Structural cases for the log-sum-exp kernels (csrc/logsumexp_impl.h) and a numpy model of which range owns which group.

The forward cuts the stored entries into ranges of R = kLseStageBytes / sizeof(Acc) entries, one wave each.  A wave reduces
the groups whose first entry lies in its range (one lane per group of <= kLseLaneMax entries in the range, the whole wave for
a longer one), leaves a tail partial for an owned group that runs past the range and a head partial when its first entry
belongs to a group that started earlier; the merge kernel combines a tail with the later heads.  The backward walks spans of
64 * kWide entries and searches each entry's group in an LDS window of kLseBwdWindow ptr entries, or in global memory when
more group starts fall inside the span.  The generator below places groups on exactly those branch points; `events` restates
the ownership rule (not the kernel's code) and reports which ones a case reaches.

Plain Python and numpy: the CPU tests pin the constants against the kernel sources and the coverage, the GPU tests run the
cases through the public API.
"""

import math

import numpy as np

# the kernel constants (parsed from the sources and compared by tests/test_lse_cases_cpu.py)
STAGE_BYTES = 8192                                   # kLseStageBytes
LANE_MAX = 48                                        # kLseLaneMax
BWD_WINDOW = 320                                     # kLseBwdWindow
WAVE = 64
ACC_BYTES = {"float32": 4, "float64": 8, "bfloat16": 4}   # accumulator of each value type (bf16 accumulates in fp32)
K_WIDE = {"float32": 4, "float64": 2, "bfloat16": 8}      # VT<V>::kWide: values per 16-byte access
DTYPES = ("float32", "float64", "bfloat16")


def range_len(dtype):
    """R: entries of one forward range (fp32 / bf16 2048, fp64 1024)."""
    return STAGE_BYTES // ACC_BYTES[dtype]


def span_len(dtype):
    """Entries of one backward wave: 64 * kWide (fp32 256, fp64 128, bf16 512)."""
    return WAVE * K_WIDE[dtype]


EVENTS = (
    "lane_48",               # an owned piece of exactly kLseLaneMax entries (lane path)
    "wide_49",               # an owned piece of kLseLaneMax + 1 entries (wave path)
    "many_wide_in_window",   # >= 16 wide groups among the 64 groups of one lane window
    "ends_on_range_end",     # a lane-path group that ends exactly on its range's end (not the last range)
    "wide_ends_on_range_end",
    "range_exact_group",     # a group of exactly R entries starting at a range start (no head, no tail)
    "double_range_group",    # a group of 2R entries starting at a range start
    "wide_owned",            # a wide group finished inside its range
    "lane_tail",             # a tail partial from the lane path
    "wide_tail",             # a tail partial from the wave path
    "head_only_range",       # a range entirely inside a group that started earlier
    "head_then_owned",       # a head partial and owned groups in the same range
    "lane_tail_3_ranges",    # a lane-path tail of a group that reaches >= 3 ranges
    "merge_gt_64",           # a group with more than 64 partials (the merge's lane-strided loop runs twice)
    "ga_is_n_groups",        # a range after the start of the last group (ga == n_groups)
    "empty_at_range_start",  # an empty group with ptr == s of a range w > 0
    "trailing_empty",        # empty groups at nnz (owned by the last range)
    "nnz_multiple_of_R",
    "nnz_multiple_of_R_plus_1",
    "nnz_zero",
    "bwd_window_full",       # a backward span whose window holds exactly kLseBwdWindow ptr entries (staged)
    "bwd_unstaged",          # a backward span with more: global-memory search
)


# ----------------------------------------------------------------------------------------------------------------------------
# coverage model


def forward_model(ptr, R):
    """Per range: (s, e, ga, gb, head_end or None, tail group or -1, [(g, lo, hi, ends_in_range)] of the owned groups)."""
    ptr = np.asarray(ptr, dtype=np.int64)
    n, nnz = ptr.size - 1, int(ptr[-1])
    n_ranges = max(1, -(-nnz // R))
    out = []
    for w in range(n_ranges):
        s = w * R
        e = min(s + R, nnz)
        last = w == n_ranges - 1
        ga = int(np.searchsorted(ptr, s, side="left"))
        gb = n if last else int(np.searchsorted(ptr, e, side="left"))
        head = None
        if s < nnz and (ga == n or ptr[ga] > s):
            head = min(int(ptr[ga]), e)
        owned, tail = [], -1
        for g in range(ga, gb):
            glo, ghi = int(ptr[g]), int(ptr[g + 1])
            owned.append((g, glo, min(ghi, e), ghi <= e))
            if ghi > e:
                tail = g
        out.append((s, e, ga, gb, head, tail, owned))
    return out


def pieces(ptr, R):
    """Range pieces of every group (an empty group counts one)."""
    ptr = np.asarray(ptr, dtype=np.int64)
    lo, hi = ptr[:-1], ptr[1:]
    return np.where(hi > lo, (hi - 1) // R - lo // R + 1, 1)


def backward_windows(ptr, span):
    """nw = r1 - r0 + 2 of every backward span (the ptr entries its window needs)."""
    ptr = np.asarray(ptr, dtype=np.int64)
    n, nnz = ptr.size - 1, int(ptr[-1])
    s = np.arange(0, nnz, span, dtype=np.int64)
    e = np.minimum(s + span, nnz)
    r0 = np.minimum(np.searchsorted(ptr, s + 1, side="left"), n) - 1
    r1 = np.minimum(np.searchsorted(ptr, e, side="left"), n) - 1
    return r1 - r0 + 2


def events(ptr, dtype):
    """The set of structural events (EVENTS) a CSR row pointer reaches in the kernels of value type `dtype`."""
    R, span = range_len(dtype), span_len(dtype)
    ptr = np.asarray(ptr, dtype=np.int64)
    n, nnz = ptr.size - 1, int(ptr[-1])
    ev = set()
    if nnz == 0 and n > 0:
        ev.add("nnz_zero")
    elif nnz % R == 0:
        ev.add("nnz_multiple_of_R")
    elif nnz % R == 1:
        ev.add("nnz_multiple_of_R_plus_1")
    model = forward_model(ptr, R)
    npc = pieces(ptr, R)
    for w, (s, e, ga, gb, head, tail, owned) in enumerate(model):
        if head is not None:
            if head >= e:
                ev.add("head_only_range")
            elif gb > ga:
                ev.add("head_then_owned")
        if s < nnz and ga == n:
            ev.add("ga_is_n_groups")
        for base in range(0, len(owned), WAVE):
            win = owned[base:base + WAVE]
            if sum(1 for _, lo, hi, _ in win if hi - lo > LANE_MAX) >= 16:
                ev.add("many_wide_in_window")
        for g, lo, hi, done in owned:
            ln = hi - lo
            wide = ln > LANE_MAX
            if ln == LANE_MAX:
                ev.add("lane_48")
            if ln == LANE_MAX + 1:
                ev.add("wide_49")
            if done and wide:
                ev.add("wide_owned")
            if done and ln > 0 and int(ptr[g + 1]) == e and e < nnz:
                ev.add("wide_ends_on_range_end" if wide else "ends_on_range_end")
            if lo == s and int(ptr[g + 1]) == e and e - s == R:
                ev.add("range_exact_group")
            if lo == s and int(ptr[g + 1]) == s + 2 * R:
                ev.add("double_range_group")
            if not done:
                ev.add("wide_tail" if wide else "lane_tail")
                if not wide and npc[g] >= 3:
                    ev.add("lane_tail_3_ranges")
                if npc[g] > WAVE:
                    ev.add("merge_gt_64")
            if ln == 0 and lo == s and w > 0:
                ev.add("empty_at_range_start")
            if ln == 0 and lo == nnz and nnz > 0 and g > 0:
                ev.add("trailing_empty")
    if nnz > 0:
        nw = backward_windows(ptr, span)
        if (nw == BWD_WINDOW).any():
            ev.add("bwd_window_full")
        if (nw > BWD_WINDOW).any():
            ev.add("bwd_unstaged")
    return ev


# ----------------------------------------------------------------------------------------------------------------------------
# generator


class _Ptr:
    """Appends groups to a CSR row pointer."""

    def __init__(self, rng):
        self.lens = []
        self.pos = 0
        self.rng = rng

    def add(self, n):
        self.lens.append(int(n))
        self.pos += int(n)
        return len(self.lens) - 1

    def empties(self, n):
        for _ in range(n):
            self.add(0)

    def pad_to(self, mod, target):
        """Short filler groups (1..8 entries) until pos ≡ target (mod `mod`)."""
        need = (target - self.pos) % mod
        while need > 8:
            k = int(self.rng.integers(1, 9))
            self.add(k)
            need -= k
        if need:
            self.add(need)

    def ptr(self):
        return np.concatenate([[0], np.cumsum(self.lens, dtype=np.int64)]).astype(np.int64)


def _main_ptr(dtype, rng):
    R, B = range_len(dtype), span_len(dtype)
    p = _Ptr(rng)
    p.add(R)                                     # exactly one range, from a range start
    p.add(2 * R)                                 # two ranges from a range start: tail, then a head-only range ending on e
    p.empties(3)                                 # empty groups at a range start
    for _ in range(6):
        p.add(LANE_MAX)
        p.add(LANE_MAX + 1)
    p.pad_to(R, 0)
    for i in range(40):                          # one 64-group window full of wide groups
        p.add(49 + i % 12)
    p.pad_to(R, 0)
    p.add(R - 1)
    p.add(R + 1)
    p.pad_to(R, R - 30)
    p.add(30)                                    # lane group ending on its range's end
    p.pad_to(R, R - 100)
    p.add(100)                                   # wide group ending on its range's end
    p.pad_to(R, R - 20)
    p.add(20 + 3 * R + 7)                        # lane tail, then 3 head partials (the last one mid-range)
    p.pad_to(R, R - 200)
    p.add(200 + R + 50)                          # wide tail, one head-only range, then a head with owned groups after it
    p.pad_to(B, 0)
    p.add(1)
    p.empties(BWD_WINDOW - 3)                    # a backward window of exactly kLseBwdWindow entries
    p.add(B - 1)
    p.pad_to(B, 5)
    p.empties(BWD_WINDOW + 80)                   # too many group starts for the window: global search
    p.add(B)
    p.pad_to(R, R - 10)
    p.add(130 * R + 33)                          # 131 range pieces: more than 64 partials in one merge
    p.pad_to(R, 17)
    p.add(3 * R - 17)                            # a long last group that ends on nnz = k·R (ga == n_groups after it)
    return p.ptr()


def _boundary_ptrs(dtype, rng):
    R = range_len(dtype)
    out = {}
    p = _Ptr(rng)
    p.add(R - 1)
    p.add(1)
    p.add(R + 1)
    p.pad_to(R, 0)
    p.add(R - 5)
    p.add(5)
    p.add(1)                                     # nnz = 3R + 1: a last range of one entry
    p.empties(4)
    out["nnz_kR_plus_1"] = p.ptr()
    p = _Ptr(rng)
    p.add(R // 2)
    p.add(R)
    p.add(R // 2)
    p.add(2 * R - 40)
    p.add(40)                                    # ends on nnz = 4R exactly
    p.empties(70)                                # trailing empty groups, more than one lane window of them
    out["nnz_kR_trailing"] = p.ptr()
    out["nnz_zero"] = np.zeros(9, dtype=np.int64)
    return out


NEEDLE_C = 8.0       # needle offset: e^8 keeps the needles above every group's absent-entry count


def needle_values(ptr, dtype, rng):
    """Baseline N(−40, 1) values, and needles j·ln2 + c_g (j = 0..3 cycling, c_g = NEEDLE_C + 0.1·(g mod 7)) at the first and
    last entry of every range piece of every group.  A lost, doubled or misassigned piece moves its group's sum of exponentials
    by at least one needle: see `needle_sensitivity`."""
    R = range_len(dtype)
    ptr = np.asarray(ptr, dtype=np.int64)
    nnz = int(ptr[-1])
    v = rng.normal(-40.0, 1.0, nnz)
    for g in range(ptr.size - 1):
        lo, hi = int(ptr[g]), int(ptr[g + 1])
        if hi == lo:
            continue
        cuts = sorted({lo, hi} | set(range((lo // R + 1) * R, hi, R)))
        pos = []
        for a, b in zip(cuts[:-1], cuts[1:]):
            pos += [a, b - 1]
        pos = sorted(set(pos))
        j = np.arange(len(pos)) % 4
        v[pos] = j * math.log(2.0) + NEEDLE_C + 0.1 * (g % 7)
    return v


def needle_sensitivity(ptr, vals, axis_len=None):
    """Per group: the least change ln(total / (total − smallest needle term)) of its exact log-sum-exp when one needle is lost
    (inf for groups without needles)."""
    ptr = np.asarray(ptr, dtype=np.int64)
    n = ptr.size - 1
    out = np.full(n, np.inf)
    for g in range(n):
        x = vals[ptr[g]:ptr[g + 1]]
        nd = x[x > 0]
        if nd.size == 0:
            continue
        total = np.exp(x).sum() + (axis_len - x.size if axis_len is not None else 0)
        out[g] = math.log(total / (total - np.exp(nd.min())))
    return out


def special_ptr_vals(dtype, rng):
    """Special values inside multi-range groups, all −inf groups, large magnitudes and very negative include_zeros groups."""
    R = range_len(dtype)
    big = 1e200 if dtype == "float64" else 1e4
    p = _Ptr(rng)
    marks = {}
    p.pad_to(R, R - 20)
    marks["nan_head"] = p.add(20 + 2 * R + 9)      # NaN in the head piece of its second range
    p.pad_to(R, R - 30)
    marks["inf_head"] = p.add(30 + 2 * R + 11)     # +inf in the head piece of its third range
    p.pad_to(R, R - 10)
    marks["ninf_piece"] = p.add(10 + 2 * R + 5)    # its whole second-range piece is −inf
    marks["ninf_lane"] = p.add(10)
    marks["ninf_wide"] = p.add(100)
    p.pad_to(R, R - 15)
    marks["ninf_multi"] = p.add(15 + R + 15)       # all −inf across two ranges (merged partials)
    marks["big_wide"] = p.add(300)
    marks["big_lane"] = p.add(12)
    p.pad_to(R, R - 40)
    marks["big_multi"] = p.add(40 + R + 40)
    marks["neg_lane"] = p.add(9)
    marks["neg_wide"] = p.add(200)
    p.pad_to(R, R - 25)
    marks["neg_multi"] = p.add(25 + R + 25)
    p.add(3)
    ptr = p.ptr()
    v = rng.standard_normal(int(ptr[-1])) * 2.0
    lo = lambda k: int(ptr[marks[k]])              # noqa: E731
    hi = lambda k: int(ptr[marks[k] + 1])          # noqa: E731
    r0 = lambda k: (lo(k) // R + 1) * R            # first range start inside the group  # noqa: E731
    v[r0("nan_head") + 3] = np.nan
    v[r0("inf_head") + R + 4] = np.inf
    v[r0("ninf_piece"):r0("ninf_piece") + R] = -np.inf
    for k in ("ninf_lane", "ninf_wide", "ninf_multi"):
        v[lo(k):hi(k)] = -np.inf
    for k in ("big_wide", "big_lane", "big_multi"):
        m = hi(k) - lo(k)
        v[lo(k):hi(k)] = big * rng.uniform(0.5, 1.0, m) * rng.choice([-1.0, 1.0], m)
    for k in ("neg_lane", "neg_wide", "neg_multi"):
        v[lo(k):hi(k)] = -big * rng.uniform(0.5, 1.0, hi(k) - lo(k))
    return ptr, v, marks


def structural_cases(dtype, seed=0):
    """[(name, ptr int64, float64 values)] for value type `dtype`: the structural patterns with needle values, the main pattern
    with randn·σ values (σ = 1, 3, 30), and the special-value pattern."""
    rng = np.random.default_rng(seed)
    main = _main_ptr(dtype, rng)
    cases = [("main_needles", main, needle_values(main, dtype, rng))]
    trailing = np.concatenate([main, np.full(100, main[-1])])
    cases.append(("main_trailing_needles", trailing, needle_values(trailing, dtype, rng)))
    for name, ptr in _boundary_ptrs(dtype, rng).items():
        cases.append((name + "_needles", ptr, needle_values(ptr, dtype, rng)))
    for sigma in (1.0, 3.0, 30.0):
        cases.append((f"main_randn{int(sigma)}", main, rng.standard_normal(int(main[-1])) * sigma))
    ptr, v, _ = special_ptr_vals(dtype, rng)
    cases.append(("specials", ptr, v))
    return cases


def axis_len_of(ptr):
    """The axis length of a case's matrix: its longest group plus a few absent entries."""
    return int(np.diff(np.asarray(ptr, dtype=np.int64)).max(initial=0)) + 7


def columns(ptr):
    """Distinct, sorted secondary indices 0..len−1 in every group (so that include_zeros counts every absent entry)."""
    ptr = np.asarray(ptr, dtype=np.int64)
    lens = np.diff(ptr)
    return np.arange(int(ptr[-1]), dtype=np.int64) - np.repeat(ptr[:-1], lens)
