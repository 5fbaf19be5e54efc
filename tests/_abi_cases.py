"""The shared C ABI test helper: the one parser of the headers under include/ with the parameter classes
(test_abi_conformance_cpu.py), the status codes, and the argument vectors of the refusal tests (test_abi_refusals_cpu.py,
test_gpu_abi_refusals.py).

Every launcher of include/tsgu_hip.h (an entry point whose last two parameters are `device, stream`) gets one BASE call that
passes all of its argument checks: 8 rows, 8 stored entries, the family's smallest width, plan structures that pass the
family's `fill`.  The parameter names come from the header itself, so a mutation is named by the parameter it changes.
"""

import ctypes
import os
import re

from torchsparsegradutils_amd import _backend

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")

OK, BAD_DTYPE, BAD_ARG, TOO_LARGE, LAUNCH, RUNTIME = 0, -1, -2, -3, -4, -5

_i32, _u32, _i64, _ptr = ctypes.c_int32, ctypes.c_uint32, ctypes.c_int64, ctypes.c_void_p


class TilePlan(ctypes.Structure):
    _fields_ = [(n, _i64) for n in ("n_rows", "n_cols", "nnz", "n_blocks")] + \
               [(n, _i32) for n in ("rows_per_block", "max_union", "max_entries", "reserved")] + \
               [(n, _ptr) for n in ("desc", "ucol", "lidx", "rptr", "cpos", "cslot", "ent", "xrow")]


class RowpackPlan(ctypes.Structure):
    _fields_ = [("nblocks", _i64)] + [(n, _i32) for n in ("ecap", "ucap", "nclasses", "rows_per_group")] + \
               [(n, _ptr) for n in ("uptr", "ucol", "upos", "sperm", "order", "vpair", "eptr", "wcls", "wbase", "cne", "srcstart")]


class LatticePlan(ctypes.Structure):
    _fields_ = [(n, _i32) for n in ("kind", "nb", "nx", "ny", "nz", "ry", "rz", "ncls", "recw", "nloc", "uniform_len", "ty", "tz",
                                    "nseg", "threads", "ring", "chunks_per_lane")] + \
               [(n, _ptr) for n in ("rec", "lens", "rcls", "rstart", "wlist")]


class MarchPlan(ctypes.Structure):
    _fields_ = [(n, _i32) for n in ("nb", "nx", "ny", "nz", "ry", "rz", "ntap")] + [("tap_dy", _i32 * 9), ("tap_dz", _i32 * 9)] + \
               [(n, _i32) for n in ("ncls", "ident", "ty", "tz", "nseg", "threads")] + [("mask", _u32), ("periodic", _i32),
                                                                                         ("uniform_len", _i32)] + \
               [(n, _ptr) for n in ("kidx", "rcls", "rstart")]


class TrsmLatticePlan(ctypes.Structure):
    _fields_ = [(n, _i32) for n in ("kind", "nlines", "nz", "ncls", "width", "uniform_len", "front_lines", "reserved")] + \
               [(n, _ptr) for n in ("tab", "lens", "rcls", "rstart")]


def _tile_limits():
    lib = _backend.load_library()
    r, u, e = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert lib.tsgu_tile_geometry(0, 32, ctypes.byref(r), ctypes.byref(u), ctypes.byref(e)) == 0
    return r.value, u.value, e.value


# plan type in the header -> (structure, integer fields of a plan that passes `fill`, pointer fields left NULL)
def _plans():
    rows, umax, emax = _tile_limits()
    taps = [(dy, dz) for dy in (-1, 0, 1) for dz in (-1, 0, 1)]
    return {
        "tsgu_tile_plan": (TilePlan, dict(n_rows=8, n_cols=8, nnz=8, n_blocks=1, rows_per_block=rows, max_union=umax, max_entries=emax),
                           ("cpos", "cslot")),
        "tsgu_rowpack_plan": (RowpackPlan, dict(nblocks=1, ecap=256, ucap=256, nclasses=0, rows_per_group=2),
                              ("upos", "sperm", "order", "vpair", "eptr", "wcls", "wbase", "cne", "srcstart")),
        "tsgu_lattice_plan": (LatticePlan, dict(kind=0, nb=1, nx=2, ny=2, nz=2, ry=1, rz=1, ncls=1, recw=8, nloc=1, uniform_len=1, ty=2,
                                                tz=2, nseg=1, threads=256, ring=4, chunks_per_lane=1), ()),
        "tsgu_march_plan": (MarchPlan, dict(nb=1, nx=3, ny=3, nz=3, ry=1, rz=1, ntap=9, tap_dy=[t[0] for t in taps],
                                            tap_dz=[t[1] for t in taps], ncls=1, ident=0, ty=3, tz=3, nseg=1, threads=256,
                                            mask=(1 << 27) - 1, periodic=7, uniform_len=27), ("rstart",)),
        "tsgu_trsm_lattice_plan": (TrsmLatticePlan, dict(kind=0, nlines=4, nz=2, ncls=1, width=4, uniform_len=1, front_lines=1), ()),
    }


# the march family walks 27 rows of 27 entries (a lattice side is at least 3); everything else 8 rows of 8 entries
_SIZES = {"n_rows": 8, "nnz": 8}
_FAMILY = {
    "tsgu_csr_spmm_march": dict(n_rows=27, nnz=729, p=16, ldb=16, ldc=16),
    "tsgu_csr_sddmm_march": dict(n_rows=27, nnz=729, p=16, ldr=16, ldc=16),
    "tsgu_csr_spmm_tile": dict(p=32, ldb=32, ldc=32),
    "tsgu_csr_sddmm_tile": dict(p=32, ldr=32, ldc=32),
    "tsgu_csr_spmm": dict(dot_w=None, dot_partial=None),
    "tsgu_csr_spmm_lattice_dot": dict(dot_rows=1, skip=None, dot_w=None),
    "tsgu_segment_mm": dict(b_stride0=64, b_stride1=8, b_stride2=1, max_tiles=64),
    "tsgu_segment_mm_grad_b": dict(chunk_rows=256, max_chunks=64),
    "tsgu_lattice_rows": dict(nb=1, nx=2, ny=2, nz=2, nd=0),
    "tsgu_lattice_row_codes": dict(nb=1, nx=2, ny=2, nz=2, nd=0, nrows=1),
    "tsgu_lattice_block_classes": dict(nb=1, nx=2, ny=2, nz=2, ty=2, tz=2, nseg=1),
    "tsgu_index_fingerprint": dict(accumulate=1),
    "tsgu_cg2_direction": dict(hist=None),
    "tsgu_csr_mm_backward_rowpack": dict(plan_pointers=("upos", "sperm")),      # the transposed walk carries a value permutation
}
_BY_NAME = dict(batch=1, b_col_stride=1, c_col_stride=1, y_col_stride=1, e_col_stride=1, g_col_stride=1, n_shift=1, w_mode=1,
                workgroups_per_cu=1, workgroups=1, workspace_bytes=4096, partial_elems=512, bytes=4096, set_stride=64, shift_stride=64,
                b_batch_stride=64, c_batch_stride=64, g_batch_stride=64, gb_batch_stride=64)


def prototypes(header):
    """The entries include/`header` declares, in declaration order: [(name, [(parameter name, type text), ...]), ...].  Comments
    are stripped first; a parameter list may span lines; `(void)` is an empty list."""
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(INCLUDE, header)).read(), flags=re.S)
    out = []
    for entry, params in re.findall(r"\b(?:int|int64_t|const char\s*\*|size_t)\s+(tsgu_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        pairs = []
        for raw in params.split(","):
            raw = " ".join(raw.split())
            if raw != "void":
                name = re.search(r"(\w+)$", raw).group(1)
                pairs.append((name, raw[: -len(name)].strip()))
        out.append((entry, pairs))
    return out


def klass_of_decl(type_text):
    """Class of a parameter of a prototype: pointer / 64-bit integer / double / int."""
    if "*" in type_text:
        return "ptr"
    if re.search(r"\bint64_t\b", type_text):
        return "i64"
    if re.search(r"\bdouble\b", type_text):
        return "dbl"
    if re.search(r"\b(int|tsgu_vtype|tsgu_itype)\b", type_text):
        return "int"
    raise AssertionError(f"unclassified parameter type {type_text!r}")


def klass_of_ctype(t):
    """Class of an entry of a ctypes `argtypes` list, in the words of `klass_of_decl`."""
    if t in (ctypes.c_void_p, ctypes.c_char_p) or hasattr(t, "_type_") and not isinstance(t._type_, str):
        return "ptr"
    return {ctypes.c_int64: "i64", ctypes.c_int: "int", ctypes.c_double: "dbl"}[t]


PARAMS = dict(prototypes("tsgu_hip.h"))
LAUNCHERS = sorted(n for n, ps in PARAMS.items() if len(ps) >= 2 and [q[0] for q in ps[-2:]] == ["device", "stream"])


class Call:
    """One entry point's BASE call.  `pointer(name, i)` supplies the address of pointer operand i (fake addresses that are never
    dereferenced for calls refused on the host, device buffers on a GPU)."""

    def __init__(self, name, pointer, device):
        self.name = name
        self.names = [p[0] for p in PARAMS[name]]
        self.types = [p[1] for p in PARAMS[name]]
        self.plan = None
        fam = _FAMILY.get(name, {})
        vals = []
        for i, (pn, pt) in enumerate(PARAMS[name]):
            if pn == "device":
                v = device
            elif pn == "stream":
                v = None
            elif pt.endswith("_plan*"):
                struct, ints, nulls = _plans()[pt.replace("const ", "").replace("*", "").strip()]
                self.plan = struct()
                for k, x in ints.items():
                    setattr(self.plan, k, (_i32 * 9)(*x) if isinstance(x, list) else x)
                for j, (fn, ft) in enumerate(struct._fields_):
                    if ft is _ptr and (fn not in nulls or fn in fam.get("plan_pointers", ())):
                        setattr(self.plan, fn, pointer(fn, 100 + j))
                v = ctypes.addressof(self.plan)
            elif pn in fam:
                v = fam[pn]
            elif pt.endswith("*"):
                v = pointer(pn, i)
            elif pt == "double":
                v = 1.0
            elif pt == "int64_t":
                v = _BY_NAME.get(pn, _SIZES.get(pn, 8))
            else:
                v = _BY_NAME.get(pn, 0)
            vals.append(v)
        self.args = vals

    def run(self, **changes):
        """Status of the call with the named parameters (or `plan_<field>` of the plan structure) replaced."""
        args = list(self.args)
        saved = {}
        for k, v in changes.items():
            if k.startswith("plan_"):
                saved[k[5:]] = getattr(self.plan, k[5:])
                setattr(self.plan, k[5:], v)
            else:
                args[self.names.index(k)] = v
        try:
            return getattr(_backend.load_library(), self.name)(*args)
        finally:
            for k, v in saved.items():
                setattr(self.plan, k, v)

    def mutations(self):
        """(label, changes) for every single-parameter change of the refusal grid, in a fixed order."""
        out = []
        for pn, pt in zip(self.names[:-2], self.types[:-2]):
            if pt.endswith("_plan*"):
                out.append((f"{pn}=NULL", {pn: None}))
                for fn, ft in type(self.plan)._fields_:
                    if ft is _ptr:
                        out.append((f"plan.{fn}=NULL", {"plan_" + fn: None}))
                    elif ft in (_i32, _u32, _i64):
                        for v in (0, -1, 3, 384, 1000) if ft is not _u32 else (0, 5):
                            if v == 0 and fn in ("ty", "tz"):
                                continue      # the stencil `fill`s divide by the tile before they look at it: a host fault, not a refusal
                            out.append((f"plan.{fn}={v}", {"plan_" + fn: v}))
            elif pt.endswith("*"):
                out.append((f"{pn}=NULL", {pn: None}))
                if self.args[self.names.index(pn)] is not None:
                    out.append((f"{pn}+4", {pn: self.args[self.names.index(pn)] + 4}))
            elif pt == "int64_t":
                for v in (-1, 0, 3, 12, 1 << 40):
                    out.append((f"{pn}={v}", {pn: v}))
            elif pt == "int":
                for v in (-1, 1, 2, 7):
                    out.append((f"{pn}={v}", {pn: v}))
        return out
