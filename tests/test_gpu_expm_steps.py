"""`tsgu_cheb_step` and `tsgu_cheb_combine` (csrc/expm_impl.h), one launch at a time on random state, against the float64
restatement in tests/_expm_ref.py.

The bound is a count of roundings, not a measurement.  With eps the machine epsilon of the value type, every output element is
within R·eps·M of the float64 result on the same (rounded) inputs, M the sum of the absolute values of the terms the element is
computed from, and R read off the expressions of csrc/tsgu_hip_expm.h:

  step      t0 = gamma·prev (1), t1 = fma(beta, x, −t0) (1), t2 = fma(alpha, prod, t1) (1 when prod is given), new = t2 + src (1 when
            src is given): R = 2 + [prod] + [src].  alpha, beta and gamma are cast to the value type once; the test passes values
            that float32 holds exactly, so the cast adds nothing.
  emit      one product and m − 1 fmas, each on a partial sum of at most M: R = m, and one more for `planes + t` with accumulate.
  spread    one product and T − 1 fmas: R = T.

Each rounding is bounded by half an eps of a partial result that is at most M·(1 + R·eps): machine epsilon is twice the unit
roundoff, which leaves room for the second-order terms and for the float64 reference's own rounding (2^-29 of an eps in fp32;
in fp64 the reference rounds as often as the kernel, which the factor of two covers as well).

Shapes.  n in {1, 37, 1025}: none a multiple of the rows per workgroup, the last more than one workgroup for every width; p in
{1, 3, 4, 5, 64, 256} and 260 (fp32) / 258 (fp64) for the lanes past 256 columns (4, 64, 256, 260, 258 take the 16-byte lanes);
m in {1, 2, chunk cap}, T in {1, 2, time cap} and 3, 5 (no power of two: the kernel is compiled for 4 and 8); planes are padded where n·p is no multiple of the lane.  Not the cross product:
every value of each parameter appears, the widest at the smallest n that still leaves a partial workgroup.
"""

import numpy as np
import pytest
import torch

import _abi_cases as A
import _expm_ref as ER
from torchsparsegradutils_amd import _backend

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
NP = {torch.float32: np.float32, torch.float64: np.float64}
DTYPES = pytest.mark.parametrize("td", [torch.float32, torch.float64], ids=["f32", "f64"])


def _caps():
    g = _backend.expm_geometry(torch.float32, 8, 1)
    return g[0], g[1]


def _wide(td, p):
    return (260 if td == torch.float32 else 258) if p == "wide" else p


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _dev(a):
    return None if a is None else torch.from_numpy(a).to(DEV)


def _within(got, want, mag, roundings, td, label):
    eps = float(np.finfo(NP[td]).eps)
    err = np.abs(got.astype(np.float64) - want)
    bound = roundings * eps * mag
    worst = float((err / np.where(bound > 0, bound, 1.0)).max())
    print(f"[{label}] max |err| / bound = {worst:.3f} (R = {roundings})")
    assert np.all(err <= bound), f"{label}: off by {worst:.3f} of the bound"


# ---- tsgu_cheb_step ------------------------------------------------------------------------------------------------------------------

def _step_state(rng, td, n, p, m_chunk, m_src, prod, alias):
    t = NP[td]
    st = {"prod": rng.standard_normal((n, p)).astype(t) if prod else None, "x": rng.standard_normal((n, p)).astype(t),
          "prev": rng.standard_normal((n, p)).astype(t),
          "chunk": rng.standard_normal((n, m_chunk, p)).astype(t) if m_chunk else None,
          "src": None if (alias or not m_src) else rng.standard_normal((n, m_src, p)).astype(t)}
    return st


def _step_launch(st, alpha, beta, gamma, src_slot, slot, alias, stop=0):
    d = {k: _dev(v) for k, v in st.items()}
    flags = torch.tensor([stop, 0], dtype=torch.int32, device=DEV)
    src = d["chunk"] if alias else d["src"]
    _backend.cheb_step(d["prod"], d["x"], d["prev"], alpha, beta, gamma, flags, src=src, src_slot=src_slot, chunk=d["chunk"], slot=slot)
    torch.cuda.synchronize()
    for key in ("prod", "x", "src"):
        if st[key] is not None:
            assert np.array_equal(_bits(d[key].cpu().numpy()), _bits(st[key])), f"{key} is an input"
    assert flags.tolist() == [stop, 0]
    return d["prev"].cpu().numpy(), None if d["chunk"] is None else d["chunk"].cpu().numpy()


STEP_CASES = [  # (n, p, chunk slots or 0, src slots or 0, prod, (alpha, beta, gamma), src aliases chunk)
    (1, 1, 0, 0, True, (0.5, -0.25, 1.0), False),
    (1, 5, 2, 0, False, (0.0, 1.0, 0.0), False),                  # w_0 enters a chunk
    (37, 1, 1, 1, True, (2.0, -1.5, 1.0), True),                  # the backward's step: src and chunk are one slot
    (37, 3, 2, 2, True, (0.75, 0.5, 1.0), False),
    (37, 4, "cap", 0, True, (1.0, -1.0, 0.0), False),             # k = 0: gamma = 0, prev is not read
    (37, 5, 0, "cap", False, (0.0, 0.0, 0.0), False),             # the last adjoint vector
    (37, 64, 2, 2, True, (0.5, 0.25, 1.0), True),
    (37, 256, "cap", 1, True, (2.0, -0.5, 1.0), False),
    (37, "wide", 2, 0, True, (1.0, 1.0, 1.0), False),
    (37, "wide", 0, 2, False, (0.0, 1.0, 0.5), False),
    (1025, 1, 2, 0, True, (0.5, 0.5, 1.0), False),
    (1025, 3, 0, 0, True, (2.0, -1.0, 1.0), False),
    (1025, 4, 2, 2, True, (0.25, 1.0, 1.0), True),
    (1025, 5, 1, 2, False, (0.0, -1.0, 2.0), False),
    (1025, 64, 2, 0, True, (1.5, 0.5, 1.0), False),
    (1025, 256, 0, 1, True, (0.5, -0.75, 1.0), False),
    (1, 256, 2, 2, True, (1.0, 0.5, 1.0), False),
    (1, "wide", 1, 1, True, (2.0, -2.0, 1.0), True),
]


@DTYPES
@pytest.mark.parametrize("n,p,m_chunk,m_src,prod,abc,alias", STEP_CASES)
def test_step_against_float64(td, n, p, m_chunk, m_src, prod, abc, alias):
    p = _wide(td, p)
    cap = _caps()[1]
    m_chunk, m_src = (cap if v == "cap" else v for v in (m_chunk, m_src))
    assert n % _backend.expm_geometry(td, n, p)[3] != 0, "n must leave a partial workgroup"
    rng = np.random.default_rng(1000 * n + 10 * p + m_chunk + 3 * m_src)
    st = _step_state(rng, td, n, p, m_chunk, m_src, prod, alias)
    slot, src_slot = max(m_chunk - 1, 0), max(m_src - 1, 0)
    if alias:
        src_slot = slot
    got_prev, got_chunk = _step_launch(st, *abc, src_slot, slot, alias)
    src_np = st["chunk"] if alias else st["src"]
    want, want_chunk, mag = ER.step(st["prod"], st["x"], st["prev"], *abc, src_np if m_src else None, src_slot, st["chunk"], slot, 0)
    R = 2 + int(prod) + int(bool(m_src))
    _within(got_prev, want, mag, R, td, f"step {td} n {n} p {p} chunk {m_chunk} src {m_src}")
    if m_chunk:
        assert np.array_equal(_bits(got_chunk[:, slot]), _bits(got_prev)), "the slot holds the bits that went over prev"
        others = [s for s in range(m_chunk) if s != slot]
        assert np.array_equal(_bits(got_chunk[:, others]), _bits(st["chunk"][:, others])), "the other slots keep their bits"
    again = _step_launch(st, *abc, src_slot, slot, alias)
    assert np.array_equal(_bits(again[0]), _bits(got_prev)), "two launches must give the same bits"
    frozen = _step_launch(st, *abc, src_slot, slot, alias, stop=1)
    assert np.array_equal(_bits(frozen[0]), _bits(st["prev"])), "prev was written under a set stop word"
    if m_chunk:
        assert np.array_equal(_bits(frozen[1]), _bits(st["chunk"])), "chunk was written under a set stop word"


@DTYPES
def test_step_copies_exactly(td):
    """(alpha, beta, gamma) = (0, 1, 0) without prod: w_0 enters the ring and the chunk with its bits."""
    rng = np.random.default_rng(5)
    st = _step_state(rng, td, 37, 5, 3, 0, False, False)
    prev, chunk = _step_launch(st, 0.0, 1.0, 0.0, 0, 1, False)
    assert np.array_equal(_bits(prev), _bits(st["x"])) and np.array_equal(_bits(chunk[:, 1]), _bits(st["x"]))


# ---- tsgu_cheb_combine ---------------------------------------------------------------------------------------------------------------

def _combine_launch(td, mode, accumulate, chunk, coef, planes, stop=0):
    T, n, p = planes.shape
    align = _backend.expm_geometry(td, n, p)[2]
    stride = -(-n * p // align) * align + align                       # always padded: the padding is never touched
    buf = torch.full((T, stride), 7.0, dtype=td, device=DEV)
    buf[:, : n * p] = _dev(planes).reshape(T, n * p)
    d_chunk, d_coef = _dev(chunk), _dev(coef)
    flags = torch.tensor([stop, 0], dtype=torch.int32, device=DEV)
    _backend.cheb_combine(mode, d_chunk, d_coef, buf, stride, flags, accumulate=accumulate)
    torch.cuda.synchronize()
    assert torch.equal(buf[:, n * p:], torch.full((T, stride - n * p), 7.0, dtype=td, device=DEV)), "the padding was written"
    assert np.array_equal(_bits(d_coef.cpu().numpy()), _bits(coef)) and flags.tolist() == [stop, 0]
    out_planes = buf[:, : n * p].reshape(T, n, p).cpu().numpy()
    out_chunk = d_chunk.cpu().numpy()
    if mode == 0:
        assert np.array_equal(_bits(out_chunk), _bits(chunk)), "chunk is an input of the emit"
        return out_planes
    assert np.array_equal(_bits(out_planes), _bits(planes)), "planes are an input of the spread"
    return out_chunk


COMBINE_CASES = [  # (n, p, m, T)
    (1, 1, 1, 1), (1, 5, 2, 2), (37, 1, "cap", 2), (37, 3, 2, "cap"), (37, 4, 1, 2), (37, 5, "cap", "cap"), (37, 64, 2, 1),
    (37, 256, 2, "cap"), (37, "wide", 2, 2), (37, "wide", 1, "cap"), (1025, 1, 2, "cap"), (1025, 3, 1, 1), (1025, 4, 2, 2),
    (1025, 5, 2, 3), (1025, 64, 2, 2), (1025, 256, 1, 2), (1, 256, "cap", 1), (1, "wide", 2, 5),
]


@DTYPES
@pytest.mark.parametrize("n,p,m,T", COMBINE_CASES)
def test_combine_against_float64(td, n, p, m, T):
    p = _wide(td, p)
    tcap, ccap = _caps()
    m, T = (ccap if m == "cap" else m), (tcap if T == "cap" else T)
    assert n % _backend.expm_geometry(td, n, p)[3] != 0, "n must leave a partial workgroup"
    rng = np.random.default_rng(100 * n + 7 * p + m + 13 * T)
    t = NP[td]
    chunk = rng.standard_normal((n, m, p)).astype(t)
    coef = rng.standard_normal((m, T, p)).astype(t)
    planes = rng.standard_normal((T, n, p)).astype(t)
    label = f"{td} n {n} p {p} m {m} T {T}"
    for accumulate in (False, True):
        got = _combine_launch(td, 0, accumulate, chunk, coef, planes)
        want, mag = ER.combine(0, accumulate, chunk, coef, planes, 0)
        _within(got, want, mag, m + int(accumulate), td, f"emit{' +=' if accumulate else ''} {label}")
        assert np.array_equal(_bits(_combine_launch(td, 0, accumulate, chunk, coef, planes)), _bits(got)), "two launches, the same bits"
    got = _combine_launch(td, 1, False, chunk, coef, planes)
    want, mag = ER.combine(1, False, chunk, coef, planes, 0)
    _within(got, want, mag, T, td, f"spread {label}")
    assert np.array_equal(_bits(_combine_launch(td, 1, False, chunk, coef, planes)), _bits(got)), "two launches, the same bits"
    assert np.array_equal(_bits(_combine_launch(td, 0, True, chunk, coef, planes, stop=1)), _bits(planes)), "written under a stop word"
    assert np.array_equal(_bits(_combine_launch(td, 1, False, chunk, coef, planes, stop=1)), _bits(chunk)), "written under a stop word"


def test_a_unit_coefficient_returns_the_bits():
    """c_0 = 1 and one slot: the emit returns the slot's bits (negative zeros included) — what t = 0 relies on."""
    x = np.random.default_rng(2).standard_normal((37, 1, 5)).astype(np.float32)
    x[3, 0, 2] = -0.0
    got = _combine_launch(torch.float32, 0, False, x, np.ones((1, 1, 5), dtype=np.float32), np.zeros((1, 37, 5), dtype=np.float32))
    assert np.array_equal(_bits(got[0]), _bits(x[:, 0]))


# ---- refusals --------------------------------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing():
    """Each refusal csrc/tsgu_hip_expm.h names returns its code; the buffers of a refused launch keep their bits."""
    lib = _backend.load_library()
    tcap, ccap = _caps()
    n, p, m, T = 37, 8, 3, 2
    g = torch.Generator(device="cpu").manual_seed(3)
    dev = {k: torch.randn(s, generator=g).to(DEV) for k, s in
           dict(prod=(n, p), x=(n, p), prev=(n, p), src=(n, m, p), chunk=(n, m, p), coef=(m, T, p), planes=(T, n * p)).items()}
    dev["flags"] = torch.zeros(2, dtype=torch.int32, device=DEV)
    snapshot = {k: v.clone() for k, v in dev.items()}
    stream = torch.cuda.current_stream(DEV).cuda_stream
    ptr = {k: v.data_ptr() for k, v in dev.items()}

    def step(**ch):
        a = dict(vtype=0, n=n, p=p, prod=ptr["prod"], x=ptr["x"], prev=ptr["prev"], alpha=0.5, beta=0.5, gamma=1.0, src=ptr["src"],
                 src_slots=m, src_slot=1, chunk=ptr["chunk"], chunk_slots=m, slot=2, flags=ptr["flags"])
        a.update(ch)
        return lib.tsgu_cheb_step(*a.values(), 0, stream)

    def combine(**ch):
        a = dict(vtype=0, mode=0, accumulate=0, n=n, p=p, m=m, T=T, chunk=ptr["chunk"], coef=ptr["coef"], planes=ptr["planes"],
                 plane_stride=n * p, flags=ptr["flags"])
        a.update(ch)
        return lib.tsgu_cheb_combine(*a.values(), 0, stream)

    for key in ("x", "prev", "flags"):
        assert step(**{key: None}) == A.BAD_ARG, key
    assert step(prod=None) == A.BAD_ARG, "a NULL prod needs alpha == 0"
    for key in ("prod", "x", "prev", "src", "chunk"):
        assert step(**{key: ptr[key] + 4}) == A.BAD_ARG, f"{key}: 16-byte alignment"
    assert step(flags=ptr["flags"] + 2) == A.BAD_ARG
    for ch in (dict(n=0), dict(p=0), dict(src_slots=0), dict(chunk_slots=0), dict(src_slot=-1), dict(src_slot=m), dict(slot=-1),
               dict(slot=m)):
        assert step(**ch) == A.BAD_ARG, ch
    assert step(vtype=2) == A.BAD_DTYPE and step(vtype=9) == A.BAD_DTYPE
    assert step(chunk_slots=ccap + 1) == A.TOO_LARGE and step(src_slots=ccap + 1) == A.TOO_LARGE
    assert step(n=1, p=257) == A.TOO_LARGE
    for key in ("chunk", "coef", "planes", "flags"):
        assert combine(**{key: None}) == A.BAD_ARG, key
    for key in ("chunk", "planes"):
        assert combine(**{key: ptr[key] + 4}) == A.BAD_ARG, f"{key}: 16-byte alignment"
    assert combine(coef=ptr["coef"] + 2) == A.BAD_ARG and combine(flags=ptr["flags"] + 2) == A.BAD_ARG
    for ch in (dict(n=0), dict(p=0), dict(m=0), dict(T=0), dict(mode=2), dict(mode=-1), dict(accumulate=2), dict(mode=1, accumulate=1),
               dict(plane_stride=n * p - 4), dict(plane_stride=n * p + 2)):
        assert combine(**ch) == A.BAD_ARG, ch
    assert combine(vtype=2) == A.BAD_DTYPE and combine(vtype=9) == A.BAD_DTYPE
    assert combine(m=ccap + 1) == A.TOO_LARGE and combine(T=tcap + 1) == A.TOO_LARGE
    assert combine(n=1, p=257, plane_stride=260) == A.TOO_LARGE
    torch.cuda.synchronize()
    for k, v in snapshot.items():
        assert torch.equal(dev[k], v), f"{k} changed under a refused launch"
