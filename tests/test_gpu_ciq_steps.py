"""`tsgu_ciq_update` and `tsgu_ciq_stop` (csrc/ciq_impl.h), one launch at a time on random state, against the float64 restatement
in tests/_ciq_ref.py.

The bound is a count of roundings, not a measurement.  With eps the machine epsilon of the value type, every output element is
within (S + 6)·eps·M of the float64 result on the same (rounded) inputs, M the sum of the absolute values of the terms the element
is computed from: w_c takes five roundings (two products, two differences, a quotient), the update a sixth, each fma of the weighted
sum one more on a partial sum that is at most the sum of the terms (S of them), the final `acc +=` one; `keep` takes seven and z one.
The float64 reference's own rounding is 2^-29 (fp32) or 1 (fp64) of an eps and has its place in the count's slack: machine epsilon
is twice the unit roundoff each rounding is really bounded by.

Shapes.  n in {1, 37, 1025}: none a multiple of the rows per workgroup, the last more than one workgroup for every width; p in
{1, 3, 4, 5, 64, 256} and 260 (fp32) / 258 (fp64) for the lanes past 256 columns (4, 64, 256, 260, 258 take the 16-byte lanes);
S in {1, 2, 12, cap}; planes are padded where n·p is no multiple of the lane.  The full cross product is not run: every n, every
p and every S appears with and without `keep`, the widest cases at the smallest n that still leaves a partial workgroup.
"""

import numpy as np
import pytest
import torch

import _abi_cases as A
import _ciq_ref as CR
from torchsparsegradutils_amd import _backend

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
NP = {torch.float32: np.float32, torch.float64: np.float64}


def _cap():
    return _backend.ciq_geometry(torch.float32, 8, 1)[0]


def _state(rng, td, n, p, S, keep, done_cols=(), stop=0):
    """Random state as numpy arrays of the value type (what the kernel reads), scal with diag away from zero."""
    t = NP[td]
    st = {
        "zc": rng.standard_normal((n, p)).astype(t), "zp": rng.standard_normal((n, p)).astype(t),
        "wpp": rng.standard_normal((S, n, p)).astype(t), "wp": rng.standard_normal((S, n, p)).astype(t),
        "acc": rng.standard_normal((n, p)).astype(t),
        "keep": rng.standard_normal((n, S, p)).astype(t) if keep else None,
        "scal": rng.standard_normal((S, 12, p)).astype(t),
        "omega": rng.uniform(0.1, 2.0, S).astype(t),
        "done": np.zeros(p, dtype=np.int32), "flags": np.array([stop, 0], dtype=np.int32),
    }
    st["scal"][0, 1] = rng.uniform(0.5, 2.0, p)                        # beta_c
    st["scal"][:, 9] = rng.uniform(0.5, 3.0, (S, p)) * rng.choice([-1.0, 1.0], (S, p))      # diag
    st["done"][list(done_cols)] = 1
    return st


def _launch(st, td):
    """One tsgu_ciq_update on device copies of `st` (planes padded to the lane); returns the outputs as float64 numpy arrays."""
    S, n, p = st["wpp"].shape
    align = _backend.ciq_geometry(td, n, p)[1]
    plane = -(-n * p // align) * align
    dev = {k: (None if v is None else torch.from_numpy(v).to(DEV)) for k, v in st.items()}
    w = []
    for key in ("wpp", "wp"):
        buf = torch.full((S, plane), 7.0, dtype=td, device=DEV)           # the padding is never touched: checked below
        buf[:, : n * p] = dev[key].reshape(S, n * p)
        w.append(buf)
    _backend.ciq_update(dev["zc"], dev["zp"], w[0], w[1], plane, dev["acc"], dev["keep"], dev["scal"], dev["omega"], dev["done"],
                        dev["flags"])
    torch.cuda.synchronize()
    assert torch.equal(w[0][:, n * p:], torch.full((S, plane - n * p), 7.0, dtype=td, device=DEV)), "the padding was written"
    for key in ("zp", "scal", "omega", "done", "flags"):
        assert np.array_equal(dev[key].cpu().numpy(), st[key], equal_nan=True), f"{key} is an input"
    assert np.array_equal(w[1][:, : n * p].reshape(S, n, p).cpu().numpy(), st["wp"])
    return {"z": dev["zc"].cpu().numpy(), "w": w[0][:, : n * p].reshape(S, n, p).cpu().numpy(), "acc": dev["acc"].cpu().numpy(),
            "keep": None if dev["keep"] is None else dev["keep"].cpu().numpy()}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _check(st, got, td, label):
    S = st["omega"].size
    want, mag = CR.update_step(st["zc"], st["zp"], st["wpp"], st["wp"], st["acc"], st["keep"], st["scal"], st["omega"], st["done"],
                               int(st["flags"][0]))
    eps = float(np.finfo(NP[td]).eps)
    before = {"z": st["zc"], "w": st["wpp"], "acc": st["acc"], "keep": st["keep"]}
    worst = 0.0
    for key in ("z", "w", "acc", "keep"):
        if want[key] is None:
            assert got[key] is None
            continue
        bound = (S + 6) * eps * mag[key]
        err = np.abs(got[key].astype(np.float64) - want[key])
        untouched = mag[key] == 0
        assert np.array_equal(_bits(got[key])[untouched], _bits(before[key])[untouched]), f"{label}: {key} must keep its bits there"
        live = ~untouched
        if live.any():
            worst = max(worst, float((err[live] / bound[live]).max()))
        assert np.all(err <= bound), f"{label}: {key} off by {float((err[live] / bound[live]).max()):.3f} of the bound"
    print(f"[ciq update] {label}: max |err| / bound = {worst:.3f}")


CASES = [  # (n, p, S, keep)
    (1, 1, 1, False), (1, 5, 2, True), (37, 1, 12, True), (37, 3, 12, False), (37, 4, 2, True), (37, 5, "cap", True),
    (37, 64, 12, True), (37, 256, 12, False), (37, 256, "cap", True), (37, "wide", 12, True), (37, "wide", 1, False),
    (1025, 1, 2, False), (1025, 3, 12, True), (1025, 4, 12, False), (1025, 5, 1, True), (1025, 64, "cap", False),
    (1025, 256, 2, True), (1025, "wide", 2, False), (1, 256, 12, True), (1, "wide", "cap", False), (1025, 3, "cap", False),
]


@pytest.mark.parametrize("td", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n,p,S,keep", CASES)
def test_update_against_float64(td, n, p, S, keep):
    p = (260 if td == torch.float32 else 258) if p == "wide" else p
    S = _cap() if S == "cap" else S
    rows = _backend.ciq_geometry(td, n, p)[2]
    assert n % rows != 0, "n must leave a partial workgroup"
    rng = np.random.default_rng(1000 * n + 10 * p + S)
    st = _state(rng, td, n, p, S, keep)
    got = _launch(st, td)
    _check(st, got, td, f"{td} n {n} p {p} S {S} keep {keep}")
    again = _launch(st, td)
    for key, v in got.items():
        assert v is None or np.array_equal(_bits(v), _bits(again[key])), f"{key}: two launches must give the same bits"


@pytest.mark.parametrize("td", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n,p,S", [(37, 5, 12), (1025, 8, 2), (37, "wide", 12), (37, 1, 2)])
def test_done_columns_and_the_stop_word(td, n, p, S):
    p = (260 if td == torch.float32 else 258) if p == "wide" else p
    rng = np.random.default_rng(77 + n + p)
    cols = sorted({0, p // 2, p - 1} | ({1, 2, 6} & set(range(p))))       # inside one 16-byte lane and across lanes
    if p == 1:
        cols = [0]
    st = _state(rng, td, n, p, S, True, done_cols=cols)
    got = _launch(st, td)
    _check(st, got, td, f"{td} n {n} p {p} S {S} done {cols}")
    for key, src in (("w", st["wpp"]), ("acc", st["acc"])):
        assert np.array_equal(_bits(got[key][..., cols]), _bits(src[..., cols])), f"{key}: a done column keeps every bit"
    assert np.array_equal(_bits(got["keep"][:, :, cols]), _bits(st["keep"][:, :, cols]))
    # (a done column's z is still normalised: _check holds every column of z against zc / beta)
    # the stop word: nothing at all is written
    st2 = _state(rng, td, n, p, S, True, stop=1)
    got2 = _launch(st2, td)
    for key, src in (("z", st2["zc"]), ("w", st2["wpp"]), ("acc", st2["acc"]), ("keep", st2["keep"])):
        assert np.array_equal(_bits(got2[key]), _bits(src)), f"{key} was written under a set stop word"


@pytest.mark.parametrize("td", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("p,S", [(1, 1), (5, 12), (256, 2), (300, 12), (1024, "cap")])
def test_stop(td, p, S):
    S = _cap() if S == "cap" else S
    t = NP[td]
    rng = np.random.default_rng(p + S)
    tol = 1e-3
    scal = rng.standard_normal((S, 12, p)).astype(t)
    scal[:, 6] = rng.uniform(1e-5, 9e-4, (S, p)) * rng.choice([-1.0, 1.0], (S, p))           # every column below tol ...
    big = np.arange(p) % 3 == 1
    scal[rng.integers(0, S), 6, big] = -0.5                                                   # ... but these: one shift above it
    nan = np.arange(p) % 7 == 3
    scal[rng.integers(0, S), 6, nan] = np.nan                                                 # NaN is never done
    exact = np.arange(p) % 5 == 0
    scal[:, 6, exact & ~big & ~nan] = t(tol)                                                  # est == tol is done (<=)
    done = np.zeros(p, dtype=np.int32)
    sticky = np.arange(p) % 4 == 2
    done[sticky] = 1                                                                          # done stays done whatever est says
    est = np.full(p, -1.0, dtype=t)

    def run(scal_np, done_np, flags_np, tol_v):
        d = [torch.from_numpy(x.copy()).to(DEV) for x in (scal_np, est, done_np, flags_np)]
        _backend.ciq_stop(d[0], tol_v, d[1], d[2], d[3])
        torch.cuda.synchronize()
        assert np.array_equal(d[0].cpu().numpy(), scal_np, equal_nan=True)
        return d[1].cpu().numpy(), d[2].cpu().numpy(), d[3].cpu().numpy()

    flags = np.array([0, 5], dtype=np.int32)
    got = run(scal, done, flags, float(t(tol)))
    want = CR.stop_step(scal, t(tol), est, done, flags)
    for g, w, name in zip(got, want, ("est", "done", "flags")):
        assert np.array_equal(g, w, equal_nan=True), name
    assert np.array_equal(got[1] != 0, sticky | ~(big | nan)) and got[2][1] == 5
    assert np.all(np.isnan(got[0][nan])) and np.all(got[0][big & ~nan] == 0.5)
    assert got[2][0] == (1 if (sticky | ~(big | nan)).all() else 0)
    # every column done -> the stop word; a set stop word -> nothing is written
    all_done = run(scal, np.ones(p, dtype=np.int32), flags, float(t(tol)))
    assert all_done[2][0] == 1 and np.all(all_done[1] == 1)
    clean = scal.copy()
    clean[:, 6] = 1e-6
    assert run(clean, np.zeros(p, dtype=np.int32), flags, float(t(tol)))[2][0] == 1
    frozen = run(clean, np.zeros(p, dtype=np.int32), np.array([1, 5], dtype=np.int32), float(t(tol)))
    assert np.all(frozen[0] == -1.0) and np.all(frozen[1] == 0) and frozen[2][0] == 1


def test_refusals_launch_nothing():
    """Each documented refusal returns its code; the buffers of a refused launch keep their bits."""
    lib = _backend.load_library()
    cap = _cap()
    n, p, S = 37, 8, 3
    td = torch.float32
    rng = np.random.default_rng(3)
    st = _state(rng, td, n, p, S, True)
    dev = {k: torch.from_numpy(v).to(DEV) for k, v in st.items()}
    plane = n * p
    w0, w1 = dev["wpp"].reshape(S, plane).contiguous(), dev["wp"].reshape(S, plane).contiguous()
    snapshot = {k: v.clone() for k, v in dev.items()}
    stream = torch.cuda.current_stream(DEV).cuda_stream

    def update(**ch):
        a = dict(vtype=0, n=n, p=p, n_shift=S, zc=dev["zc"].data_ptr(), zp=dev["zp"].data_ptr(), wpp=w0.data_ptr(), wp=w1.data_ptr(),
                 shift_stride=plane, acc=dev["acc"].data_ptr(), keep=dev["keep"].data_ptr(), scal=dev["scal"].data_ptr(),
                 omega=dev["omega"].data_ptr(), done=dev["done"].data_ptr(), flags=dev["flags"].data_ptr())
        a.update(ch)
        return lib.tsgu_ciq_update(*a.values(), 0, stream)

    est = torch.zeros(p, device=DEV)

    def stop(**ch):
        a = dict(vtype=0, p=p, n_shift=S, scal=dev["scal"].data_ptr(), tol=1e-4, est=est.data_ptr(), done=dev["done"].data_ptr(),
                 flags=dev["flags"].data_ptr())
        a.update(ch)
        return lib.tsgu_ciq_stop(*a.values(), 0, stream)

    for key in ("zc", "zp", "wpp", "wp", "acc", "scal", "omega", "done", "flags"):
        assert update(**{key: None}) == A.BAD_ARG, key
    for key in ("zc", "zp", "wpp", "wp", "acc", "keep"):
        assert update(**{key: dev["zc"].data_ptr() + 4}) == A.BAD_ARG, f"{key}: 16-byte alignment"
    for key in ("scal", "omega", "done", "flags"):
        assert update(**{key: dev[key].data_ptr() + 2}) == A.BAD_ARG, f"{key}: element alignment"
    for ch in (dict(n=0), dict(p=0), dict(n_shift=0), dict(shift_stride=plane - 4), dict(shift_stride=plane + 2)):
        assert update(**ch) == A.BAD_ARG, ch
    assert update(vtype=2) == A.BAD_DTYPE and update(vtype=9) == A.BAD_DTYPE
    assert update(n_shift=cap + 1) == A.TOO_LARGE and update(n=1, p=257, shift_stride=260) == A.TOO_LARGE
    for key in ("scal", "est", "done", "flags"):
        assert stop(**{key: None}) == A.BAD_ARG, key
    assert stop(p=0) == A.BAD_ARG and stop(n_shift=0) == A.BAD_ARG and stop(est=est.data_ptr() + 2) == A.BAD_ARG
    assert stop(vtype=2) == A.BAD_DTYPE and stop(n_shift=cap + 1) == A.TOO_LARGE
    torch.cuda.synchronize()
    for k, v in snapshot.items():
        assert torch.equal(dev[k], v), f"{k} changed under a refused launch"
    assert torch.equal(est, torch.zeros(p, device=DEV))
