"""The host schedule of the fused Krylov loops (`_graph.run_chunked`) without a GPU: `_graph.capture` / `_graph.replay` are replaced
by fakes and the sequence of eager runs, capture attempts, replays and polls is compared with traces written down by hand for the
parameters of the four loops (both CG forms, MINRES, BiCGSTAB): `E n` = n eager body calls, `C` / `C✗` = capture recorded / refused,
`R` = replay, `P` = poll.  Also the fold / unfold helper for right-hand sides with batch dimensions."""

import pytest
import torch

from torchsparsegradutils_amd.utils import _graph
from torchsparsegradutils_amd.utils._operator import batch_fold


class Recorder:
    """Fakes for capture / replay and a body / poll pair that write the trace."""

    def __init__(self, monkeypatch, min_iters=64, refuse_after=None, done_at_poll=None, on_body=None):
        self.trace, self.runs = [], []      # runs: the body positions of every eager run and of every capture attempt, in order
        self.eager, self.polls, self.replays = [], 0, 0
        self.refuse_after, self.done_at_poll, self.on_body = refuse_after, done_at_poll, on_body
        self.capturing = None
        monkeypatch.setattr(_graph, "MIN_ITERS", min_iters)
        monkeypatch.setattr(_graph, "capture", self.capture)
        monkeypatch.setattr(_graph, "replay", self.replay)

    def _flush(self):
        if self.eager:
            self.trace.append(f"E{len(self.eager)}")
            self.runs.append(("E", self.eager))
            self.eager = []

    def body(self, j):
        (self.eager if self.capturing is None else self.capturing).append(j)
        if self.on_body is not None:
            self.on_body()

    def poll(self):
        self._flush()
        self.trace.append("P")
        self.polls += 1
        return self.done_at_poll is not None and self.polls >= self.done_at_poll

    def capture(self, body, repeat):
        self._flush()
        self.capturing = []
        for _ in range(repeat if self.refuse_after is None else self.refuse_after):
            body()
        self.runs.append(("C", self.capturing))
        self.capturing = None
        self.trace.append("C" if self.refuse_after is None else "C✗")
        return None if self.refuse_after is not None else "graph"

    def replay(self, graph):
        assert graph == "graph"
        self._flush()
        self.trace.append("R")
        self.replays += 1


def T(text):
    """'E11 P C (R P)x24 E3 P' -> the list of tokens."""
    out, toks, i = [], text.split(), 0
    while i < len(toks):
        if toks[i].startswith("("):
            j = i
            while ")" not in toks[j]:
                j += 1
            group = [t.strip("()") for t in toks[i:j]] + [toks[j].split(")")[0]]
            out += group * int(toks[j].split(")x")[1])
            i = j + 1
        else:
            out.append(toks[i])
            i += 1
    return out


def cg(bound, min_iter_index=10):
    return dict(chunk=8, bound=bound, first=max(8, min_iter_index + 1))


MINRES = dict(chunk=10)
BICGSTAB = dict(chunk=4, capture_from=16)

# (name, driver arguments, MIN_ITERS, done at poll, trace, iterations queued)
CASES = [
    ("cg-203", cg(203), 64, None, "E11 P C (R P)x24", 203),
    ("cg-206", cg(206), 64, None, "E11 P C (R P)x24 E3 P", 206),
    ("cg-30", cg(30), 64, None, "E11 P E8 P E8 P E3 P", 30),
    ("cg-203-done-at-3", cg(203), 64, 3, "E11 P C R P R P", 27),
    ("cg-5", cg(5, min_iter_index=4), 64, None, "E5 P", 5),
    # 6 iterations left at the chunk boundary: a graph recorded here could never be replayed, so none is
    ("cg-17-min-iters-4", cg(17), 4, None, "E11 P E6 P", 17),
    # the poll after the tail is the value MINRES reports in last_solve_info
    ("minres-152", dict(MINRES, bound=152), 64, None, "E10 P C (R P)x14 E2 P", 152),
    ("minres-39", dict(MINRES, bound=39), 64, None, "(E10 P)x3 E9 P", 39),
    ("bicgstab-99", dict(BICGSTAB, expected=99), 64, 9, "(E4 P)x4 C (R P)x5", 36),
    ("bicgstab-60", dict(BICGSTAB, expected=60), 64, 9, "(E4 P)x9", 36),
]


@pytest.mark.parametrize("name,kw,min_iters,done_at,trace,queued", CASES, ids=[c[0] for c in CASES])
def test_schedule_of_each_loop(name, kw, min_iters, done_at, trace, queued, monkeypatch):
    rec = Recorder(monkeypatch, min_iters=min_iters, done_at_poll=done_at)
    k, done = _graph.run_chunked(rec.body, rec.poll, capturable=True, **kw)
    assert rec.trace == T(trace)
    assert k == queued and done == (done_at is not None)


@pytest.mark.parametrize("name,kw,min_iters,done_at,trace,queued", CASES, ids=[c[0] for c in CASES])
def test_not_capturable_never_captures(name, kw, min_iters, done_at, trace, queued, monkeypatch):
    rec = Recorder(monkeypatch, min_iters=min_iters, done_at_poll=done_at)
    k, done = _graph.run_chunked(rec.body, rec.poll, capturable=False, **kw)
    chunk, first = kw["chunk"], kw.get("first", kw["chunk"])
    # the same iterations in the same runs, all of them eager
    want, at = [], 0
    for tok in T(trace):
        if tok == "P":
            want.append("P")
        elif tok != "C":
            run = int(tok[1:]) if tok.startswith("E") else chunk
            assert run == (first if at == 0 else chunk) or at + run == kw["bound"]
            want.append(f"E{run}")
            at += run
    assert rec.trace == want and k == queued and done == (done_at is not None)


def test_refused_capture_restores_once_and_is_not_retried(monkeypatch):
    rec = Recorder(monkeypatch, refuse_after=3)
    snapshots, restored = [], []

    def snapshot():
        snapshots.append(("snapshot", len(rec.trace)))
        return snapshots[-1]

    k, done = _graph.run_chunked(rec.body, rec.poll, capturable=True, snapshot=snapshot, restore=restored.append, **cg(100))
    assert rec.trace == T("E11 P C✗ (E8 P)x11 E1 P") and k == 100 and not done
    assert snapshots == [("snapshot", 2)]           # taken once, after `E11 P` and before the attempt
    assert restored == snapshots                    # handed back exactly once
    assert rec.runs[1] == ("C", [0, 1, 2])


def test_minres_positions(monkeypatch):
    """The stopping test of MINRES is the body at position 9: the last call of every whole chunk, never in the tail."""
    for bound, tail in ((152, [0, 1]), (39, list(range(9)))):
        rec = Recorder(monkeypatch)
        _graph.run_chunked(rec.body, rec.poll, capturable=True, bound=bound, **MINRES)
        assert rec.runs[-1] == ("E", tail) and 9 not in rec.runs[-1][1]
        for kind, positions in rec.runs[:-1]:
            assert positions == list(range(10)), (kind, positions)
        assert ("C" in [kind for kind, _ in rec.runs]) == (bound == 152)


@pytest.mark.parametrize("refuse_after", [None, 0, 3, 8])
def test_host_state_after_a_capture(refuse_after, monkeypatch):
    """A body that flips a parity bit and swaps buffer roles, as the two-launch CG and MINRES bodies do.  A refused capture has run
    the Python body but nothing on the device, and leaves the state of the snapshot; a recorded chunk of even length leaves the
    state it started from.  So every eager iteration, and the first one baked into the graph at every replay, sees the parity of
    the number of iterations the device has executed."""
    state = {"parity": 0}
    roles = ["a", "b"]
    executed = [0]                                 # iterations the device has run
    baked, around_capture = [], {}

    def check(parity):
        assert parity == executed[0] % 2 and roles == (["a", "b"] if state["parity"] == 0 else ["b", "a"])

    def on_body():
        if rec.capturing is None:
            check(state["parity"])
            executed[0] += 1
        else:
            baked.append(state["parity"])
        state["parity"] ^= 1
        roles.reverse()

    def snapshot():
        around_capture["before"] = (dict(state), roles[:])
        return around_capture["before"]

    def restore(saved):
        state.update(saved[0])
        roles[:] = saved[1]
        around_capture["restored"] = True

    rec = Recorder(monkeypatch, refuse_after=refuse_after, on_body=on_body)
    fake_replay = rec.replay

    def replay(graph):
        check(baked[0])
        executed[0] += 8
        fake_replay(graph)

    monkeypatch.setattr(_graph, "replay", replay)
    k, _ = _graph.run_chunked(rec.body, rec.poll, capturable=True, snapshot=snapshot, restore=restore, **cg(100))
    assert k == executed[0] == 100
    assert around_capture["before"] == ({"parity": 1}, ["b", "a"])           # 11 eager iterations came first
    assert around_capture.get("restored", False) == (refuse_after is not None)
    assert (rec.replays > 0) == (refuse_after is None)
    assert (dict(state), roles) == ({"parity": 0}, ["a", "b"])               # 100 iterations: back where it started


def test_batch_fold_round_trip_and_layout():
    n, k = 5, 4
    t = torch.arange(2 * 3 * n * k, dtype=torch.float64).reshape(2, 3, n, k)
    fold, unfold, wrap = batch_fold(t.shape)
    f = fold(t)
    assert f.shape == (n, 6 * k)
    assert torch.equal(unfold(f), t)
    assert torch.equal(f[:, (1 * 3 + 2) * k + 1], t[1, 2, :, 1])     # column (item, j) of the folded layout
    # the two expressions this helper replaced
    nb, batch_shape = 6, (2, 3)
    assert torch.equal(f, t.reshape(nb, n, k).permute(1, 0, 2).reshape(n, nb * k))
    assert torch.equal(unfold(f), f.reshape(n, nb, k).permute(1, 0, 2).reshape(batch_shape + (n, k)))
    assert torch.equal(wrap(lambda v: 2 * v)(f), 2 * f)


def test_batch_unfold_with_a_leading_shift_dimension():
    n, k, shifts = 5, 4, 3
    nb, batch_shape = 6, (2, 3)
    _, unfold, _ = batch_fold((2, 3, n, k))
    s = torch.randn(shifts, n, nb * k, generator=torch.Generator().manual_seed(0))
    lead = (shifts,)
    want = s.reshape(lead + (n, nb, k)).movedim(-2, -3).reshape(lead + batch_shape + (n, k))
    got = unfold(s)
    assert got.shape == (shifts, 2, 3, n, k) and torch.equal(got, want)
    assert torch.equal(got[2, 1, 0, :, 3], s[2, :, (1 * 3 + 0) * k + 3])
