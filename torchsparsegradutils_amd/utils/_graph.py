"""hipGraph capture of a launch-bound iteration chunk.

The Krylov loops keep every scalar, flag and iteration counter on the device, so one iteration is the same
sequence of launches every time and a chunk of iterations can be recorded once and replayed with a single
host call (iterations after convergence are device-side no-ops).  Allocations made inside the chunk come
from the graph's private pool and stay valid across replays."""

from __future__ import annotations

import os

import torch

MIN_ITERS = int(os.environ.get("TSGU_GRAPH_MIN_ITERS", "64"))  # remaining iterations that justify a capture (0: never)
STATS = {"captures": 0, "replays": 0, "last_error": None}  # diagnostics for tests / tuning


def enabled() -> bool:
    return MIN_ITERS > 0 and not torch.cuda.is_current_stream_capturing()


def capture(body, repeat: int):
    """Record ``repeat`` calls of ``body`` (kernel launches on the current stream, no host reads) into a
    hipGraph.  Only bodies made of this package's own launches are recorded (the callers never pass a user
    callable: an operator that synchronises or calls a non-capturable library would poison the stream).
    Returns None if the runtime refuses the capture; nothing has executed in that case."""
    graph = torch.cuda.CUDAGraph()
    try:
        # thread_local: the plan builder's worker thread (or any other thread of the application) may allocate or
        # launch on its own stream while this thread records
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            for _ in range(repeat):
                body()
    except Exception as exc:  # noqa: BLE001
        STATS["last_error"] = repr(exc)
        return None
    STATS["captures"] += 1
    return graph


def replay(graph) -> None:
    graph.replay()
    STATS["replays"] += 1


def run_chunked(body, poll, chunk, *, bound=None, expected=None, first=None, capture_from=None, capturable=False,
                snapshot=None, restore=None):
    """The host schedule of every fused Krylov loop: queue iterations in runs, read the stop word after each run, and
    once the solve is clearly a long one record ``chunk`` iterations as a hipGraph and replay that.

    ``body(j)`` queues one iteration, ``j`` its position inside the current run; ``poll() -> bool`` is the caller's
    read of its stop word (iterations queued past the stop are no-ops on the device).  The first run is ``first``
    iterations (default ``chunk``) and always eager, every later one ``chunk``, all clipped to ``bound`` (None: the
    device ends the solve).  From ``capture_from`` iterations on (default ``first``), while a whole chunk fits under
    the bound and ``expected - k >= MIN_ITERS`` (``expected``: iterations the solve may still need, default ``bound``),
    a ``capturable`` loop makes ONE capture attempt; afterwards a run is a replay when the graph exists and a whole
    chunk fits, eager otherwise.  ``capturable`` is the caller's promise that the body is only this package's own
    launches, and includes ``enabled()``.  A refused capture has run the Python of ``body`` but nothing on the
    device: ``snapshot()`` is taken before the attempt and ``restore(snapshot)`` puts the host's view back.  A chunk
    that is recorded must leave that view where it was (an even number of buffer swaps).
    Returns (iterations queued, last poll result)."""
    first = chunk if first is None else first
    capture_from = first if capture_from is None else capture_from
    expected = bound if expected is None else expected
    k, done, graph = 0, False, None
    while not done and (bound is None or k < bound):
        fits = bound is None or k + chunk <= bound
        if capturable and fits and k >= capture_from and expected - k >= MIN_ITERS:
            saved = snapshot() if snapshot is not None else None
            position = iter(range(chunk))
            graph = capture(lambda: body(next(position)), chunk)
            capturable = False  # one attempt: what is left only falls
            if graph is None and restore is not None:
                restore(saved)
        if graph is not None and fits:
            replay(graph)
            k += chunk
        else:
            run = first if k == 0 else chunk
            if bound is not None:
                run = min(run, bound - k)
            for j in range(run):
                body(j)
            k += run
        done = poll()
    return k, done
