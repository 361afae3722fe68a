"""The A/B protocol of the tools that decide a knob's default, and the rule they decide by.

The rule: a knob defaults to on only if the new form's p90 lies strictly below the old form's p10 (``wins``), the forms
ALTERNATING in one process (``alternate``): after ``warmup`` calls of every form, ``rounds`` rounds in which each form in turn gets
``calls`` timed calls; per form and clock the median, p10 and p90 by ``np.percentile`` (``stats``).

What the tools vary is an argument of ``alternate``, not a copy of its loop:

* ``clocks``      "host" (``time.perf_counter`` around the call, started on an idle device: a synchronise precedes every call),
                  "device" (a pair of events on the stream around the call), or both.  Device events alone take no synchronise
                  before the call: the calls queue up behind each other as they do in use.
* ``host_stops``  "before" the closing synchronise — forms that end with their result on the host, so everything they launched has
                  finished when they return — or "after" it — forms that leave work on the device.
* ``before``      an untimed ``before(name)`` ahead of every call of form ``name``, warm-up calls included.
* ``source``      where synchronise and the device clock come from: ``CudaSource`` unless a test passes a stand-in.

Which clock a verdict reads is the tool's choice and is named at its ``wins`` / ``report`` call.

Also here, once: the command line the tools share (``add_arguments`` / ``parse``), the exit without a GPU (``require_gpu``), and
the writer of the result text (``emit``)."""
import os
import time

import numpy as np

CLOCKS = ("host", "device")


class CudaSource:
    """The timing source on ``torch.cuda``: ``start`` / ``stop`` record a fresh pair of events on the current stream (made ahead
    of the call, so that the host clock does not hold their construction), ``elapsed`` waits for the second and returns the ms
    between them."""

    def __init__(self):
        import torch
        self.cuda = torch.cuda
        self.pair = self.events()

    def events(self):
        return self.cuda.Event(enable_timing=True), self.cuda.Event(enable_timing=True)

    def synchronise(self):
        self.cuda.synchronize()

    def start(self):
        self.pair[0].record()

    def stop(self):
        self.pair[1].record()

    def elapsed(self):
        first, last = self.pair
        self.pair = self.events()
        last.synchronize()
        return first.elapsed_time(last)


def stats(ms):
    return {"median": float(np.median(ms)), "p10": float(np.percentile(ms, 10)), "p90": float(np.percentile(ms, 90))}


def time_call(fn, source, clocks=("device",), host_stops="before"):
    """One timed call of ``fn`` -> {clock: ms}."""
    host, device = "host" in clocks, "device" in clocks
    if host:
        source.synchronise()
        t0 = time.perf_counter()
    if device:
        source.start()
    fn()
    if device:
        source.stop()
    ms = {}
    if host:
        if host_stops == "after":
            source.synchronise()
        ms["host"] = (time.perf_counter() - t0) * 1e3
    if device:
        ms["device"] = source.elapsed()
    return ms


def alternate(forms, calls, rounds, warmup, clocks=CLOCKS, host_stops="before", before=None, source=None):
    """``{name: {clock: stats}}`` of the callables ``forms`` = {name: fn}, timed in turn as the module docstring says."""
    assert set(clocks) <= set(CLOCKS) and host_stops in ("before", "after")
    source = source or CudaSource()
    for name, fn in forms.items():
        for _ in range(warmup):
            if before:
                before(name)
            fn()
    source.synchronise()
    times = {name: {clock: [] for clock in CLOCKS if clock in clocks} for name in forms}
    for _ in range(rounds):
        for name, fn in forms.items():
            for _ in range(calls):
                if before:
                    before(name)
                for clock, ms in time_call(fn, source, clocks, host_stops).items():
                    times[name][clock].append(ms)
    return {name: {clock: stats(v) for clock, v in t.items()} for name, t in times.items()}


def wins(res, new, old, clock):
    """The rule for a default: the new form's p90 on ``clock`` strictly below the old form's p10."""
    return res[new][clock]["p90"] < res[old][clock]["p10"]


def report(title, res, new, old, lines, clock="host", width=10):
    """Appends the title, one line per form and clock, and the line of the medians' ratio and the rule on ``clock`` to ``lines``;
    returns ``wins``."""
    lines.append(f"# {title}")
    pad = max(len(c) for c in res[new])
    for name in (new, old):
        for c, s in res[name].items():
            lines.append(f"#   {name:{width}s} {c:{pad}s}: median {s['median']:9.4f}  p10 {s['p10']:9.4f}  p90 {s['p90']:9.4f}")
    won = wins(res, new, old, clock)
    wall = {"host": "host wall", "device": "device events"}[clock]
    lines.append(f"#   {wall} {old} / {new} = {res[old][clock]['median'] / res[new][clock]['median']:.2f} (medians); "
                 f"{new} p90 below {old} p10: {won}")
    return won


def add_arguments(ap, calls, rounds, warmup, out=True, what="form"):
    """``--calls / --rounds / --warmup / --out`` with the tool's defaults; ``rounds=None`` and ``out=False`` leave theirs out."""
    ap.add_argument("--calls", type=int, default=calls, help=f"timed calls per round and {what}")
    if rounds is not None:
        ap.add_argument("--rounds", type=int, default=rounds)
    ap.add_argument("--warmup", type=int, default=warmup)
    if out:
        ap.add_argument("--out", type=str, default=None)


def parse(ap):
    """The arguments, ``--out`` made absolute (some tools change their working directory)."""
    a = ap.parse_args()
    if getattr(a, "out", None):
        a.out = os.path.abspath(a.out)
    return a


def require_gpu(tool):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit(f"{tool}: no GPU visible; a timing taken without one says nothing")


def emit(lines, out=None):
    """The result text to stdout and, with ``out``, to that file."""
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text)
