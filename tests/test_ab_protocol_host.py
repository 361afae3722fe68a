"""``tools/ab_protocol.py`` on the host: the order in which ``alternate`` calls the forms and the timing source, ``stats`` against
``np.percentile``, and the strict rule ``wins`` that the knob defaults are decided by."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import ab_protocol as ab  # noqa: E402


class FakeSource:
    """A timing source that records what is asked of it into the list the forms write to."""

    def __init__(self, log):
        self.log = log

    def synchronise(self):
        self.log.append("sync")

    def start(self):
        self.log.append("start")

    def stop(self):
        self.log.append("stop")

    def elapsed(self):
        self.log.append("elapsed")
        return 1.0


def forms_into(log):
    return {"A": lambda: log.append("A"), "B": lambda: log.append("B")}


def test_every_form_is_warmed_then_the_forms_take_turns():
    log = []
    res = ab.alternate(forms_into(log), calls=2, rounds=3, warmup=1, source=FakeSource(log))
    assert [x for x in log if x in "AB"] == ["A", "B"] + ["A", "A", "B", "B"] * 3
    assert set(res) == {"A", "B"} and list(res["A"]) == ["host", "device"]
    assert res["B"]["device"] == {"median": 1.0, "p10": 1.0, "p90": 1.0}


@pytest.mark.parametrize("clocks, host_stops, call", [
    (("host", "device"), "before", ["sync", "start", "A", "stop", "elapsed"]),
    (("host", "device"), "after", ["sync", "start", "A", "stop", "sync", "elapsed"]),
    (("host",), "after", ["sync", "A", "sync"]),
    (("device",), "before", ["start", "A", "stop", "elapsed"]),
])
def test_what_surrounds_a_timed_call(clocks, host_stops, call):
    log = []
    res = ab.alternate({"A": lambda: log.append("A")}, calls=2, rounds=1, warmup=2, clocks=clocks, host_stops=host_stops,
                       source=FakeSource(log))
    assert log == ["A", "A", "sync"] + call * 2                  # the warm-up, one synchronise, the timed calls
    assert list(res["A"]) == list(clocks)


def test_before_runs_untimed_ahead_of_every_call():
    log = []
    ab.alternate(forms_into(log), calls=1, rounds=1, warmup=1, clocks=("device",), before=lambda name: log.append("before " + name),
                 source=FakeSource(log))
    assert log == ["before A", "A", "before B", "B", "sync", "before A", "start", "A", "stop", "elapsed", "before B", "start", "B", "stop",
                   "elapsed"]


def test_stats_are_numpy_s_percentiles():
    ms = [3.0, 1.0, 4.0, 1.5, 9.0, 2.6, 5.0, 3.5, 8.0, 9.7, 0.25]
    assert ab.stats(ms) == {"median": float(np.percentile(ms, 50)), "p10": float(np.percentile(ms, 10)), "p90": float(np.percentile(ms, 90))}
    assert ab.stats(ms)["p10"] == 1.0 and ab.stats(ms)["p90"] == 9.0             # 11 values: the second lowest and second highest


def test_wins_is_strict_and_reads_the_clock_it_is_told():
    def res(new_p90, old_p10, clock="host", other=(0.0, 1.0)):
        quiet = "device" if clock == "host" else "host"
        return {"new": {clock: {"p90": new_p90}, quiet: {"p90": other[0]}}, "old": {clock: {"p10": old_p10}, quiet: {"p10": other[1]}}}

    assert not ab.wins(res(2.0, 2.0), "new", "old", "host")
    assert ab.wins(res(np.nextafter(2.0, 0.0), 2.0), "new", "old", "host")
    assert not ab.wins(res(2.5, 2.0), "new", "old", "host")
    # the other clock says the opposite each time
    assert ab.wins(res(2.0, 2.0), "new", "old", "device")
    assert not ab.wins(res(2.0, 2.0, clock="device"), "new", "old", "device") and ab.wins(res(2.0, 2.0, clock="device"), "new", "old", "host")
    assert not ab.wins(res(1.0, 2.0, other=(3.0, 2.0)), "new", "old", "device")
