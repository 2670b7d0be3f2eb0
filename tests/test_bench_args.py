"""bench.py's command line: a plain run is the headline figure alone; --full, off by default, adds the legs that run on their own
behind the timed region (CPU baseline, side measurements, streaming ceiling, the Lighting kernel alone)."""
import sys

import bench


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_full_is_off_by_default(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "20", "--warmup", "5")
    assert a.full is False
    assert (a.gpus, a.steps, a.warmup, a.dump_outputs) == (1, 20, 5, None)


def test_full_turns_the_other_legs_on(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "20", "--warmup", "5", "--full")
    assert a.full is True and not a.no_extras and not a.no_cpu_baseline
