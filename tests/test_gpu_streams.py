"""Every call on its context's stream, off the default one: the records of tests/_stream_worker.py, one fresh process a
family of tests/stream_cases.py, one test a case.

A case passes when both probes do. H (the default stream is held while the call runs on a side-stream context): the probe was valid - the
spin on the default stream was still running when the side stream had finished - and the outputs are the default-stream call's bytes, read
on the side stream and again after a wait for the device. S (the side stream is held, the real inputs queued behind the spin over a decoy):
the call returned while the spin ran (the host-upload wrappers of stream_cases.NOT_ASYNC excepted) and the outputs are the same bytes. A
void probe, a preflight that could not tell the streams apart, and a worker that ended early all fail every case they leave open."""
import json
import sys
from pathlib import Path

import pytest

from tests import stream_cases as SC

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
WORKER = str(ROOT / "tests" / "_stream_worker.py")

# Measured on an MI355X, a worker from its start to its end (python and torch starting, the preflight, every case's runs with their spins of
# 20 ms, up to 130 ms in the frame family): visibility 3.0 s, lighting 2.6 s, post 3.1 s, raster 3.3 s, builds 3.4 s, frame 4.3 s (the
# 2^20-instance case included). Some thirty times the slowest: the limit is for a worker that hangs, not for a slow one.
TIMEOUT = 120

_RECORDS = {}


@pytest.fixture(scope="module")
def family_record(hotpath, spawn_ranks, tmp_path_factory):
    """family_record(name) -> the worker's result file of that family; the worker runs once, whatever it ends with."""
    def run(family):
        if family not in _RECORDS:
            out = tmp_path_factory.mktemp(f"streams_{family}")
            res = spawn_ranks([sys.executable, WORKER, "--family", family, "--out", str(out)], [dict(OMP_NUM_THREADS=4)], timeout=TIMEOUT)
            file = out / f"{family}.json"
            _RECORDS[family] = (res, json.loads(file.read_text()) if file.exists() else None)
        return _RECORDS[family]
    yield run
    _RECORDS.clear()


@pytest.mark.parametrize("family,case", [(f, c) for f, names in SC.FAMILIES.items() for c in names])
def test_the_call_is_on_its_contexts_stream(family_record, record_property, family, case):
    res, record = family_record(family)
    assert res["rc"] == [0] and record is not None and record["error"] is None, f"the {family} worker failed:\n" + "\n".join(res["tail"]) + \
        ("\n" + str(record["error"]) if record else "")
    assert record["preflight"]["ok"], record["preflight"]
    assert case in record["cases"], f"the {family} worker has no record of {case}: {sorted(record['cases'])}"
    rec = record["cases"][case]
    record_property("blocker_ms", rec.get("blocker_ms"))  # (two_contexts has no spin and no probe: None)
    record_property("call_ms", rec.get("call_ms"))
    for probe, flags in (("H", ("valid",)), ("S", ("returned_early", "must_return_early"))):
        for flag in flags:
            record_property(f"{probe}.{flag}", rec.get(probe, {}).get(flag))
    print(json.dumps(rec, indent=1))
    assert rec["ok"], json.dumps(rec, indent=1)
