"""The stream tests' worker: one fresh process a family of tests/stream_cases.py, so that its few streams each have a hardware
queue of their own.

    python tests/_stream_worker.py --family NAME --out DIR      ->  DIR/NAME.json

For every case: `want` is the call on a default-stream context, waited for (the path the rest of the suite holds to the oracle and the
float64 restatements); then two probes on a context made with the side stream A and called with the default stream current.

  H  the current stream is held: a bounded spin (torch.cuda._sleep) runs on the default stream, the call is made, A alone is waited for.
     The probe is valid only if the spin is still running then (otherwise something of the call went behind it: void, which fails). The
     outputs, read back on A, are `want`'s bytes; and again after a wait for the device, when whatever the call left on the default
     stream has landed.
  S  the context's stream is held: the input buffers hold a decoy, and on A the spin, then the copies of the real inputs over the decoy
     are queued. The call must return while the spin runs (`returned_early`; the cases of stream_cases.NOT_ASYNC are not held to that),
     and after a wait for the device the outputs are `want`'s bytes: a launch that ran ahead on another stream has read the decoy.

The spin of a case lasts 20 times what its call took on the default stream, at least 20 ms and at most 500 ms; its cycles are calibrated
once with events. Before anything, the preflight shows for (null, A), (A, null) and (A, B) that a one-element add_ on the second stream
completes while the spin holds the first: streams that share a hardware queue cannot tell anything, and are reported as that. The worker
stops at the first HIP error, and writes what it has."""
import argparse
import hashlib
import json
import sys
import time
import traceback
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from tests import stream_cases as SC  # noqa: E402

FILL = 0xA5
MIN_MS, MAX_MS, TIMES = 20.0, 500.0, 20.0


class Blocker:
    """torch.cuda._sleep, its cycles per millisecond measured once from two lengths (the difference takes the launch's own time out)."""

    def __init__(self, torch):
        self.torch = torch
        torch.cuda._sleep(1000)  # (the kernel is loaded)
        torch.cuda.synchronize()
        self.lengths = (2_000_000, 20_000_000)
        self.measured_ms = [self._time(c) for c in self.lengths]
        self.cycles_per_ms = (self.lengths[1] - self.lengths[0]) / max(self.measured_ms[1] - self.measured_ms[0], 1e-3)

    def _time(self, cycles):
        torch = self.torch
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        torch.cuda._sleep(cycles)
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def hold(self, stream, ms):
        """Queue the spin on `stream` and return the event recorded behind it."""
        torch = self.torch
        with torch.cuda.stream(stream):
            torch.cuda._sleep(int(ms * self.cycles_per_ms))
            held = torch.cuda.Event()
            held.record()
        return held


def duration_ms(call_ms):
    return min(MAX_MS, max(MIN_MS, TIMES * call_ms))


def preflight(torch, blocker):
    """(A, B, record): side streams that do not share a hardware queue with the null stream or each other, at most four candidates each."""
    null = torch.cuda.default_stream()
    word = torch.zeros(1, device="cuda")
    torch.cuda.synchronize()
    record = {"pairs": [], "ok": False}

    def independent(x, y, what):
        torch.cuda.synchronize()
        held = blocker.hold(x, 100.0)
        with torch.cuda.stream(y):
            word.add_(1)
        y.synchronize()
        free = not held.query()
        torch.cuda.synchronize()
        record["pairs"].append({"held": what[0], "free": what[1], "ok": free})
        return free

    def pick(checks, label):
        for _ in range(4):
            s = torch.cuda.Stream()
            if all(independent(x if x is not None else s, y if y is not None else s, (xn or label, yn or label)) for x, xn, y, yn in checks):
                return s
        return None

    a = pick([(null, "null", None, None), (None, None, null, "null")], "A")
    b = pick([(a, "A", None, None)], "B") if a is not None else None
    record["ok"] = a is not None and b is not None
    if not record["ok"]:
        record["why"] = "these streams share a queue: the probes cannot tell"
    return a, b, record


class Runner:
    duration_ms = staticmethod(duration_ms)

    def __init__(self, torch, blocker, a, b):
        from unclerenderer_amd.hotpath import HotPath
        self.torch, self.blocker, self.A, self.B = torch, blocker, a, b
        self.default, self.side = HotPath(0), HotPath(0, a)
        self.states = {}

    # ---- buffers ----
    def upload(self, array):
        from unclerenderer_amd.hotpath import to_device
        a = np.ascontiguousarray(array)
        if a.dtype == np.float16:
            a = a.view(np.uint16)
        return to_device(a.copy())

    def buffers(self, case, seed, st):
        """The case's inputs of `seed` and its outputs full of FILL, as device tensors; the device is waited for."""
        torch = self.torch
        fixed = case.fixed_inputs(st)
        d = {k: self.upload(v) for k, v in case.host(seed).items()}
        for k in fixed:
            fixed[k].copy_(d[k].view(fixed[k].dtype))
            d[k] = fixed[k]
        for k, (shape, dtype) in case.outputs().items():
            dt = getattr(torch, dtype)
            n = int(np.prod(shape)) * torch.empty(0, dtype=dt).element_size()
            d[k] = torch.full((n,), FILL, dtype=torch.uint8, device="cuda").view(dt).view(shape)
        torch.cuda.synchronize()
        return d

    def state(self, case, hp):
        key = (case.name, id(hp))
        if key not in self.states:
            with self.torch.cuda.stream(hp.stream):
                self.states[key] = case.prepare(hp, self.upload)
            self.torch.cuda.synchronize()
        return self.states[key]

    # ---- results ----
    def read(self, case, got):
        """{name: bytes} of every returned tensor, by a copy on the current stream, and the call's host results."""
        tensors = {k: v for k, v in got.items() if not k.startswith("_")}
        raw = {k: v.contiguous().view(-1).view(self.torch.uint8).cpu().numpy() for k, v in tensors.items()}
        extra = dict(raw)
        if "constants" in tensors:
            extra["_constants_address"] = tensors["constants"].data_ptr()
        out = {k: np.ascontiguousarray(case.canonical(k, v, extra)).tobytes() for k, v in raw.items()}
        host = case.host_results(got)
        if host is not None:
            out["host results"] = json.dumps(host).encode()
        return out

    @staticmethod
    def differing(got, want):
        bad = []
        for k in want:
            if got.get(k) != want[k]:
                g, w = np.frombuffer(got.get(k, b""), np.uint8), np.frombuffer(want[k], np.uint8)
                if g.size == w.size:
                    at = np.flatnonzero(g != w)
                    bad.append(f"{k}: {at.size} of {w.size} bytes differ, first at {int(at[0])}")
                else:
                    bad.append(f"{k}: {g.size} bytes, want {w.size}")
        return bad

    # ---- the three runs of a case ----
    def want(self, case):
        """(bytes of the call on the default-stream context, what the call took in ms): run twice, the second timed; both the same bytes."""
        torch = self.torch
        st = self.state(case, self.default)
        results, ms = [], 0.0
        for _ in range(2):
            d = self.buffers(case, SC.REAL, st)
            t0 = time.perf_counter()
            got = case.call(self.default, st, d)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            results.append(self.read(case, got))
        if results[0] != results[1]:
            raise AssertionError(f"{case.name}: two runs on the default stream differ: {self.differing(results[0], results[1])}")
        return results[1], ms

    def probe_h(self, case, want, ms):
        torch = self.torch
        st = self.state(case, self.side)
        d = self.buffers(case, SC.REAL, st)
        held = self.blocker.hold(torch.cuda.default_stream(), ms)
        got = case.call(self.side, st, d)
        self.A.synchronize()
        valid = not held.query()
        with torch.cuda.stream(self.A):
            on_stream = self.read(case, got)
        torch.cuda.synchronize()
        after = self.read(case, got)
        rec = {"valid": valid, "on_stream": self.differing(on_stream, want), "after_device_wait": self.differing(after, want)}
        rec["ok"] = valid and not rec["on_stream"] and not rec["after_device_wait"]
        return rec

    def probe_s(self, case, want, ms):
        torch = self.torch
        st = self.state(case, self.side)
        d = self.buffers(case, SC.DECOY, st)
        real = {k: self.upload(v) for k, v in case.host(SC.REAL).items()}
        torch.cuda.synchronize()
        held = self.blocker.hold(self.A, ms)
        with torch.cuda.stream(self.A):
            for k, v in real.items():
                d[k].copy_(v)
        got = case.call(self.side, st, d)
        returned_early = not held.query()
        torch.cuda.synchronize()
        after = self.read(case, got)
        must = case.name not in SC.NOT_ASYNC
        rec = {"returned_early": returned_early, "must_return_early": must, "after_device_wait": self.differing(after, want)}
        rec["ok"] = (returned_early or not must) and not rec["after_device_wait"]
        return rec

    def decoy(self, case, want):
        """What probe S can show: "differs" when the decoy's own outputs on the default-stream context are other bytes than `want`
        (else a launch that read the decoy would pass: that fails the case), "none" for a case without device inputs."""
        if not case.host(SC.DECOY):
            return "none"
        st = self.state(case, self.default)
        got = case.call(self.default, st, self.buffers(case, SC.DECOY, st))
        self.torch.cuda.synchronize()
        return "differs" if self.differing(self.read(case, got), want) else "same"

    def run(self, case, probes="HS"):
        want, call_ms = self.want(case)
        ms = duration_ms(call_ms)
        rec = {"call_ms": round(call_ms, 3), "blocker_ms": round(ms, 1), "sha256": {k: hashlib.sha256(v).hexdigest()[:16] for k, v in want.items()}}
        rec["ok"] = True
        if "H" in probes:
            rec["H"] = self.probe_h(case, want, ms)
            rec["ok"] = rec["ok"] and rec["H"]["ok"]
        if "S" in probes:
            decoy = self.decoy(case, want)
            rec["S"] = self.probe_s(case, want, ms)
            rec["S"]["decoy"] = decoy  # ("none": S has no decoy, it holds the call to returning early and to the bytes alone)
            rec["S"]["ok"] = rec["S"]["ok"] and decoy != "same"
            rec["ok"] = rec["ok"] and rec["S"]["ok"]
        return rec

    def close(self):
        self.states.clear()
        self.default.close()
        self.side.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--family", required=True, choices=sorted(SC.FAMILIES))
    ap.add_argument("--out", required=True)
    ap.add_argument("--only", default=None, help="one case of the family (a tool's run; the tests run whole families)")
    ap.add_argument("--probes", default="HS", choices=("HS", "H", "S"), help="the probes to apply (a tool's run; the tests apply both)")
    args = ap.parse_args()
    out = Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    result = {"family": args.family, "cases": {}, "error": None}
    rc = 0
    try:
        import torch
        blocker = Blocker(torch)
        result["calibration"] = {"cycles": list(blocker.lengths), "ms": [round(v, 3) for v in blocker.measured_ms], "cycles_per_ms": round(blocker.cycles_per_ms)}
        a, b, result["preflight"] = preflight(torch, blocker)
        if result["preflight"]["ok"]:
            runner = Runner(torch, blocker, a, b)
            if args.family == "frame":
                from tests import _stream_frames
                _stream_frames.run(runner, result["cases"], args.only)
            else:
                for name, case in SC.cases(args.family).items():
                    if args.only in (None, name):
                        try:
                            result["cases"][name] = runner.run(case, args.probes)
                        except SC.HOST_ERRORS:  # (the case's own host code or a comparison: the next case may run)
                            result["cases"][name] = {"ok": False, "error": traceback.format_exc()}
                        print(name, "ok" if result["cases"][name]["ok"] else "FAILED", flush=True)
            torch.cuda.synchronize()
            runner.close()
    except Exception:  # (a HIP error among them: nothing more is started)
        result["error"] = traceback.format_exc()
        print(result["error"], file=sys.stderr, flush=True)
        rc = 1
    (out / f"{args.family}.json").write_text(json.dumps(result, indent=1))
    return rc


if __name__ == "__main__":
    sys.exit(main())
