#!/usr/bin/env python3
"""Device time of the solution-sensitivity calls next to the solve they differentiate.

Two workloads at B = 8192, fp64:
  * quad13 N=20 on the bench's own first-step QPs (batched.first_step_qps): 99.6 % empty active sets;
  * the force N=20 B=48 pattern of tests/sens_ref.py (start states +-0.2 / +-0.6 off the reference), tiled to
    B = 8192: most sets non-empty, up to 39 bounds.
Per workload the median of `--reps` HIP-event timings (after a warm-up) of the stream-ordered calls
sens_forward_async(0), sens_adjoint_async() and solve_async() on the same handle. Prints one JSON line per
workload; --out writes them to a file as well.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from drone_attitude_control_amd import AcadosOcpSolver, _lib  # noqa: E402
from drone_attitude_control_amd.batched import first_step_qps, workload  # noqa: E402
from drone_attitude_control_amd.models import OCPS  # noqa: E402


def hip_runtime():
    _lib.load()
    hip = ctypes.CDLL("libamdhip64.so.7")
    hip.hipEventCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
    hip.hipEventRecord.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    hip.hipEventSynchronize.argtypes = [ctypes.c_void_p]
    hip.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, ctypes.c_void_p]
    hip.hipEventDestroy.argtypes = [ctypes.c_void_p]
    return hip


def timed(hip, s, call, reps, warmup=3):
    """Median / min device ms of `call()` between two events on the handle's stream."""
    stream = s.lib.nmpc_get_stream(s._h)
    e0, e1 = ctypes.c_void_p(), ctypes.c_void_p()
    assert hip.hipEventCreate(ctypes.byref(e0)) == 0 and hip.hipEventCreate(ctypes.byref(e1)) == 0
    ms = []
    for i in range(warmup + reps):
        assert hip.hipEventRecord(e0, stream) == 0
        call()
        assert hip.hipEventRecord(e1, stream) == 0
        assert hip.hipEventSynchronize(e1) == 0
        s.synchronize()
        t = ctypes.c_float()
        assert hip.hipEventElapsedTime(ctypes.byref(t), e0, e1) == 0
        if i >= warmup:
            ms.append(t.value)
    hip.hipEventDestroy(e0)
    hip.hipEventDestroy(e1)
    return float(np.median(ms)), float(np.min(ms))


def measure(hip, label, model, N, x0, yref, reps):
    B = x0.shape[0]
    s = AcadosOcpSolver(OCPS[model](N), batch=B)
    s.set_batch("x0", x0)
    s.set_batch("yref", yref)
    s.solve()
    _, _, st = s.sens_batch(0)
    rng = np.random.default_rng(11)
    s.adjoint_batch(rng.normal(size=(B, N + 1, s.nx)), rng.normal(size=(B, N, s.nu)))   # stages the cotangents
    U = s.get_batch("u")
    from oracle import models as om
    spec = om.MODELS[model](N)
    lbu, ubu = spec.lbu, spec.ubu
    on_u = ((U <= lbu + 1e-7 * (1 + np.abs(lbu))) | (U >= ubu - 1e-7 * (1 + np.abs(ubu)))).any(axis=(1, 2))
    res = {"workload": label, "model": model, "N": N, "batch": B, "reps": reps,
           "sens_status_counts": {int(k): int((st == k).sum()) for k in np.unique(st)},
           "instances_with_an_input_on_bound": int(on_u.sum())}
    for key, call in (("sens_forward_stage0", lambda: s.sens_forward_async(0)),
                      ("sens_forward_stageN", lambda: s.sens_forward_async(N)),
                      ("sens_adjoint", s.sens_adjoint_async),
                      ("solve", s.solve_async)):
        med, mn = timed(hip, s, call, reps)
        res[key + "_ms"] = {"median": round(med, 4), "min": round(mn, 4)}
    res["forward_over_solve"] = round(res["sens_forward_stage0_ms"]["median"] / res["solve_ms"]["median"], 3)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import sens_ref as sr
    hip = hip_runtime()
    out = []
    table, off, xi = workload("quad13", 20, a.batch)
    x0, yref = first_step_qps("quad13", 20, table, off, xi)
    out.append(measure(hip, "quad13 first-step QPs", "quad13", 20, x0, yref, a.reps))
    model, N, B, scale = sr.CASES["force_N20"]
    _, _, x0, Y, Ye = sr.inputs(model, N, B, scale)
    reps = (a.batch + B - 1) // B
    x0 = np.tile(x0, (reps, 1))[:a.batch]
    yref = np.tile(sr.stacked_yref(Y, Ye), (reps, 1))[:a.batch]
    out.append(measure(hip, "force N=20 B=48 pattern, tiled", "force", 20, x0, yref, a.reps))
    for r in out:
        print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in out:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
