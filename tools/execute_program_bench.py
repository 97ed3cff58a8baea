#!/usr/bin/env python3
"""Times execute_program (profiles/execute_program_notes.md) on device data, per field and size:
  predefined   E (A B - C) by the predefined program: one launch, five vector passes over memory
  three_calls  vector_mul, vector_sub, vector_mul into a scratch vector: three launches, nine passes
  copy         a device-to-device copy that moves five vectors' worth of bytes (half read, half written): the roof
  interp_eq    the same function as a user program, on the interpreter
  interp_chain a chain of 40 operations over two inputs, on the interpreter (three vector passes)
Every call returns with its stream drained (the copy is followed by a device synchronise), so a host clock around it times the work,
launch and synchronisation included. A timed window is `inner` calls of one variant; the variants' windows run interleaved, `reps`
times after a warm-up of each, and the median per call is reported. The three E (A B - C) variants are compared byte for byte first.
usage: tools/execute_program_bench.py [--cases babybear:24 bn254:22] [--reps 15] [--inner 20] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["babybear:24", "bn254:22"])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20, help="calls per timed window")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from icicle_amd import Program, VecOpsConfig, execute_program, runtime, vecops
    from icicle_amd._lib import SUMCHECK_FIELDS, check, lib
    from icicle_amd.runtime import DeviceVec
    from tests.sumcheck_model import FIELDS

    if runtime.get_device_count() < 1:
        sys.exit("execute_program_bench: no HIP device")
    runtime.set_device(0)
    rng = np.random.default_rng(1)
    median = lambda v: sorted(v)[len(v) // 2]
    results = []
    for case in a.cases:
        field, logn = case.split(":")
        n, w, p = 1 << int(logn), SUMCHECK_FIELDS[field], FIELDS[field][0]
        host = [rng.integers(0, 1 << 32, size=(n, w), dtype=np.uint64).astype(np.uint32) for _ in range(4)]
        for h in host:  # the top word below the modulus' top word: canonical
            h[:, w - 1] %= np.uint32(p >> (32 * (w - 1)))
        vec_bytes = 4 * w * n
        A, B, C, E = [DeviceVec.from_host(h) for h in host]
        out = {k: DeviceVec(vec_bytes) for k in ("predefined", "three_calls", "interp_eq", "interp_chain")}
        src, dst = DeviceVec(5 * vec_bytes // 2), DeviceVec(5 * vec_bytes // 2)
        predefined = Program.predefined(field, 1)

        def eq(x):
            x[4] = x[3] * (x[0] * x[1] - x[2])

        def chain(x):
            acc = x[0]
            for j in range(40):
                acc = acc * x[1] if j % 2 == 0 else acc + x[0]
            x[2] = acc

        user_eq, user_chain = Program.from_function(field, eq, 5), Program.from_function(field, chain, 3)
        cfg = VecOpsConfig.default

        def three_calls():
            t = out["three_calls"]
            vecops.vector_mul(field, A, B, cfg(), out=t, size=n)
            vecops.vector_sub(field, t, C, cfg(), out=t, size=n)
            vecops.vector_mul(field, E, t, cfg(), out=t, size=n)

        variants = {
            "predefined": lambda: execute_program(field, [A, B, C, E, out["predefined"]], predefined, cfg(), size=n),
            "three_calls": three_calls,
            "copy": lambda: (check(lib.icicle_copy(dst.ptr, src.ptr, src.nbytes)), runtime.device_synchronize()),
            "interp_eq": lambda: execute_program(field, [A, B, C, E, out["interp_eq"]], user_eq, cfg(), size=n),
            "interp_chain": lambda: execute_program(field, [A, B, out["interp_chain"]], user_chain, cfg(), size=n),
        }
        for fn in variants.values():  # warm up every shape the timed window uses
            fn(), fn()
        same = out["predefined"].to_host()
        assert np.array_equal(same, out["three_calls"].to_host()) and np.array_equal(same, out["interp_eq"].to_host()), "the variants disagree"
        times = {k: [] for k in variants}
        for _ in range(a.reps):
            for k, fn in variants.items():
                t0 = time.perf_counter()
                for _ in range(a.inner):
                    fn()
                times[k].append((time.perf_counter() - t0) * 1e3 / a.inner)
        ms = {k: median(v) for k, v in times.items()}
        passes = {"predefined": 5, "three_calls": 9, "copy": 5, "interp_eq": 5, "interp_chain": 3}
        row = {"field": field, "log_n": int(logn), "vector_bytes": vec_bytes, "reps": a.reps, "inner": a.inner,
               "ms": {k: round(v, 4) for k, v in ms.items()}, "ms_min": {k: round(min(v), 4) for k, v in times.items()},
               "ms_max": {k: round(max(v), 4) for k, v in times.items()},
               "GBps": {k: round(passes[k] * vec_bytes / ms[k] / 1e6, 1) for k in ms},
               "predefined_over_three_calls": round(ms["predefined"] / ms["three_calls"], 3),
               "predefined_fraction_of_copy_roof": round(ms["copy"] / ms["predefined"], 3),
               "interp_eq_over_predefined": round(ms["interp_eq"] / ms["predefined"], 2),
               "interp_chain_over_predefined": round(ms["interp_chain"] / ms["predefined"], 2),
               "interp_eq_fraction_of_copy_roof": round(ms["copy"] / ms["interp_eq"], 3)}
        results.append(row)
        print(json.dumps(row), flush=True)
        for v in [A, B, C, E, src, dst] + list(out.values()):
            v.free()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
