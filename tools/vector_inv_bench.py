#!/usr/bin/env python3
"""Times vector_inv / vector_div / vector_sum / vector_product (profiles/vector_inv_notes.md) on device data, per field and size:
  inv          vector_inv: one a^(p-2) chain per tile of icicle_hip_vector_inv_tile(words) elements
  inv_program  the same result by an `inverse` user program through execute_program: one chain per element
  div          vector_div
  div_program  that program followed by vector_mul
  sum, product the two reductions (one read pass)
  add          vector_add (two read passes, one write pass): the stream the reductions are set against, as bytes moved per second
Every call returns with its stream drained, so a host clock around it times the work, launch and synchronisation included. A timed
window is `inner` calls of one variant; the variants' windows run interleaved, `reps` times after a warm-up of each, and the median per
call is reported. The two routes to an inverse and to a quotient are compared byte for byte first.
usage: tools/vector_inv_bench.py [--cases babybear:24 bn254:22] [--reps 9] [--inner 5] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["babybear:16", "babybear:20", "babybear:24", "koalabear:24", "bn254:16", "bn254:20", "bn254:22", "bls12_381:22"])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=5, help="calls per timed window")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from icicle_amd import Program, VecOpsConfig, execute_program, runtime, vecops
    from icicle_amd._lib import SUMCHECK_FIELDS
    from icicle_amd.runtime import DeviceVec
    from tests.sumcheck_model import FIELDS

    if runtime.get_device_count() < 1:
        sys.exit("vector_inv_bench: no HIP device")
    runtime.set_device(0)
    rng = np.random.default_rng(1)
    median = lambda v: sorted(v)[len(v) // 2]
    results = []
    for case in a.cases:
        field, logn = case.split(":")
        n, w, p = 1 << int(logn), SUMCHECK_FIELDS[field], FIELDS[field][0]
        host = [rng.integers(0, 1 << 32, size=(n, w), dtype=np.uint64).astype(np.uint32) for _ in range(2)]
        for h in host:  # the top word below the modulus' top word: canonical
            h[:, w - 1] %= np.uint32(p >> (32 * (w - 1)))
        host[0][::1000] = 0  # some zeros: both routes give 0 for them
        vec_bytes = 4 * w * n
        A, B = [DeviceVec.from_host(h) for h in host]
        out = {k: DeviceVec(vec_bytes) for k in ("inv", "inv_program", "div", "div_program", "add")}
        red = {k: DeviceVec(4 * w) for k in ("sum", "product")}

        def inverse(x):
            x[1] = x[0].inverse()

        program = Program.from_function(field, inverse, 2)
        cfg = VecOpsConfig.default

        def div_program():
            t = out["div_program"]
            execute_program(field, [A, t], program, cfg(), size=n)
            vecops.vector_mul(field, B, t, cfg(), out=t, size=n)

        variants = {
            "inv": lambda: vecops.vector_inv(field, A, cfg(), out=out["inv"], size=n),
            "inv_program": lambda: execute_program(field, [A, out["inv_program"]], program, cfg(), size=n),
            "div": lambda: vecops.vector_div(field, B, A, cfg(), out=out["div"], size=n),
            "div_program": div_program,
            "sum": lambda: vecops.vector_sum(field, A, cfg(), out=red["sum"], size=n),
            "product": lambda: vecops.vector_product(field, A, cfg(), out=red["product"], size=n),
            "add": lambda: vecops.vector_add(field, A, B, cfg(), out=out["add"], size=n),
        }
        for fn in variants.values():  # warm up every shape the timed window uses
            fn(), fn()
        assert np.array_equal(out["inv"].to_host(), out["inv_program"].to_host()), "the two routes to an inverse disagree"
        assert np.array_equal(out["div"].to_host(), out["div_program"].to_host()), "the two routes to a quotient disagree"
        times = {k: [] for k in variants}
        for _ in range(a.reps):
            for k, fn in variants.items():
                t0 = time.perf_counter()
                for _ in range(a.inner):
                    fn()
                times[k].append((time.perf_counter() - t0) * 1e3 / a.inner)
        ms = {k: median(v) for k, v in times.items()}
        passes = {"inv": 2, "inv_program": 2, "div": 3, "div_program": 5, "sum": 1, "product": 1, "add": 3}
        row = {"field": field, "log_n": int(logn), "vector_bytes": vec_bytes, "tile": vecops.vector_inv_tile(field), "reps": a.reps, "inner": a.inner,
               "ms": {k: round(v, 4) for k, v in ms.items()}, "ms_min": {k: round(min(v), 4) for k, v in times.items()},
               "ms_max": {k: round(max(v), 4) for k, v in times.items()},
               "GBps": {k: round(passes[k] * vec_bytes / ms[k] / 1e6, 1) for k in ms},
               "inv_program_over_inv": round(ms["inv_program"] / ms["inv"], 2),
               "div_program_over_div": round(ms["div_program"] / ms["div"], 2)}
        results.append(row)
        print(json.dumps(row), flush=True)
        for v in [A, B] + list(out.values()) + list(red.values()):
            v.free()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
