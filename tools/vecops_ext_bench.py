#!/usr/bin/env python3
"""Times the extension-field vector operations (profiles/vecops_ext_notes.md) on device data, per field:
  add, sub, mul, div          two extension vectors in, one out: three streams of 16 bytes per element
  mixed_mul                   an extension vector times a base-field vector
  scalar_mul, inv             one extension vector in, one out
  sum, product                one read pass
  copy2, copy3                a device-to-device copy that moves as many bytes as two and as three such streams do: the ceiling
  base_inv                    vector_inv of the base field over the same bytes (4 or 2 times the element count)
Every call returns with its stream drained, so a host clock around it times the work, launch and synchronisation included. A timed
window is `inner` calls of one variant; the variants' windows run interleaved, `reps` times after a warm-up of each, and the median per
call is reported, with the fraction of the matching copy's bandwidth each operation reaches.
The seven-call emulation of an extension product through base-field operations is not timed: the base-field functions take
contiguous vectors only, and the coefficients of an extension vector are interleaved, so it cannot be expressed without transposing.
usage: tools/vecops_ext_bench.py [--fields babybear koalabear goldilocks] [--log-size 24] [--reps 9] [--inner 5] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STREAMS = {"add": 3, "sub": 3, "mul": 3, "div": 3, "scalar_mul": 2, "inv": 2, "base_inv": 2, "sum": 1, "product": 1, "copy2": 2, "copy3": 3}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--fields", nargs="+", default=["babybear", "koalabear", "goldilocks"])
    ap.add_argument("--log-size", type=int, default=24, help="log2 of the number of extension elements")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=5, help="calls per timed window")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from icicle_amd import VecOpsConfig, runtime, vecops
    from icicle_amd._lib import lib, check
    from icicle_amd.runtime import DeviceVec
    from oracle import pyref

    if runtime.get_device_count() < 1:
        sys.exit("vecops_ext_bench: no HIP device")
    runtime.set_device(0)
    rng = np.random.default_rng(1)
    median = lambda v: sorted(v)[len(v) // 2]
    results = []
    n = 1 << a.log_size
    for field in a.fields:
        p, bw = pyref.NTT_FIELDS[field].p, vecops._WORDS[field]
        if bw == 1:
            host = [rng.integers(0, p, size=(n, 4), dtype=np.uint32) for _ in range(2)]
        else:
            host = [rng.integers(0, p, size=(n, 2), dtype=np.uint64).view(np.uint32).reshape(n, 4) for _ in range(2)]
        host[0][::1000] = 0  # some zeros among the divisors
        vec_bytes = 16 * n
        A, B = [DeviceVec.from_host(h) for h in host]
        base = DeviceVec.from_host(np.ascontiguousarray(host[1][:, :bw]))
        scalar = DeviceVec.from_host(np.ascontiguousarray(host[1][:1]))
        out, red = DeviceVec(vec_bytes), DeviceVec(16)
        big = [DeviceVec(vec_bytes * 3 // 2) for _ in range(2)]
        cfg = VecOpsConfig.default

        def copy(dst, src, nbytes):  # the copy returns before it is done: drain the device as the vector functions drain their stream
            check(lib.icicle_copy(dst.ptr, src.ptr, nbytes), "icicle_copy")
            runtime.device_synchronize()

        ext = dict(size=n, extension=True)
        variants = {
            "copy2": lambda: copy(out, A, vec_bytes),
            "copy3": lambda: copy(big[0], big[1], vec_bytes * 3 // 2),
            "add": lambda: vecops.vector_add(field, A, B, cfg(), out=out, **ext),
            "sub": lambda: vecops.vector_sub(field, A, B, cfg(), out=out, **ext),
            "mul": lambda: vecops.vector_mul(field, A, B, cfg(), out=out, **ext),
            "mixed_mul": lambda: vecops.vector_mixed_mul(field, A, base, cfg(), out=out, size=n),
            "scalar_mul": lambda: vecops.scalar_mul_vec(field, scalar, B, cfg(), out=out, **ext),
            "inv": lambda: vecops.vector_inv(field, A, cfg(), out=out, **ext),
            "div": lambda: vecops.vector_div(field, B, A, cfg(), out=out, **ext),
            "sum": lambda: vecops.vector_sum(field, A, cfg(), out=red, **ext),
            "product": lambda: vecops.vector_product(field, B, cfg(), out=red, **ext),
            "base_inv": lambda: vecops.vector_inv(field, A, cfg(), out=out, size=n * 4 // bw),
        }
        for fn in variants.values():  # warm up every shape the timed window uses
            fn(), fn()
        times = {k: [] for k in variants}
        for _ in range(a.reps):
            for k, fn in variants.items():
                t0 = time.perf_counter()
                for _ in range(a.inner):
                    fn()
                times[k].append((time.perf_counter() - t0) * 1e3 / a.inner)
        ms = {k: median(v) for k, v in times.items()}
        streams = dict(STREAMS, mixed_mul=2 + bw / 4)
        gbps = {k: streams[k] * vec_bytes / ms[k] / 1e6 for k in ms}
        ceiling = {k: gbps["copy3" if streams[k] > 2 else "copy2"] for k in ms}
        row = {"field": field, "log_n": a.log_size, "vector_bytes": vec_bytes, "tile": vecops.extension_vector_inv_tile(field), "reps": a.reps, "inner": a.inner,
               "ms": {k: round(v, 4) for k, v in ms.items()}, "ms_min": {k: round(min(v), 4) for k, v in times.items()},
               "ms_max": {k: round(max(v), 4) for k, v in times.items()}, "GBps": {k: round(v, 1) for k, v in gbps.items()},
               "fraction_of_copy": {k: round(gbps[k] / ceiling[k], 3) for k in ms if not k.startswith("copy")},
               "inv_over_base_inv": round(ms["inv"] / ms["base_inv"], 2)}
        results.append(row)
        print(json.dumps(row), flush=True)
        for v in [A, B, base, scalar, out, red] + big:
            v.free()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
