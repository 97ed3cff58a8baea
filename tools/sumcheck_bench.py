#!/usr/bin/env python3
"""Times the sumcheck prover (profiles/sumcheck_notes.md): EQ_X_AB_MINUS_C over four polynomials of 2^k elements on the device, BabyBear
and BN254, a Keccak-256 transcript. Per size and field: the whole prove call (a host clock around a call that returns with its stream
drained) and, from device events around each round's two launches (icicle_hip_sumcheck_time_rounds), every round's time, the bytes
that round moves -- round 0 reads 4 n elements; round r >= 1 reads 4 n / 2^(r-1) and writes 4 n / 2^r while a later round reads them
-- and its bytes per second as a fraction of the roof: a device-to-device copy measured in the same run, in interleaved repetitions,
that moves the same byte count as round 0 (half of it read, half written).
usage: tools/sumcheck_bench.py [--log-n 20 22 24] [--fields babybear bn254] [--reps 7]"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, nargs="+", default=[20, 22, 24])
    ap.add_argument("--fields", nargs="+", default=["babybear", "bn254"])
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()

    from icicle_amd import ReturningValueProgram, Sumcheck, SumcheckTranscriptConfig, runtime
    from icicle_amd._lib import SUMCHECK_FIELDS, check, lib
    from icicle_amd.hash import Hasher
    from icicle_amd.runtime import DeviceVec
    from tests import sumcheck_model as sm

    if runtime.get_device_count() < 1:
        sys.exit("sumcheck_bench: no HIP device")
    runtime.set_device(0)
    check(lib.icicle_hip_sumcheck_time_rounds(True))
    rng = np.random.default_rng(1)
    median = lambda v: sorted(v)[len(v) // 2]
    for field in a.fields:
        p, w = sm.FIELDS[field][0], SUMCHECK_FIELDS[field]
        program = ReturningValueProgram.predefined(field, 1)
        tcfg = SumcheckTranscriptConfig(Hasher.keccak256(), "domain_separator_label", "round_poly_label", "round_challenge_label", 1)
        for logn in a.log_n:
            n, m, eb = 1 << logn, 4, 4 * w
            if w == 1:
                host = [rng.integers(0, p, size=n, dtype=np.uint32) for _ in range(m)]
            else:  # 8 random words with the top one below p's: canonical
                host = [rng.integers(0, 1 << 32, size=(n, w), dtype=np.uint64).astype(np.uint32) for _ in range(m)]
                for h in host:
                    h[:, w - 1] %= np.uint32(p >> (32 * (w - 1)))
            polys = [DeviceVec.from_host(h) for h in host]
            round_bytes = [m * n * eb] + [m * (n >> (r - 1)) * eb + (m * (n >> r) * eb if r + 1 < logn else 0) for r in range(1, logn)]
            src, dst = DeviceVec(round_bytes[0] // 2), DeviceVec(round_bytes[0] // 2)
            sc = Sumcheck(field)

            def prove():
                sc.prove(polys, 0, program, tcfg)

            def copy():
                check(lib.icicle_copy(dst.ptr, src.ptr, src.nbytes))
                check(lib.icicle_device_synchronize())

            prove(), copy()  # warm-up
            t_prove, t_copy, t_rounds = [], [], []
            ms, count = (ctypes.c_double * 64)(), ctypes.c_int()
            for _ in range(a.reps):
                t = time.perf_counter()
                prove()
                t_prove.append((time.perf_counter() - t) * 1e3)
                check(lib.icicle_hip_sumcheck_round_times(ms, 64, ctypes.byref(count)))
                assert count.value == logn, count.value
                t_rounds.append([ms[r] for r in range(logn)])
                t = time.perf_counter()
                copy()
                t_copy.append((time.perf_counter() - t) * 1e3)
            roof = round_bytes[0] / (median(t_copy) * 1e-3)  # bytes per second, read + written
            rounds = [median([t[r] for t in t_rounds]) for r in range(logn)]
            print(f"{field} 2^{logn}: prove median {median(t_prove):.3f} ms (min {min(t_prove):.3f}, max {max(t_prove):.3f}), kernels {sum(rounds):.3f} ms; "
                  f"copy of {round_bytes[0] >> 20} MiB moved: median {median(t_copy):.3f} ms = {roof / 1e12:.2f} TB/s", flush=True)
            for r in range(logn):
                rate = round_bytes[r] / (rounds[r] * 1e-3)
                print(f"{field} 2^{logn} round {r:2d}: {rounds[r]:8.4f} ms  {round_bytes[r] / 2**20:10.3f} MiB  {rate / 1e12:6.3f} TB/s  {100 * rate / roof:5.1f} % of the copy", flush=True)
            for v in polys + [src, dst]:
                v.free()
    check(lib.icicle_hip_sumcheck_time_rounds(False))


if __name__ == "__main__":
    main()
