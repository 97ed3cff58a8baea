#!/usr/bin/env python3
"""Times poly_eval and poly_division (profiles/poly_notes.md) on device data, per field:
  eval_point     poly_eval of 2^c coefficients on a domain of 2^d points: the plan takes the point route (one lane per point)
  eval_one       poly_eval of 2^n coefficients at ONE point: the plan takes the split route (a wave per chunk, then one chunk)
  eval_one_point the same call forced onto the point route ("hip_poly_eval_chunk" = -1): one lane walks the whole polynomial
  sum            vector_sum over the same 2^n coefficients: it reads the same bytes and does one multiplication less per element
  div_long / div_balanced / div_deg1   poly_division of 2^m coefficients by a denominator of degree 2^m - 2^(m-4), 2^(m-1) and 1
  ref_*          the reference CPU backend (oracle/_ref) on the same inputs, one call each, compared byte for byte with the device
Every device call returns with its stream drained, so a host clock around it times the work, launch and synchronisation included. A
timed window is `inner` calls of one variant; the windows of the variants of one case run interleaved, `reps` times after a warm-up of
each, and the median per call is reported.
usage: tools/poly_bench.py [--cases babybear:24:16 bn254:22:13] [--reps 9] [--inner 5] [--out FILE]     (field:n:m as above)"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["babybear:24:16", "goldilocks:23:15", "bn254:22:13", "bls12_377:20:13"])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=5, help="calls per timed window")
    ap.add_argument("--point-coeffs", type=int, default=10, help="log2 coefficients of eval_point")
    ap.add_argument("--point-domain", type=int, default=18, help="log2 points of eval_point")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from icicle_amd import runtime, vecops
    from icicle_amd.runtime import DeviceVec
    from tests import poly_ref as R

    if runtime.get_device_count() < 1:
        sys.exit("poly_bench: no HIP device")
    runtime.set_device(0)
    rng = np.random.default_rng(1)
    median = lambda v: sorted(v)[len(v) // 2]

    def rand_words(n, f, nonzero_top=True):
        p, w = R.modulus(f), R.FIELDS[f]
        if w == 1:
            x = rng.integers(0, p, size=(n, 1), dtype=np.uint32)
        else:
            x = rng.integers(0, 1 << 32, size=(n, w), dtype=np.uint64).astype(np.uint32)
            x[:, w - 1] %= np.uint32(p >> (32 * (w - 1)))
        if nonzero_top:
            x[n - 1, 0] |= 1
        return x

    def run_timed(variants):
        """variants: name -> (callable, inner); returns name -> median seconds per call"""
        for fn, _ in variants.values():
            fn()
        times = {k: [] for k in variants}
        for _ in range(a.reps):
            for k, (fn, inner) in variants.items():
                t0 = time.perf_counter()
                for _ in range(inner):
                    fn()
                times[k].append((time.perf_counter() - t0) / inner)
        return {k: median(v) for k, v in times.items()}

    def once(fn):
        t0 = time.perf_counter()
        r = fn()
        return r, time.perf_counter() - t0

    results = []
    for case in a.cases:
        f, logn, logm = case.split(":")
        logn, logm = int(logn), int(logm)
        w, p = R.FIELDS[f], R.modulus(f)
        eb = 4 * w
        # ---- evaluation ----
        n, pc, pd = 1 << logn, 1 << a.point_coeffs, 1 << a.point_domain
        coeffs, domain = rand_words(n, f), rand_words(pd, f, False)
        dc, dd = DeviceVec.from_host(coeffs), DeviceVec.from_host(domain)
        ev_many, ev_one, ev_one_pt, s_out = DeviceVec(pd * eb), DeviceVec(eb), DeviceVec(eb), DeviceVec(eb)
        variants = {
            "eval_point": (lambda: vecops.poly_eval(f, dc, dd, out=ev_many, coeffs_size=pc, domain_size=pd), a.inner),
            "eval_one": (lambda: vecops.poly_eval(f, dc, dd, out=ev_one, coeffs_size=n, domain_size=1), a.inner),
            "sum": (lambda: vecops.vector_sum(f, dc, out=s_out, size=n), a.inner),
        }
        t = run_timed(variants)
        one_point = lambda: vecops.poly_eval(f, dc, dd, out=ev_one_pt, coeffs_size=n, domain_size=1, chunk=-1)
        one_point()  # seconds per call: a warm-up and one timed call
        t["eval_one_point"] = once(one_point)[1]
        (ref_one, t_ref_one) = once(lambda: R.ref_eval(f, coeffs, n, domain[:1]))
        rp = min(pd, 1 << 12)  # the reference on a prefix of the domain: it is one CPU thread
        (ref_many, t_ref_many) = once(lambda: R.ref_eval(f, coeffs[:pc], pc, domain[:rp]))
        assert np.array_equal(ev_one.to_host(shape=(1, w)), ref_one) and np.array_equal(ev_one_pt.to_host(shape=(1, w)), ref_one), (f, "eval_one")
        assert np.array_equal(ev_many.to_host(shape=(pd, w))[:rp], ref_many), (f, "eval_point")
        row = {"field": f, "words": w, "eval_one_coeffs_log2": logn, "eval_point_coeffs_log2": a.point_coeffs, "eval_point_domain_log2": a.point_domain,
               "ms": {k: round(v * 1e3, 4) for k, v in t.items()},
               "ref_ms": {"eval_one": round(t_ref_one * 1e3, 2), "eval_point_scaled": round(t_ref_many * 1e3 * pd / rp, 2)},
               "eval_one_over_sum": round(t["eval_one"] / t["sum"], 2),
               "eval_one_GBps": round(n * eb / t["eval_one"] / 1e9, 1), "sum_GBps": round(n * eb / t["sum"] / 1e9, 1),
               "eval_point_Gmul_per_s": round(pc * pd / t["eval_point"] / 1e9, 2)}
        # ---- division ----
        m = 1 << logm
        num = rand_words(m, f)
        dn = DeviceVec.from_host(num)
        T = vecops.poly_division_tile(f)
        div, dens = {}, {"div_long": m - (m >> 4) + 1, "div_balanced": (m >> 1) + 1, "div_deg1": 2}
        keep = {}
        for name, bsz in dens.items():
            den = rand_words(bsz, f)
            db = DeviceVec.from_host(den)
            q_size = m - bsz + 1
            qo, ro = DeviceVec(q_size * eb), DeviceVec(m * eb)
            keep[name] = (den, db, q_size, qo, ro)
            div[name] = (lambda db=db, bsz=bsz, q_size=q_size, qo=qo, ro=ro: vecops.poly_division(f, dn, db, q_out=qo, r_out=ro, num_size=m, den_size=bsz, q_size=q_size, r_size=m),
                         max(1, a.inner // 2))
        td = run_timed(div)
        ref_div = {}
        for name, (den, db, q_size, qo, ro) in keep.items():
            (rq, rr), tr = once(lambda: R.ref_division(f, num, m, den, den.shape[0], q_size, m, guard=False))
            assert np.array_equal(qo.to_host(shape=(q_size, w)), rq) and np.array_equal(ro.to_host(shape=(m, w)), rr), (f, name)
            ref_div[name] = round(tr * 1e3, 2)
        row["division"] = {"numerator_log2": logm, "tile": T, "ms": {k: round(v * 1e3, 3) for k, v in td.items()}, "ref_ms": ref_div,
                           "tiles": {k: -(-(m - b + 1) // T) for k, b in dens.items()},
                           "speedup_over_ref": {k: round(ref_div[k] / (td[k] * 1e3), 1) for k in td}}
        print(json.dumps(row), flush=True)
        results.append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
