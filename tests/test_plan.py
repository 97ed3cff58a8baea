"""CPU: the NTT pass decomposition (icicle_amd/csrc/ntt_plan.h) compiled for the host -- every pass covers a row exactly
once and the last pass's scatter is a permutation, for every size up to 2^27 (31-bit fields) / 2^22 (256-bit fields); the
lane-native launch geometry of interleaved transforms (ntt_plan.h fast_pass_geometry, what ntt_run launches) maps every
logical element to the same word with and without column / outer-index groups."""
import ctypes
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def _lib():
    so = os.path.join(HERE, "_build", "libplan.so")
    os.makedirs(os.path.dirname(so), exist_ok=True)
    src = os.path.join(HERE, "plan_harness.cpp")
    hdrs = [os.path.join(HERE, "..", "icicle_amd", "csrc", h) for h in ("ntt_plan.h", "msm_plan.h")]
    if not os.path.exists(so) or max([os.path.getmtime(src)] + [os.path.getmtime(h) for h in hdrs]) > os.path.getmtime(so):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", src, "-o", so])
    return ctypes.CDLL(so)


def test_ntt_plan_covers_every_slot_once():
    lib = _lib()
    assert lib.plan_check(27, 22) == 0
    assert lib.msm_groups_check() == 0  # window groups of the pipelined MSM schedule (msm_plan.h)
    assert lib.split_shape_check() == 0  # shapes of a transform split over device slots (ntt_plan.h)
    assert lib.msm_plan_check() == 0  # the window plan of msm() (msm_plan.h make_plan)
    # ECNTT: stage widths + the radix-2^r matrix-form index algebra, simulated mod a small prime against the O(n^2) definition
    assert lib.ecntt_plan_check() == 0


def test_lane_native_geometry_groups_change_no_address():
    """Interleaved transforms (columns_batch 2..160, 192, 256 columns; the extension field, columns and rows), every size 2^1..2^27,
    kNN / kNR / kRN / kRR, plain and both coset directions: for every pass, grouped launch rows (cg columns in pass 0 / the last pass,
    ag outer indices in the middle one) touch exactly the words the ungrouped pass assigns to the same logical element, never a
    padding lane of the padded work buffer, never a word outside the buffer (tests/plan_harness.cpp lane_plan_check; a non-zero
    value encodes the first failing shape). 48 columns at 2^25..2^27 -- padded work buffer plus groups -- is the case that was
    wrong: the group strides were built from the caller's element stride on the work buffer's side."""
    lib = _lib()
    assert lib.lane_plan_check(1, 27) == 0


def _route(lib, point_bytes, logn, tot, inverse=False, coset=False, forced_r=0, budget=0, gtab_mode=-1):
    out = (ctypes.c_int * 70)()
    lib.ecntt_route_probe.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint64, ctypes.c_int,
                                      ctypes.POINTER(ctypes.c_int)]
    assert lib.ecntt_route_probe(point_bytes, logn, tot, int(inverse), int(coset), forced_r, budget, gtab_mode, out) == 0
    nst = out[0]
    return dict(nst=nst, rmax=out[1], stage_gtab=out[2], scale_runs=out[3], scale_gtab=out[4], budget=out[5], widths=list(out[6:6 + nst]))


def test_ecntt_route_on_each_side_of_every_boundary():
    """ntt_plan.h ecntt_route, the one place where ecntt_run decides its kernels. The expectations are the rules themselves, written out:
    budget 16384 quads below 2^14 points and 32768 from there; radix 2 (rmax == 1) when tot * 3 / 2 -- in integers -- exceeds the budget;
    a scale pass on an inverse or coset call, its tables in global memory when tot > 20480 (108-byte points) / 12288 (168-byte points);
    the radix-2 stage tables in global memory when tot / 2 -- in integers -- exceeds the same figure. (tot = 10923 is odd: its tot * 3 / 2
    is 16384 in integers, so the radix-2 band starts at 10924; an odd tot is a batch of one-point transforms, which have no stage.)"""
    lib = _lib()
    logn = 4  # the 16-point transforms of tests/test_gpu_ecntt_routes.py; the rules read tot only
    for pb in (108, 168):
        lds = 20480 if pb == 108 else 12288
        for tot, budget, radix2 in ((10922, 16384, False), (10923, 16384, False), (10924, 16384, True), (16383, 16384, True), (16384, 32768, False),
                                    (21845, 32768, False), (21846, 32768, True), (592, 16384, False), (11216, 16384, True), (32816, 32768, True), (40976, 32768, True)):
            r = _route(lib, pb, logn, tot)
            assert r["budget"] == budget and (r["rmax"] == 1) == radix2, (pb, tot, r)
            assert sum(r["widths"]) == logn and r["widths"][0] == r["rmax"] and r["nst"] == len(r["widths"])
            if radix2:
                assert r["widths"] == [1, 1, 1, 1]
            else:  # the widest stage whose tot (2^r - 1) / 2 products stay within the budget, at most the whole transform
                exp = max(w for w in range(1, 5) if w == 1 or tot * (2 ** w - 1) // 2 <= budget)
                assert r["rmax"] == exp, (pb, tot, r)
            assert r["stage_gtab"] == int(radix2 and tot // 2 > lds) and r["scale_runs"] == 0 and r["scale_gtab"] == 0
        assert _route(lib, pb, logn, 592)["widths"] == [4]
        # scale tables: tot against 12288 / 20480, only on a call that scales at all
        for tot in (12288, 12289, 20480, 20481):
            for inverse, coset in ((False, False), (True, False), (False, True), (True, True)):
                r = _route(lib, pb, logn, tot, inverse, coset)
                assert r["scale_runs"] == int(inverse or coset) and r["scale_gtab"] == int((inverse or coset) and tot > lds), (pb, tot, inverse, coset, r)
        # stage tables: tot / 2 against the same figures; all of these are radix 2 (tot >= 21846)
        for tot in (24576, 24577, 24578, 40960, 40961, 40962):
            r = _route(lib, pb, logn, tot, True, True)
            want = {168: tot >= 24578, 108: tot >= 40962}[pb]
            assert r["rmax"] == 1 and r["stage_gtab"] == int(want) and r["scale_gtab"] == 1, (pb, tot, r)
    assert _route(lib, 108, logn, 24578)["stage_gtab"] == 0 and _route(lib, 168, logn, 24576)["stage_gtab"] == 0
    # the three overrides: a forced radix, a forced budget, forced table placement (which applies to the radix-2 stages only)
    assert _route(lib, 168, 7, 128, forced_r=1) == dict(nst=7, rmax=1, stage_gtab=0, scale_runs=0, scale_gtab=0, budget=16384, widths=[1] * 7)
    assert _route(lib, 168, 7, 128, forced_r=1, gtab_mode=1)["stage_gtab"] == 1
    assert _route(lib, 168, 4, 32816, gtab_mode=0)["stage_gtab"] == 0
    assert _route(lib, 168, 7, 128, forced_r=2, gtab_mode=1) == dict(nst=4, rmax=2, stage_gtab=0, scale_runs=0, scale_gtab=0, budget=16384, widths=[2, 2, 2, 1])
    assert _route(lib, 168, 9, 1024, forced_r=2)["widths"] == [2, 2, 2, 2, 1]
    assert _route(lib, 108, 9, 512, forced_r=4)["widths"] == [3, 3, 3] and _route(lib, 108, 7, 128, forced_r=4)["widths"] == [4, 3]
    r = _route(lib, 108, 4, 592, budget=64)
    assert r["budget"] == 64 and r["rmax"] == 1 and r["stage_gtab"] == 0
    assert _route(lib, 108, 0, 5, True, False) == dict(nst=0, rmax=1, stage_gtab=0, scale_runs=1, scale_gtab=0, budget=16384, widths=[])
