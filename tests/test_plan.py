"""CPU: the NTT pass decomposition (icicle_amd/csrc/ntt_plan.h) compiled for the host -- every pass covers a row exactly
once and the last pass's scatter is a permutation, for every size up to 2^27 (31-bit fields, 256-bit fields, goldilocks), the latter two
with the tile width and block size ntt_big.hip launches with (big_pass_geometry: LDS bytes, blockDim % T, whole stage groups, up to 2^28); the
lane-native launch geometry of interleaved transforms (ntt_plan.h fast_pass_geometry, what ntt_run launches) maps every
logical element to the same word with and without column / outer-index groups."""
import ctypes
import itertools
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def _lib():
    so = os.path.join(HERE, "_build", "libplan.so")
    os.makedirs(os.path.dirname(so), exist_ok=True)
    src = os.path.join(HERE, "plan_harness.cpp")
    hdrs = [os.path.join(HERE, "..", "icicle_amd", "csrc", h) for h in ("ntt_plan.h", "msm_plan.h")]
    if not os.path.exists(so) or max([os.path.getmtime(src)] + [os.path.getmtime(h) for h in hdrs]) > os.path.getmtime(so):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-pthread", src, "-o", so])
    return ctypes.CDLL(so)


def test_ntt_plan_covers_every_slot_once():
    lib = _lib()
    assert lib.plan_check(27, 28) == 0
    # the geometry ntt_big.hip launches with (ntt_plan.h big_pass_geometry), at the sizes where a pass gains rows: (rows, T, threads, LDS bytes)
    # per pass. 2^25: the first 512-row pass, for a 256-bit field exactly the 72 KiB bound with 512 threads; 2^28: 1024 rows, the tile halves.
    for logn, elem, tcap, r16, want in ((24, 36, 4, 0, [(8, 4, 256, 36864)] * 3), (25, 36, 4, 0, [(9, 4, 512, 73728), (8, 4, 256, 36864), (8, 4, 256, 36864)]),
                                        (27, 36, 4, 0, [(9, 4, 512, 73728)] * 3), (28, 36, 4, 0, [(10, 2, 512, 73728), (9, 4, 512, 73728), (9, 4, 512, 73728)]),
                                        (25, 8, 16, 1, [(9, 16, 512, 65536), (8, 16, 256, 32768), (8, 16, 256, 32768)]),
                                        (28, 8, 16, 1, [(10, 8, 512, 65536), (9, 16, 512, 65536), (9, 16, 512, 65536)]), (3, 8, 16, 1, [(3, 1, 64, 64)])):
        out = (ctypes.c_int * 6)()
        got = []
        for p in range(len(want)):
            assert lib.big_pass_probe(logn, p, elem, tcap, r16, out) == len(want)
            assert out[3] == (1 << out[0]) * out[1] and out[2] * out[3] == 1 << logn
            got.append((out[0], out[1], out[4], out[5]))
        assert got == want, (logn, elem, got)
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


# ---- the MSM's launch decisions (msm_plan.h), probed through tests/plan_harness.cpp ----
_KNOB_ORDER = ("hb_set", "hb", "mrow_set", "mrow", "acc_waves_set", "acc_waves", "reduce_balance", "reduce_small", "reduce_quad", "host_combine", "batch_horner")


def _knobs(hb=None, mrow=None, acc_waves=None, reduce_balance=0, reduce_small=1, reduce_quad=1, host_combine=1, batch_horner=1):
    """MsmKnobs as the probes read them; None = the variable is not set."""
    v = dict(hb_set=int(hb is not None), hb=hb or 0, mrow_set=int(mrow is not None), mrow=mrow or 0, acc_waves_set=int(acc_waves is not None),
             acc_waves=acc_waves or 0, reduce_balance=reduce_balance, reduce_small=reduce_small, reduce_quad=reduce_quad, host_combine=host_combine,
             batch_horner=batch_horner)
    return (ctypes.c_int * len(_KNOB_ORDER))(*[v[k] for k in _KNOB_ORDER])


def _sort(lib, n, c, pf=1, **kn):
    out = (ctypes.c_int * 5)()
    if not lib.msm_sort_probe(n, c, pf, _knobs(**kn), out):
        return None
    return dict(hb=out[0], lb=out[1], jb=out[2], chunk_log=out[3], nblk=out[4])


_CHUNK = {0: None, 1: "k_reduce_wave_quad", 2: "k_reduce_small", 3: "k_reduce_wave"}
_WINDOW = {0: None, 1: "k_reduce_window_quad", 2: "k_reduce_window"}


def _reduce(lib, nb, nw, wpf=None, batch=1, rwl=256, w0=0, n_lo=0, seg_lo=-1, nsegr=-1, hook=False, NG=1, bb=1, quad_ok=True, **kn):
    out = (ctypes.c_int * 21)()
    assert lib.msm_reduce_probe(batch, wpf if wpf is not None else nw, nb, rwl, w0, nw, n_lo, seg_lo, nsegr, int(hook), NG, bb, int(quad_ok), _knobs(**kn), out) == 0
    names = ("mrow", "m", "nseg", "log_chunk", "chunk", "window", "direct", "nlo_w", "nsq", "mq", "lw_log", "per_wave", "nblocks", "mrow_lo", "nseg_lo",
             "log_chunk_lo", "wchunks", "wchunk_size", "wthreads", "cost_q", "cost_s")
    r = dict(zip(names, out))
    r["chunk"], r["window"] = _CHUNK[r["chunk"]], _WINDOW[r["window"]]
    return r


def test_msm_sort_plan():
    """msm_plan.h msm_sort_plan: one level up to c = 11 (pass A sorts by the whole key), then hb = ceil((c - 1) / 2) high bits, at most 10, the
    rest -- at most 11 -- low bits; pass-A chunks of 2^17 scalars, larger when that would take more than 512 blocks, never so large that
    index, low key bits and precompute index overflow 31 bits. ICICLE_HIP_MSM_HB is clamped into [kb - 11, min(kb, 10)], kb = c - 1."""
    lib = _lib()
    for c in range(2, 12):
        assert _sort(lib, 1 << 16, c) == dict(hb=c - 1, lb=0, jb=0, chunk_log=17, nblk=1), c
    for c, hb, lb in ((12, 6, 5), (16, 8, 7), (20, 10, 9), (22, 10, 11)):
        s = _sort(lib, 1 << 20, c)
        assert (s["hb"], s["lb"]) == (hb, lb) and s["hb"] + s["lb"] == c - 1, (c, s)
    assert _sort(lib, 1 << 26, 20) == dict(hb=10, lb=9, jb=0, chunk_log=17, nblk=512)
    assert _sort(lib, 1 << 27, 20) == dict(hb=10, lb=9, jb=0, chunk_log=18, nblk=512)  # more scalars: larger chunks, still 512 blocks
    assert _sort(lib, 5000, 13) == dict(hb=6, lb=6, jb=0, chunk_log=17, nblk=1)
    assert _sort(lib, (1 << 17) + 1, 13)["nblk"] == 2
    assert _sort(lib, 1 << 14, 15, pf=2)["jb"] == 1 and _sort(lib, 1 << 14, 15, pf=5)["jb"] == 3
    for c in (5, 12, 16, 22):
        kb = c - 1
        for hb in (-40, 0, 3, 4, 7, 10, 11, 40):
            want = max(kb - 11, min(min(kb, 10), hb))
            s = _sort(lib, 1 << 20, c, hb=hb)
            assert (s is None) == (want < 0), (c, hb, s)
            if s is not None:
                assert (s["hb"], s["lb"]) == (want, kb - want), (c, hb, s)
    # max_chunk = 31 - lb - jb below 10: c = 22 (lb = 11) on a table of 2048 precomputed multiples
    assert _sort(lib, 1 << 10, 22, pf=1024) == dict(hb=10, lb=11, jb=10, chunk_log=10, nblk=1)
    assert _sort(lib, 1 << 10, 22, pf=2048) is None
    # more than 512 pass-A blocks: chunk_log is capped at max_chunk
    assert _sort(lib, 1 << 19, 22, pf=1024) == dict(hb=10, lb=11, jb=10, chunk_log=10, nblk=512)
    assert _sort(lib, (1 << 19) + 1, 22, pf=1024) is None
    assert _sort(lib, 1 << 29, 22) == dict(hb=10, lb=11, jb=0, chunk_log=20, nblk=512)
    assert _sort(lib, 1 << 30, 22) is None


def test_msm_reduce_geometry():
    """msm_plan.h msm_reduce_geom: mrow = max(1, nb / (64 rwl), min(cap, nb / 64)) rows per lane; cap 16, but for a single MSM with windows of
    8192 buckets and more the power of two (>= 2) at which wpf * nb / (64 mrow) waves still fill 1024 SIMDs once; ICICLE_HIP_MSM_MROW
    replaces the cap. m = 64 mrow buckets per chunk, nseg = max(1, nb / m) chunks per window."""
    lib = _lib()

    def geom(nb, wpf, **kw):
        r = _reduce(lib, nb, wpf, wpf=wpf, **kw)
        assert r["m"] == 64 * r["mrow"] and r["nseg"] == max(1, nb // r["m"]) and (1 << r["log_chunk"]) == r["m"]
        return r["mrow"], r["nseg"]

    assert geom(16384, 17) == (8, 32) and 17 * 32 == 544  # 2^16, c = 15
    assert geom(65536, 15) == (16, 64)                     # 2^20, c = 17
    assert geom(8192, 17) == (4, 32) and geom(8192, 2) == (2, 64)
    assert geom(4096, 17) == (16, 4)                       # below 8192 buckets: cap 16
    assert geom(16384, 17, batch=2) == (16, 16)            # a batch: cap 16
    for nb in (1, 2, 32):
        assert geom(nb, 32) == (1, 1)
    assert geom(64, 32) == (1, 1) and geom(128, 32) == (2, 1) and geom(1024, 32) == (16, 1) and geom(2048, 32) == (16, 2)
    assert geom(1 << 21, 12) == (128, 256) and geom(1 << 21, 12, rwl=128) == (256, 128)  # at most rwl chunks per window
    assert geom(16384, 17, mrow=4) == (4, 64) and geom(16384, 17, mrow=32) == (32, 8) and geom(32, 17, mrow=4) == (1, 1)


def test_msm_reduce_route_on_each_side_of_every_switch():
    """msm_plan.h msm_reduce_route, the one place where the bucket reduction of a window group picks its kernels. The expectations are the
    rules: k_reduce_small for whole windows of 16..512 buckets, 64 and more of them; the four-lane kernels for one group of one MSM on a
    uniform plan on one device, the wave kernel when (2 mq + 13) * 13 * rounds < (2 mrow + 19) * 29 * rounds and nb <= 65536, the window
    kernel when a window has at most 64 chunks; else k_reduce_wave and k_reduce_window."""
    lib = _lib()
    # 2^16 terms, c = 15 -- the "57 chunks of 288 buckets" of tests/test_gpu_msm.py
    r = _reduce(lib, 16384, 17)
    assert (r["mrow"], r["nseg"]) == (8, 32) and r["chunk"] == "k_reduce_wave_quad" and (r["mq"], r["nsq"]) == (18, 57) and 16 * 18 == 288
    assert (r["cost_q"], r["cost_s"]) == (637, 1015) and not r["direct"]
    assert (r["window"], r["wchunks"], r["wchunk_size"], r["wthreads"]) == ("k_reduce_window_quad", 57, 288, 256)
    # 2^20 terms, c = 17: the one-lane wave kernel wins, the window kernel stays four-lane
    r = _reduce(lib, 65536, 15)
    assert (r["mrow"], r["nseg"]) == (16, 64) and (r["cost_q"], r["cost_s"]) == (1833, 1479)
    assert r["chunk"] == "k_reduce_wave" and r["nblocks"] == 960 and not r["direct"]
    assert (r["window"], r["wchunks"], r["wchunk_size"], r["wthreads"]) == ("k_reduce_window_quad", 64, 1024, 256)
    # beyond: more than 65536 buckets, more than 64 chunks
    for nb, rwl in ((1 << 17, 256), (1 << 17, 128), (1 << 19, 256), (1 << 21, 256), (1 << 21, 128)):
        r = _reduce(lib, nb, 13, rwl=rwl)
        assert r["cost_q"] == 0 and r["chunk"] == "k_reduce_wave" and r["nblocks"] == 13 * r["nseg"] and r["window"] == "k_reduce_window", (nb, r)
        assert r["nseg"] > 64 and r["wthreads"] == min(rwl, 1 << (r["nseg"] - 1).bit_length()), (nb, rwl, r)
    for nsegr, threads in ((1, 64), (64, 64), (65, 128), (128, 128), (129, 256), (200, 256)):  # a hook's slice of 256 chunks
        r = _reduce(lib, 1 << 21, 12, hook=True, seg_lo=3, nsegr=nsegr)
        assert (r["chunk"], r["window"], r["wthreads"], r["nblocks"]) == ("k_reduce_wave", "k_reduce_window", threads, 12 * nsegr), (nsegr, r)
    # each of these alone switches the four-lane route off
    for off in (dict(hook=True), dict(NG=2), dict(bb=2), dict(n_lo=5), dict(seg_lo=1), dict(nsegr=31), dict(quad_ok=False), dict(reduce_quad=0)):
        r = _reduce(lib, 16384, 17, **off)
        assert (r["chunk"], r["window"], r["wthreads"], r["cost_q"], r["cost_s"]) == ("k_reduce_wave", "k_reduce_window", 64, 0, 0), (off, r)
        assert r["nblocks"] == (17 * 31 if "nsegr" in off else 5 * 16 + 12 * 32 if "n_lo" in off else 17 * 32), (off, r)
    # batches of small windows
    for nb, lw_log in ((16, 2), (32, 2), (64, 3), (128, 4), (256, 5), (512, 5)):
        for bb in (1, 8):
            r = _reduce(lib, nb, 64, wpf=64 // bb, batch=bb, bb=bb)
            assert r["nseg"] == 1 and (r["chunk"], r["window"], r["direct"], r["lw_log"], r["per_wave"]) == ("k_reduce_small", None, 1, lw_log, 64 >> lw_log), (nb, r)
    for nb, nw in ((16, 63), (512, 63), (8, 64), (1024, 64)):
        for bb in (1, 8):
            r = _reduce(lib, nb, nw, batch=bb, bb=bb)
            assert r["nseg"] == 1 and r["chunk"] in ("k_reduce_wave", "k_reduce_wave_quad") and (r["chunk"] == "k_reduce_wave_quad") == (bb == 1 and nb >= 16), (nb, nw, r)
    assert _reduce(lib, 512, 64, n_lo=3)["chunk"] == "k_reduce_wave" and _reduce(lib, 512, 64, hook=True, nsegr=1, seg_lo=1)["chunk"] == "k_reduce_wave"
    # ICICLE_HIP_MSM_REDUCE_SMALL=0: the four-lane route where its conditions hold, else the one-lane kernel writing the window sums
    r = _reduce(lib, 512, 64, reduce_small=0)
    assert (r["chunk"], r["nsq"], r["mq"], r["window"], r["wchunks"], r["wchunk_size"], r["wthreads"]) == ("k_reduce_wave_quad", 16, 2, "k_reduce_window_quad", 16, 32, 64)
    assert (r["cost_q"], r["cost_s"]) == ((2 * 2 + 13) * 13, (2 * 8 + 19) * 29)
    for kw in (dict(reduce_quad=0), dict(bb=8, batch=8)):
        r = _reduce(lib, 512, 64, reduce_small=0, **kw)
        assert (r["chunk"], r["window"], r["direct"], r["nblocks"]) == ("k_reduce_wave", None, 1, 64), (kw, r)
    # one chunk per window, the whole window: the chunk kernel writes the window sums, no window kernel
    for nb in (1, 8, 1024):
        r = _reduce(lib, nb, 10, batch=4, bb=4)
        assert r["nseg"] == 1 and (r["chunk"], r["window"], r["direct"], r["nblocks"]) == ("k_reduce_wave", None, 1, 10), (nb, r)
    r = _reduce(lib, 16, 10)  # the four-lane wave kernel with one chunk per window does the same
    assert (r["chunk"], r["nsq"], r["mq"], r["direct"], r["window"]) == ("k_reduce_wave_quad", 1, 1, 1, None)
    r = _reduce(lib, 32, 10)
    assert (r["chunk"], r["nsq"], r["mq"], r["direct"], r["window"], r["wchunks"], r["wthreads"]) == ("k_reduce_wave_quad", 2, 1, 0, "k_reduce_window_quad", 2, 64)
    # mixed widths: windows below n_lo have half the buckets
    nb, n_lo, wpf = 1 << 21, 10, 12
    for w0, nw in ((0, 12), (8, 4), (10, 2), (0, 10), (4, 3)):
        for kw in (dict(), dict(reduce_balance=1), dict(reduce_balance=1, hook=True), dict(reduce_balance=1, mrow=1), dict(mrow=64)):
            r = _reduce(lib, nb, nw, wpf=wpf, w0=w0, n_lo=n_lo, **kw)
            nlo_w = min(max(n_lo, w0), w0 + nw) - w0
            halve = kw.get("reduce_balance") and nlo_w > 0 and r["mrow"] >= 2 and not kw.get("hook")
            mrow_lo = r["mrow"] // 2 if halve else r["mrow"]
            nseg_lo = max(1, (nb // 2) // (64 * mrow_lo))
            assert (r["nlo_w"], r["mrow_lo"], r["nseg_lo"], r["log_chunk_lo"]) == (nlo_w, mrow_lo, nseg_lo, r["log_chunk"] - int(bool(halve))), (w0, nw, kw, r)
            assert r["nblocks"] == nlo_w * nseg_lo + (nw - nlo_w) * r["nseg"] and r["chunk"] == "k_reduce_wave" and r["window"] == "k_reduce_window"
            assert r["wthreads"] == min(256, max(64, 1 << (max(r["nseg"], nseg_lo if nlo_w else 0) - 1).bit_length()))
    assert _reduce(lib, nb, 12, n_lo=10)["mrow_lo"] == 128 and _reduce(lib, nb, 12, n_lo=10, reduce_balance=1)["mrow_lo"] == 64


# the uniform single MSMs of tests/test_gpu_msm_quad_reduce.py: (scalar bits, c) -> (windows, buckets) by make_plan, and for c = 8, 13, 16 of a
# 254-bit scalar the two costs msm_reduce_route compares (four-lane against one-lane)
QUAD_REDUCE_SHAPES = {(254, 8): (32, 128), (254, 13): (20, 4096), (254, 16): (16, 32768), (255, 8): (32, 128), (255, 13): (20, 4096), (255, 16): (16, 32768)}
QUAD_REDUCE_COSTS = {8: (195, 667), 13: (325, 1479), 16: (1001, 1015)}


def test_directed_quad_reduce_shapes_take_the_four_lane_kernels():
    """tests/test_gpu_msm_quad_reduce.py must not drift onto the one-lane kernels unnoticed: every (scalar bits, c) it runs as a uniform single
    MSM of 2^10 .. 2^12 terms reduces its buckets with k_reduce_wave_quad and k_reduce_window_quad, for G1 and for the G2 with quad_ok
    (BN254's, c = 8 and 13). c = 16 sits next to the switch: 1001 against 1015."""
    lib = _lib()
    for (bits, c), (nw, nb) in QUAD_REDUCE_SHAPES.items():
        for n in ((1 << 10) + 1, 1 << 11, 1 << 12):
            out = (ctypes.c_int * 5)()
            assert lib.msm_plan_probe(n, bits, c, out) == 0
            assert tuple(out) == (c, nw, nw, nb, 0), (bits, c, n, tuple(out))  # uniform: no narrow windows, no base table
        r = _reduce(lib, nb, nw)
        assert r["chunk"] == "k_reduce_wave_quad" and r["window"] == "k_reduce_window_quad" and not r["direct"], (bits, c, r)
        assert (r["cost_q"], r["cost_s"]) == QUAD_REDUCE_COSTS[c] and r["cost_q"] < r["cost_s"], (bits, c, r)
        assert r["wchunks"] == r["nsq"] > 1 and r["wchunk_size"] == 16 * r["mq"] and r["nsq"] * 16 * r["mq"] >= nb, (bits, c, r)
        # the knob of the one-lane tests really is what keeps them off these kernels
        off = _reduce(lib, nb, nw, reduce_quad=0)
        assert off["chunk"] == "k_reduce_wave" and off["window"] in (None, "k_reduce_window"), (bits, c, off)
    # a G2 curve without quad_ok (BLS12-381's, BLS12-377's) never takes them
    for nw, nb in set(QUAD_REDUCE_SHAPES.values()):
        r = _reduce(lib, nb, nw, quad_ok=False)
        assert r["chunk"] == "k_reduce_wave" and r["window"] != "k_reduce_window_quad", (nb, nw, r)


def test_msm_combine_route_and_accumulate_waves():
    """msm_plan.h msm_combine_route: the host Horner combine exactly for a single MSM without a hook whose result goes to the host or whose
    call is synchronous, with at most 64 windows; else k_final_horner for 64 and more MSMs of two and more windows; else k_final, followed by
    k_final_combine when an MSM has more than 16 windows. msm_acc_waves: the k_accumulate instantiation per curve class."""
    lib = _lib()
    names = {0: "host", 1: "k_final_horner", 2: "k_final", 3: "k_final+k_final_combine"}
    for on_dev, is_async, (batch, bb), hook, wpf, hc, bh in itertools.product((0, 1), (0, 1), ((1, 1), (2, 1), (2, 2), (63, 63), (64, 64), (200, 100)), (0, 1),
                                                                            (1, 2, 16, 17, 64, 65), (0, 1), (0, 1)):
        got = names[lib.msm_combine_probe(on_dev, is_async, batch, bb, hook, wpf, _knobs(host_combine=hc, batch_horner=bh))]
        if hc and (not on_dev or not is_async) and batch == 1 and bb == 1 and not hook and wpf <= 64:
            want = "host"
        elif bh and bb >= 64 and wpf >= 2:
            want = "k_final_horner"
        else:
            want = "k_final+k_final_combine" if wpf > 16 else "k_final"
        assert got == want, (on_dev, is_async, batch, bb, hook, wpf, hc, bh)

    def acc(is_g2, xyzz, limbs, co_ok=False, **kn):
        out = (ctypes.c_int * 2)()
        assert lib.msm_acc_probe(int(is_g2), xyzz, limbs, int(co_ok), _knobs(**kn), out) == 0
        return out[0], bool(out[1])

    g1_9, g1_14, g2_288, g2_448 = (False, 144, 9), (False, 224, 14), (True, 288, 9), (True, 448, 14)  # BN254, BLS12-381; G1, G2
    assert acc(*g1_9) == (3, False) and acc(*g1_14) == (2, False) and acc(*g2_288) == (2, False) and acc(*g2_448) == (1, False)
    assert acc(*g1_9, co_ok=True) == (2, True) and acc(*g1_9, co_ok=True, acc_waves=4) == (2, True)
    for w in (-1, 0, 1, 2, 3, 4, 5, 8):
        assert acc(*g1_9, acc_waves=w) == acc(*g1_14, acc_waves=w) == (w if w in (1, 2, 4) else 3, False), w
        assert acc(*g2_288, acc_waves=w) == (2 if w >= 2 else 1, False) and acc(*g2_448, acc_waves=w) == (1, False), w

    # msm_batch_fold: c = 10 on 254-bit scalars -- 26 windows of 512 buckets, one sort level, one pass-A block
    lib.msm_fold_probe.argtypes = [ctypes.c_int] * 5 + [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    n, wpf, nbk, proj = 4096, 26, 512, 108
    per = wpf * n * 4 + wpf * n * 4 + wpf * nbk * (proj + 12) + wpf * 512 * 1 * 8

    def fold(batch, free, hook=False, staged=0):
        return lib.msm_fold_probe(n, 254, batch, 10, proj, staged, free, int(hook), _knobs())

    assert fold(128, 2 * 5 * per) == 5 and fold(128, 2 * 5 * per - 2) == 4 and fold(128, 0) == 1  # half of the free memory
    assert fold(128, 2 * 5 * (per + 1000), staged=1000) == 5
    assert fold(128, 1 << 62) == 128 and fold(4096, 1 << 62) == min(4096, (48 << 30) // per, 60000 // wpf) == 60000 // wpf
    assert fold(128, 0, hook=True) == 128 and fold(60000 // wpf, 0, hook=True) == 60000 // wpf and fold(60000 // wpf + 1, 0, hook=True) == 0
