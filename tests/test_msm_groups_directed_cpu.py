"""CPU: what tests/test_gpu_msm_groups_directed.py claims about its inputs, from the project's own code and a model of it.

The launch decisions come from msm_plan.h through tests/plan_harness.cpp (msm_plan_seg_probe, msm_reduce_probe): for every shape of the GPU
module the chunk kernel, the window kernel, the direct store, lw_log, wthreads, mrow and nseg are asserted here, with rwl and quad_ok derived
from the group's point size (tests/msm_directed.py Group). The bucket contents come from a Python model of the signed recoding (msm_directed.recode:
DigitIter, WinWidths, negate-if-top-bit in msm_impl.hpp): every overflow launch has exactly the intended bucket sizes and the intended largest
number of overflow segments, the heavy values touch no window but 0, and "top bucket only" fills the last bucket of its windows.
The three thresholds of k_fold_overflow are device code (msm_impl.hpp k_fold_overflow: "G = mx <= 2 ? 1u : (mx <= 32 ? 4u : (mx <= 256 ? 16u : 64u))");
msm_directed.fold_width restates them and the launches sit on both sides of each."""
import ctypes

import numpy as np
import pytest

from tests import msm_directed as D
from tests.test_plan import _lib, _reduce


def _plan(lib, n, bits, c=0, batch=1, pf=1, bitsize=0, windows=0):
    out = (ctypes.c_int * 7)()
    assert lib.msm_plan_seg_probe(n, bits, c, batch, pf, bitsize, windows, out) == 0
    return dict(zip(("c", "nwin", "wpf", "nb", "n_lo", "negate", "seg"), out))


def _seg(n, nb):
    """msm_plan.h make_plan: the power of two from 64 up that holds twice the average bucket"""
    seg = 64
    while seg * nb < 2 * n:
        seg *= 2
    return seg


def _widths(p):
    return [p["c"] - 1 if w < p["n_lo"] else p["c"] for w in range(p["nwin"])]


def test_point_sizes_give_the_window_block_and_the_four_lane_switch():
    got = {g.id: (g.proj_bytes, g.xyzz_bytes, g.rwl, g.quad_ok, g.bits) for g in (D.ModelGroup(*x) for x in D.GROUPS)}
    assert got == {"bn254": (108, 144, 256, True, 254), "grumpkin": (108, 144, 256, True, 254), "bls12_381": (168, 224, 256, True, 255),
                   "bls12_377": (168, 224, 256, True, 253), "bn254_g2": (216, 288, 256, True, 254), "bls12_381_g2": (336, 448, 128, False, 255),
                   "bls12_377_g2": (336, 448, 128, False, 253)}


def test_recoding_model_gives_back_the_scalar():
    """sum d_w 2^offset_w == s for a uniform plan (the spare bits of the top window take the last carry), == +-s' with s' = s or r - s for a
    mixed plan; no digit beyond 2^(w - 1) in size"""
    rng = np.random.default_rng(5)
    for g in (D.ModelGroup("bls12_377", False), D.ModelGroup("bn254", False), D.ModelGroup("bls12_381", False)):
        vals = D.rand_scalars(rng, 200, g.r) + [0, 1, g.r - 1, (1 << (g.bits - 1)) - 1, 1 << (g.bits - 1)]
        plans = [D.uniform_widths(g.bits, c) for c in (5, 7, 8, 10, 13, 16, 18, 19)] + [D._plan_widths(g.bits, D.mixed_windows(g.bits, c)) for c in D.ONE_LANE_CS]
        for k, wins in enumerate(plans):
            mixed = k >= 8
            for s in vals:
                ds = D.recode(s, [w for _, w in wins], r=g.r, negate=mixed)
                assert all(abs(d) <= 1 << (w - 1) for d, (_, w) in zip(ds, wins))  # bucket |d| - 1 lies inside the window's buckets
                tot = sum(d << off for d, (off, _) in zip(ds, wins))
                assert tot == s or (mixed and s >> (g.bits - 1) and -tot == g.r - s), (g.id, k, s)


@pytest.mark.parametrize("bits", [253, 254, 255])
@pytest.mark.parametrize("variant", ["single", "second_of_two", "table_of_two"])
def test_overflow_launches_hold_the_intended_buckets(bits, variant):
    """section 1: c = 13, seg = 64 by make_plan for every launch size; the chosen buckets of window 0 have exactly the chosen sizes, nothing
    else overflows, so the largest number of overflow segments is the table's mx and k_fold_overflow folds with the table's G lanes"""
    lib = _lib()
    g = D.ModelGroup({253: "bls12_377", 254: "bn254", 255: "bls12_381"}[bits], False)
    batch, pf = (2, 1) if variant == "second_of_two" else (1, 2) if variant == "table_of_two" else (1, 1)
    for name, (sizes_of, mx, G) in D.OVERFLOW_LAUNCHES.items():
        if variant != "single" and name != 2:
            continue
        seg = 64
        vals, bases = D.in_overflow(g.r, g.bases_fn, g.neg_rows, seg, sizes_of(seg))
        n = len(vals)
        p = _plan(lib, n, bits, c=D.OVERFLOW_C, batch=batch, pf=pf)
        nwin = (bits + 1 + 12) // 13
        assert n <= 1 << 15 and p == dict(c=13, nwin=nwin, wpf=(nwin + pf - 1) // pf, nb=4096, n_lo=0, negate=0, seg=seg), (name, n, p)
        cnt = D.bucket_counts(vals, _widths(p), wpf=p["wpf"])
        sizes = sizes_of(seg)
        assert {b + 1: m for (w, b), m in cnt.items() if w == 0 and b + 1 in sizes} == sizes
        assert all(m <= seg for (w, b), m in cnt.items() if not (w == 0 and b + 1 in sizes))  # nothing else overflows
        assert all(D.recode(v, _widths(p))[1:] == [0] * (p["nwin"] - 1) for v in sizes)         # the heavy values: window 0 only
        extras = [(m + seg - 1) // seg - 1 for m in sizes.values()]
        assert max(extras) == mx and D.fold_width(mx) == G, (name, extras)
        assert int((~bases.any(axis=1)).sum()) >= 3 and len(bases) == n  # zero rows
    # the thresholds themselves: 2 | 3, 32 | 33, 256 | 257
    assert [D.fold_width(m) for m in (1, 2, 3, 32, 33, 256, 257, 5000)] == [1, 1, 4, 4, 16, 16, 64, 64]
    assert sorted(mx for _, mx, _ in D.OVERFLOW_LAUNCHES.values()) == [2, 32, 33, 256, 257]


@pytest.mark.parametrize("cname,g2", D.NEVER_ONE_LANE, ids=[D.gid(*g) for g in D.NEVER_ONE_LANE])
def test_directed_patterns_take_the_one_lane_reduction(cname, g2):
    """section 2: k_reduce_wave (+ k_reduce_window from 13-bit windows up) for BLS G2 on uniform plans, for every group on forced mixed plans
    and as a batch of two"""
    lib = _lib()
    g = D.ModelGroup(cname, g2)
    want = {8: (128, 2, 1), 13: (4096, 16, 4), 16: (32768, 8, 64)}  # c: nb, mrow, nseg of a single MSM
    for c in D.ONE_LANE_CS:
        nb, mrow, nseg = want[c]
        nw = (g.bits + 1 + c - 1) // c
        for n in ((1 << 10) + 1, 1 << 10, 1 << 12, (1 << 11) + 7):
            assert _plan(lib, n, g.bits, c=c) == dict(c=c, nwin=nw, wpf=nw, nb=nb, n_lo=0, negate=0, seg=64), (c, n)
        if not g.quad_ok:  # uniform single MSMs: the production route of BLS G2
            r = _reduce(lib, nb, nw, rwl=g.rwl, quad_ok=False)
            assert (r["chunk"], r["mrow"], r["nseg"], r["nblocks"]) == ("k_reduce_wave", mrow, nseg, nw * nseg), (c, r)
            assert (r["window"], r["direct"], r["wthreads"]) == ((None, 1, 0) if c == 8 else ("k_reduce_window", 0, 64)), (c, r)
        # forced mixed plans: W windows of c - 1 and c bits; the narrow ones use half the buckets. No four-lane kernel for any group.
        W = D.mixed_windows(g.bits, c)
        p = _plan(lib, 1 << 12, g.bits, windows=W)
        x = g.bits - (c - 1) * W
        assert p == dict(c=c, nwin=W, wpf=W, nb=nb, n_lo=W - x, negate=1, seg=_seg(1 << 12, nb // 2)) and 0 < x < W, (c, p)  # (seg: from the narrow windows)
        assert [w for _, w in D._plan_widths(g.bits, W)] == _widths(p)
        r = _reduce(lib, nb, W, rwl=g.rwl, n_lo=p["n_lo"], quad_ok=g.quad_ok)
        assert (r["chunk"], r["nlo_w"], r["cost_q"]) == ("k_reduce_wave", W - x, 0), (c, r)
        assert r["nblocks"] == (W - x) * r["nseg_lo"] + x * r["nseg"] and r["nseg_lo"] == max(1, r["nseg"] // 2)
        assert (r["window"], r["direct"]) == ((None, 1) if c == 8 else ("k_reduce_window", 0)) and (r["mrow"], r["nseg"]) == (mrow, nseg), (c, r)
        if c in D.BATCH_CS and g.quad_ok:  # a batch of two: twice the windows in one launch, 16 rows per lane
            r = _reduce(lib, nb, 2 * nw, wpf=nw, batch=2, bb=2, rwl=g.rwl, quad_ok=True)
            assert (r["chunk"], r["window"], r["mrow"], r["nseg"], r["wthreads"]) == ("k_reduce_wave", "k_reduce_window", 16, nb // 1024, 64), (c, r)
    # bls12_381 G1 with hip_msm_windows = 21: 18 windows of 12 bits below 3 of 13
    if g.bits == 255:
        assert _plan(lib, 4096, 255, windows=21)["n_lo"] == 18


@pytest.mark.parametrize("bits", [253, 254, 255])
def test_top_bucket_only_fills_the_last_bucket(bits):
    """every second window below the top one holds all the terms of one parity in its LAST bucket (digit 2^(w - 1)): bucket nb - 1 of a wide
    window, nb / 2 - 1 of a narrow one; nothing anywhere else"""
    g = D.ModelGroup({253: "bls12_377", 254: "bn254", 255: "bls12_381"}[bits], False)
    plans = [(D.uniform_widths(bits, c), False) for c in (5, 7, 8, 10, 13, 16, 18, 19)] + [(D._plan_widths(bits, D.mixed_windows(bits, c)), True) for c in D.ONE_LANE_CS]
    for wins, mixed in plans:
        vals, _ = D.in_top_bucket_only(g.r, g.bases_fn, wins)
        cnt = D.bucket_counts(vals, [w for _, w in wins], r=g.r, negate=mixed)
        filled = [k for k, (off, w) in enumerate(wins) if off + w < bits]
        assert len(filled) >= len(wins) - 2 and cnt == {(k, (1 << (wins[k][1] - 1)) - 1): len(vals) // 2 for k in filled}, (bits, wins[0], mixed)
        nb = 1 << (max(w for _, w in wins) - 1)
        # (253 bits on a mixed plan of 7- or 12-bit windows: the one wide window is the top one, which the input leaves empty)
        assert any(b == nb - 1 for _, b in cnt) == any(wins[k][1] == max(w for _, w in wins) for k in filled)
        assert mixed or (len(wins) - 2, nb - 1) in cnt or (len(wins) - 3, nb - 1) in cnt


@pytest.mark.parametrize("cname,g2", D.SMALL_GROUPS, ids=[D.gid(*g) for g in D.SMALL_GROUPS])
def test_small_windows_take_k_reduce_small_at_every_lane_width(cname, g2):
    """section 3: batch * wpf >= 64 whole windows of 16 .. 512 buckets: k_reduce_small with 4, 8, 16, 32 lanes per window, writing the window
    sums itself; which shapes leave the last wave partly empty"""
    lib = _lib()
    g = D.ModelGroup(cname, g2)
    partly = []
    for c, batch, bitsize in D.SMALL_SHAPES:
        for n in (300, 700, 1024):
            p = _plan(lib, n, g.bits, c=c, batch=batch, bitsize=bitsize)
            nwin = ((bitsize or g.bits) + 1 + c - 1) // c
            assert p == dict(c=c, nwin=nwin, wpf=nwin, nb=1 << (c - 1), n_lo=0, negate=0, seg=_seg(n, 1 << (c - 1))), (c, n, p)
        nw = batch * p["wpf"]
        r = _reduce(lib, p["nb"], nw, wpf=p["wpf"], batch=batch, bb=batch, rwl=g.rwl, quad_ok=g.quad_ok)
        assert nw >= 64 and (r["chunk"], r["window"], r["direct"], r["nseg"]) == ("k_reduce_small", None, 1, 1), (c, r)
        assert (r["lw_log"], r["per_wave"]) == (D.SMALL_LW_LOG[c], 64 >> D.SMALL_LW_LOG[c]) and p["nb"] >> r["lw_log"] in (4, 8, 16), (c, r)
        if nw % r["per_wave"]:
            partly.append((c, batch, bitsize))
    assert partly == [(5, 2, 0), (7, 2, 0), (8, 3, 247), (10, 3, 240)]
    assert sorted({D.SMALL_LW_LOG[c] for c, _, _ in partly}) == [2, 3, 4, 5]


def test_the_window_kernel_runs_all_128_lanes():
    """section 4: bls12_381 G2 (rwl = 128), 1024 terms, c = 18 / 19: 128 chunks of 16 / 32 rows per lane, k_reduce_window with 128 threads"""
    lib = _lib()
    g = D.ModelGroup(*D.FULL_WINDOW_GROUP)
    assert (g.rwl, g.quad_ok) == (128, False)
    for c, nwin, mrow in ((18, 15, 16), (19, 14, 32)):
        p = _plan(lib, 1024, g.bits, c=c)
        assert p == dict(c=c, nwin=nwin, wpf=nwin, nb=1 << (c - 1), n_lo=0, negate=0, seg=64), (c, p)
        r = _reduce(lib, p["nb"], nwin, rwl=g.rwl, quad_ok=g.quad_ok)
        assert (r["chunk"], r["window"], r["direct"], r["mrow"], r["nseg"], r["wthreads"], r["nblocks"]) == ("k_reduce_wave", "k_reduce_window", 0, mrow, 128, 128, nwin * 128), (c, r)
        assert 64 * r["mrow"] * r["nseg"] == p["nb"] and p["nb"] * nwin * g.proj_bytes < 1.3 * (1 << 30)
        # the block size is the group's: a group with 256 window lanes would run the same window as 128 / 256 chunks of 16 rows
        assert _reduce(lib, p["nb"], nwin, rwl=256, quad_ok=False)["mrow"] == 16
