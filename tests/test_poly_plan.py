"""CPU: the host-only planning of vecops_poly.hip (icicle_amd/csrc/poly_plan.h) through tests/poly_plan_harness.cpp, built with g++ as a
library for the directed checks below and, with -fsanitize=address,undefined, as a program of its own that walks the same functions.
The expectations are the rules of poly_plan.h written out: the route and chunks of poly_eval at its thresholds, the tile schedule of the
division, the geometry of the degree scan and every argument rule."""
import ctypes
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "poly_plan_harness.cpp")
HDR = os.path.join(HERE, "..", "icicle_amd", "csrc", "poly_plan.h")
OK, EMPTY, BAD_POINTER, BAD_ARGUMENT = 0, 1, 2, 3
P = 2013265921


def _stale(target):
    return not os.path.exists(target) or max(os.path.getmtime(SRC), os.path.getmtime(HDR)) > os.path.getmtime(target)


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(HERE, "_build", "libpoly_plan.so")
    os.makedirs(os.path.dirname(so), exist_ok=True)
    if _stale(so):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", SRC, "-o", so])
    lib = ctypes.CDLL(so)
    u64, i64, u64p, i64p = ctypes.c_uint64, ctypes.c_int64, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int64)
    lib.pp_eval_plan.argtypes = [u64, u64, ctypes.c_int, u64p]
    lib.pp_eval_levels.argtypes = [u64, u64, ctypes.c_int, u64p, ctypes.c_int]
    lib.pp_hnz_plan.argtypes = [u64, u64p]
    lib.pp_div_tiles.argtypes = [i64, i64, i64]
    lib.pp_div_tiles.restype = u64
    lib.pp_div_tile.argtypes = [i64, i64, i64, i64, i64p]
    lib.pp_slice_check.argtypes = [ctypes.c_int, u64, ctypes.c_int, u64, ctypes.c_int, u64, u64, u64, u64, u64, u64]
    lib.pp_hnz_check.argtypes = [ctypes.c_int, u64, u64, u64]
    lib.pp_eval_check.argtypes = [ctypes.c_int, u64, u64, u64, u64, u64, ctypes.c_int]
    lib.pp_division_check.argtypes = [ctypes.c_int, u64, u64, u64, u64, u64, i64]
    lib.pp_degree_check.argtypes = [i64, i64, u64, u64]
    lib.pp_overlap.argtypes = [u64, u64, ctypes.c_int, u64, u64, ctypes.c_int]
    lib.pp_div_simulate.argtypes = [u64p, i64, u64p, i64, i64]
    return lib


def eval_plan(lib, n, pairs, key=0):
    out = (ctypes.c_uint64 * 3)()
    lib.pp_eval_plan(n, pairs, key, out)
    return bool(out[0]), out[1], out[2]


def eval_levels(lib, n, pairs, key=0):
    out = (ctypes.c_uint64 * 80)()
    k = lib.pp_eval_levels(n, pairs, key, out, 40)
    assert k >= 0
    return [(out[2 * i], out[2 * i + 1]) for i in range(k)]


def test_poly_eval_route_at_its_thresholds(lib):
    """point route: ceil(pairs / 64) >= 1024 waves, or at most 1024 coefficients; else the split route towards 4096 waves, chunks a multiple
    of 64 and at least 256; the second level (at most 4096 values) is one chunk"""
    big = 1 << 20
    # the pairs threshold: 1023 * 64 = 65472 pairs are 1023 waves
    assert eval_plan(lib, big, 65471)[0] and eval_plan(lib, big, 65472)[0] and not eval_plan(lib, big, 65473)[0]
    # the coefficient threshold
    assert not eval_plan(lib, 1023, 1)[0] and not eval_plan(lib, 1024, 1)[0] and eval_plan(lib, 1025, 1) == (True, 256, 5)
    # one point: 4096 chunks once the polynomial is long enough, never chunks below 256
    assert eval_plan(lib, 1 << 24, 1) == (True, 4096, 4096) and eval_levels(lib, 1 << 24, 1) == [(4096, 4096), (4096, 1)]
    assert eval_plan(lib, (1 << 24) + 1, 1) == (True, 4160, 4033)
    assert eval_plan(lib, 1 << 16, 1) == (True, 256, 256) and eval_levels(lib, 1 << 16, 1) == [(256, 256), (256, 1)]
    # more pairs, fewer chunks per pair: 3 pairs want ceil(4096 / 3) = 1366 chunks
    split, c, chunks = eval_plan(lib, 1 << 24, 3)
    assert split and c % 64 == 0 and c == -(-(-(-(1 << 24) // 1366)) // 64) * 64 and chunks == -(-(1 << 24) // c) <= 1366
    assert eval_plan(lib, big, 4096) == (True, big, 1) and eval_plan(lib, big, 5000) == (True, big, 1)
    # the key: -1 is the point route whatever the shape, a positive value the split route with that chunk, 1 is taken as 2
    assert not eval_plan(lib, 1 << 24, 1, -1)[0] and eval_plan(lib, 5, 1 << 20, 16) == (True, 16, 1)
    for n, chunks in ((15, 1), (16, 1), (17, 2), (53, 4)):
        assert eval_plan(lib, n, 1, 16) == (True, 16, chunks)
    assert eval_levels(lib, 53, 3, 16) == [(16, 4), (16, 1)] and eval_levels(lib, 16 * 16 + 1, 1, 16) == [(16, 17), (16, 2), (16, 1)]
    assert eval_levels(lib, 9, 1, 1) == [(2, 5), (2, 3), (2, 2), (2, 1)]
    assert eval_levels(lib, 1, 1, 16) == [(16, 1)] and eval_levels(lib, 1 << 24, 1, -1) == []


def test_degree_scan_geometry(lib):
    out = (ctypes.c_uint64 * 2)()
    for size, want in ((1, (1, 1)), (4096, (1, 4096)), (4097, (2, 2049)), (1 << 22, (1024, 4096)), ((1 << 22) + 1, (1024, 4097)), (1 << 30, (1024, 1 << 20))):
        lib.pp_hnz_plan(size, out)
        assert tuple(out) == want and out[0] * out[1] >= size, size


def tile(lib, dn, db, T, t):
    out = (ctypes.c_int64 * 6)()
    if not lib.pp_div_tile(dn, db, T, t, out):
        return None
    return dict(zip(("hi", "lo", "cnt", "nb", "upd_lo", "upd_cnt"), out))


def test_division_tile_schedule(lib):
    """nq quotient coefficients in tiles of T from the top: tile t covers q[lo..hi], hi = nq - 1 - t T, lo = max(0, hi - T + 1); its window
    of the remainder is r[deg_b + lo .. deg_b + hi]; the update covers r[lo .. lo + deg_b); only the last tile is partial"""
    assert [lib.pp_tile(w) for w in (0, 1, 2, 3, 4, 8, 16)] == [0, lib.pp_tile(1), lib.pp_tile(1), 0, 0, lib.pp_tile(1), 0]
    T = lib.pp_tile(1)
    assert T >= 2
    for nq in (1, T - 1, T, T + 1, 2 * T + 3):
        for db in (0, 1, T - 1, T, T + 1):
            dn = db + nq - 1
            ntiles = lib.pp_div_tiles(dn, db, T)
            assert ntiles == -(-nq // T), (nq, db)
            covered = []
            for t in range(ntiles):
                w = tile(lib, dn, db, T, t)
                assert w["hi"] == nq - 1 - t * T and w["lo"] == max(0, w["hi"] - T + 1) and w["cnt"] == w["hi"] - w["lo"] + 1, (nq, db, t, w)
                assert w["cnt"] == T or (t == ntiles - 1 and w["lo"] == 0 and w["cnt"] == nq - t * T), (nq, db, t, w)
                assert w["nb"] == min(T, db + 1) and (w["upd_lo"], w["upd_cnt"]) == (w["lo"], db)
                assert db + w["hi"] <= dn and w["upd_lo"] + w["upd_cnt"] == db + w["lo"]  # the update ends where the window begins
                covered += range(w["lo"], w["hi"] + 1)
            assert sorted(covered) == list(range(nq)) and tile(lib, dn, db, T, ntiles) is None
    # nothing to divide
    assert lib.pp_div_tiles(3, 4, T) == 0 and lib.pp_div_tiles(-1, 2, T) == 0 and lib.pp_div_tiles(5, -1, T) == 0
    assert tile(lib, 3, 4, T, 0) is None and tile(lib, -1, 0, T, 0) is None and tile(lib, 5, -1, T, 0) is None


def test_division_schedule_divides(lib):
    """the two kernels' work, replayed on integers mod p by the harness from the schedule alone: q b + r == numerator and deg r < deg b"""
    import random

    rng = random.Random(2239)
    for T in (4, lib.pp_tile(1)):
        for nq in (1, T - 1, T, T + 1, 2 * T + 3):
            for db in (0, 1, T - 1, T, T + 1):
                dn = db + nq - 1
                num, den = [rng.randrange(P) for _ in range(dn + 1)], [rng.randrange(P) for _ in range(db + 1)]
                num[dn], den[db] = num[dn] or 1, den[db] or 1
                if nq > 4:
                    num[dn - 1] = num[dn - 2] = 0
                assert lib.pp_div_simulate((ctypes.c_uint64 * len(num))(*num), dn, (ctypes.c_uint64 * len(den))(*den), db, T) == 0, (T, nq, db)


def test_every_argument_rule(lib):
    A, B, C, D = 0x10000, 0x20000, 0x30000, 0x40000

    def slice_(cfg=1, inp=A, out=B, offset=3, stride=5, size_in=24, size_out=5, in_dev=1, out_dev=1, batch=1, eb=4):
        return lib.pp_slice_check(cfg, inp, in_dev, out, out_dev, offset, stride, size_in, size_out, batch, eb)

    assert slice_() == OK and slice_(cfg=0) == BAD_POINTER and slice_(cfg=0, size_out=0) == BAD_POINTER
    assert slice_(size_out=0) == EMPTY and slice_(size_out=0, inp=0, out=0, offset=99) == EMPTY  # the empty call comes before the vectors
    assert slice_(inp=0) == BAD_POINTER and slice_(out=0) == BAD_POINTER and slice_(inp=0, size_out=6) == BAD_POINTER
    assert slice_(size_out=6) == BAD_ARGUMENT and slice_(offset=4) == BAD_ARGUMENT and slice_(size_in=23) == BAD_ARGUMENT
    assert slice_(stride=0, offset=23) == OK and slice_(stride=0, offset=24) == BAD_ARGUMENT and slice_(stride=0, offset=24, size_out=1) == BAD_ARGUMENT
    assert slice_(offset=(1 << 64) - 1, stride=(1 << 64) - 1, size_out=(1 << 64) - 1) == BAD_ARGUMENT  # no wrap-around
    # overlap: 24 * 3 elements of 4 bytes in, 5 * 3 out
    assert slice_(batch=3, out=A + 288) == OK and slice_(batch=3, out=A + 284) == BAD_ARGUMENT and slice_(batch=3, out=A - 60) == OK
    assert slice_(batch=3, out=A - 56) == BAD_ARGUMENT and slice_(out=A) == BAD_ARGUMENT and slice_(out=A, out_dev=0) == OK

    hnz = lib.pp_hnz_check
    assert hnz(1, A, B, 7) == OK and hnz(0, A, B, 7) == BAD_POINTER and hnz(1, 0, B, 7) == BAD_POINTER and hnz(1, A, 0, 7) == BAD_POINTER
    assert hnz(1, A, B, 0) == BAD_ARGUMENT and hnz(1, 0, B, 0) == BAD_POINTER and hnz(0, 0, 0, 0) == BAD_POINTER

    ev = lib.pp_eval_check
    assert ev(1, A, B, C, 5, 4, 0) == OK and ev(1, A, B, C, 5, 4, -1) == OK and ev(1, A, B, C, 5, 4, 16) == OK
    assert ev(0, A, B, C, 5, 4, 0) == BAD_POINTER and [ev(1, *ptrs, 5, 4, 0) for ptrs in ((0, B, C), (A, 0, C), (A, B, 0))] == [BAD_POINTER] * 3
    assert ev(1, A, B, C, 0, 4, 0) == BAD_ARGUMENT and ev(1, A, B, C, 5, 0, 0) == BAD_ARGUMENT and ev(1, A, B, C, 5, 4, -2) == BAD_ARGUMENT
    assert ev(1, 0, B, C, 0, 4, -7) == BAD_POINTER  # a missing vector comes before the other rules

    dv = lib.pp_division_check
    assert dv(1, A, B, C, D, 9, 3) == OK and dv(0, A, B, C, D, 9, 3) == BAD_POINTER
    assert [dv(1, *ptrs, 9, 3) for ptrs in ((0, B, C, D), (A, 0, C, D), (A, B, 0, D), (A, B, C, 0))] == [BAD_POINTER] * 4
    assert dv(1, A, B, C, D, 0, 3) == BAD_ARGUMENT and dv(1, A, B, C, D, 9, 0) == BAD_ARGUMENT and dv(1, A, B, C, D, 9, -1) == BAD_ARGUMENT
    assert dv(1, 0, B, C, D, 0, 0) == BAD_POINTER

    dg = lib.pp_degree_check
    assert dg(5, 2, 4, 6) == OK and dg(5, 2, 9, 9) == OK
    assert dg(5, -1, 9, 9) == BAD_ARGUMENT                       # a zero denominator
    assert dg(5, 2, 4, 5) == BAD_ARGUMENT                        # r_size < deg_n + 1
    assert dg(5, 2, 3, 6) == BAD_ARGUMENT                        # q_size < deg_n - deg_b + 1
    assert dg(2, 5, 0, 3) == OK and dg(2, 5, 0, 2) == BAD_ARGUMENT  # shorter than the denominator: no quotient needed, r holds the numerator
    assert dg(-1, 0, 0, 0) == OK and dg(-1, -1, 9, 9) == BAD_ARGUMENT  # a zero numerator needs no room at all

    ov = lib.pp_overlap
    assert ov(A, 16, 1, A + 15, 4, 1) and not ov(A, 16, 1, A + 16, 4, 1) and ov(A + 8, 16, 0, A, 9, 0) and not ov(A + 8, 16, 0, A, 8, 0)
    assert not ov(A, 16, 1, A, 16, 0) and not ov(A, 0, 1, A, 16, 1)


def test_plan_harness_under_address_and_undefined_behaviour_sanitizers():
    """a stand-alone program: nothing of it is loaded into this interpreter"""
    exe = os.path.join(HERE, "_build", "poly_plan_harness_san")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    if _stale(exe):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-DPOLY_PLAN_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                               "-static-libubsan", SRC, "-o", exe])
    run = subprocess.run([exe], text=True, capture_output=True)
    assert run.returncode == 0 and "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, (run.stdout[-500:], run.stderr[-2000:])
    assert run.stdout.startswith("checksum ")
