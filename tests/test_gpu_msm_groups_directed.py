"""GPU parity of the MSM's group-dependent kernels (msm_impl.hpp k_accumulate, k_fold_overflow, k_reduce_wave, k_reduce_small,
k_reduce_window, k_final*) on DIRECTED inputs, for all seven groups they are instantiated for: G1 of bn254, bls12_381, bls12_377, grumpkin
and G2 of bn254, bls12_381, bls12_377. The kernels differ per group in register budget, in the block size of the window kernel and in the
addition formula; the directed inputs of the neighbouring modules reach them for bn254 and grumpkin (and partly bls12_381 G1 / BN254 G2) only.

Oracle: the bases are (K0 + i) G from generate_affine_points, a negated row counts as -(K0 + i), a zero row as nothing, so the expected
result is ((sum s_i k_i) mod r) G -- one scalar multiplication on Python integers (tests/msm_directed.py Group.expected), compared on affine
coordinates. Once per group and section the smallest input is also compared with the reference CPU backend.

 0. generate_affine_points against the Python definition: the oracle rests on it.
 1. Overflow segments: buckets of window 0 with chosen sizes (seg, seg + 1, k seg, ...), one MSM per fold width of k_fold_overflow
    (G = 1, 4, 16, 16, 64), plus the overflow threads of the second MSM of a batch with its own bases and of an MSM on a base table.
 2. The six directed bucket patterns through k_reduce_wave / k_reduce_window for the five groups that never had them: BLS G2 on uniform
    plans (their production route), every group on forced mixed-width plans, the four-lane-capable ones also as a batch of two.
 3. k_reduce_small with 4, 8, 16 and 32 lanes per window, full and partly empty last waves.
 4. k_reduce_window with all 128 lanes of its smaller block (bls12_381 G2, c = 18 and 19: 16 and 32 rows per lane in k_reduce_wave).
That every shape takes the route it is meant to, and that every input fills the buckets it is meant to, is asserted on the CPU from
msm_plan.h and a model of the recoding: tests/test_msm_groups_directed_cpu.py."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import ref
from tests import msm_directed as D
from tests.util import rand_scalars, to_words

pytestmark = pytest.mark.gpu
# MEASURED on an MI355X (one run each): this module alone 112 tests in 9.0 s of pytest (11.2 s wall), 2.7 s of that session setup; the
# slowest test 0.2 s (the 2^14 generated points against 1040 Python additions), the four-input k_reduce_small cases on BLS12-381 G2
# 0.10 - 0.16 s, c = 19 with its 1.2 GB of buckets 0.07 s (the allocation succeeded: both window sizes stay), every other test under
# 0.1 s. The Python integers are the cost, not the kernels; the reference's G2 legs (one per group and section, 1000 - 2000 terms) do
# not show among the slowest, so none was cut. The whole GPU suite with this module: 1780 passed, 11 skipped in 930.6 s (934 s wall, 82 s
# of it session setup). The suite without it was not measured on that machine: it differs by these 112 tests, about 10 s.
# THAT THE TESTS CAN FAIL: against a library with three changes that alter a value but no address, loop bound or barrier -- k_fold_overflow
# without the addition of the last tree level (s = 1), k_reduce_small without the d = 2 step of its suffix scan, k_reduce_window without the
# s2 = 64 level of its block tree -- 85 of the 112 tests fail: every overflow test with G >= 4 (42; the seven G = 1 launches have no tree and
# pass) and the 17 one-lane pattern tests whose c = 8 launch holds a bucket of more than two overflow segments; all 24 k_reduce_small tests, at their first input (random scalars:
# no overflowing bucket); both 128-lane window tests, also at the random input. The generator tests and the patterns without a heavy bucket
# pass, as they must: window blocks of 64 threads never reach the s2 = 64 level.

ALL = pytest.mark.parametrize("cname,g2", D.GROUPS, ids=[D.gid(*g) for g in D.GROUPS])


@functools.lru_cache(maxsize=None)
def _group(cname, g2):
    from icicle_amd import msm as M

    return D.Group(cname, g2).bind(lambda n, k0: M.generate_affine_points(cname, n, k0=k0, g2=g2))


@functools.lru_cache(maxsize=None)
def _ref(cname, g2):
    return ref.RefCurve(cname, g2=True) if g2 else ref.RefCurve(cname)


def _config(hip, **kw):
    cfg = hip.MSMConfig.default()
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def _plan(hip, g, n, windows=0, **kw):
    """the plan msm() makes for this call (icicle_hip_msm_plan_info)"""
    from icicle_amd._lib import lib

    out = (ctypes.c_int * 8)()
    assert lib.icicle_hip_msm_plan_info(n, g.bits, ctypes.byref(_config(hip, **kw)), windows, out) == 0
    return dict(zip(("c", "nwin", "n_lo", "negate", "nb", "used", "seg", "wpf"), out))


def _msm(hip, g, sc, bases, windows=0, **kw):
    from icicle_amd import msm as M
    from icicle_amd._lib import lib

    cfg = _config(hip, **kw)
    ext = None
    if windows:
        ext = lib.create_config_extension()
        lib.config_extension_set_int(ext, b"hip_msm_windows", windows)
        cfg.ext = ext
    try:
        return M.msm(g.cname, sc, bases, cfg, g2=g.g2)
    finally:
        if ext:
            lib.destroy_config_extension(ext)


class Input:
    """scalars (Python integers; a batch: the MSMs one after the other) and bases, with the expected affine results"""

    def __init__(self, g, vals, bases, batch=1, shared=True, bitsize=0):
        self.g, self.batch, self.shared, self.bitsize = g, batch, shared, bitsize
        self.n = len(vals) // batch
        assert len(vals) == batch * self.n and len(bases) == (self.n if shared else batch * self.n)
        self.sc, self.bases = to_words(vals, 8), bases
        self.exp = [g.expected(vals[b * self.n:(b + 1) * self.n], bases if shared else bases[b * self.n:(b + 1) * self.n], bitsize) for b in range(batch)]

    def config(self):
        kw = dict(bitsize=self.bitsize) if self.bitsize else {}
        if self.batch > 1:
            kw.update(batch_size=self.batch, are_points_shared_in_batch=self.shared)
        return kw

    def check(self, hip, what, windows=0, reference=False, bases=None, **kw):
        got = _msm(hip, self.g, self.sc, self.bases if bases is None else bases, windows=windows, **self.config(), **kw)
        for b in range(self.batch):
            assert self.g.affine(got[b]) == self.exp[b], f"{self.g.id} {what} {kw} windows={windows} MSM {b}"
        if reference:
            refc = _ref(self.g.cname, self.g.g2)
            exp = refc.msm(self.sc, self.bases, batch=self.batch, shared=self.shared, bitsize=self.bitsize)
            assert np.array_equal(refc.to_affine(got), refc.to_affine(exp)), f"{self.g.id} {what}: reference"
            assert all(refc.is_on_curve(got[b]) for b in range(self.batch))
        return got


# ---- 0. the generator ----
@ALL
def test_generated_points_are_the_multiples_of_the_generator(hip, cname, g2):
    """(K0 + i) G for i < 1040 -- the 1024 distinct bases of every input here, sixteen points per thread, the first block of 64 threads and
    the start of the second -- and the last point of 2^14"""
    from icicle_amd import msm as M

    g = D.Group(cname, g2)
    n = 1 << 14
    pts = M.generate_affine_points(cname, n, k0=D.K0, g2=g2)
    assert np.array_equal(pts[:1040], g.rows(g.gen(1040, D.K0)))
    assert np.array_equal(pts[n - 1:], g.rows(g.gen(1, D.K0 + n - 1)))
    assert np.array_equal(_group(cname, g2)._base, pts[:D.PERIOD])


# ---- 1. overflow segments ----
def _overflow_input(hip, g, launch, **plan_kw):
    sizes_of, mx, G = D.OVERFLOW_LAUNCHES[launch]
    seg = _plan(hip, g, 1 << 15, c=D.OVERFLOW_C, **plan_kw)["seg"]
    sizes = sizes_of(seg)
    vals, bases = D.in_overflow(*g.fns(), seg, sizes)
    p = _plan(hip, g, len(vals), c=D.OVERFLOW_C, **plan_kw)
    assert len(vals) <= 1 << 15 and (p["c"], p["seg"], p["n_lo"]) == (D.OVERFLOW_C, seg, 0), p
    assert max((m + seg - 1) // seg - 1 for m in sizes.values()) == mx and D.fold_width(mx) == G
    return vals, bases


@pytest.mark.parametrize("launch", sorted(D.OVERFLOW_LAUNCHES), ids=[f"mx{mx}_G{G}" for _, (_, mx, G) in sorted(D.OVERFLOW_LAUNCHES.items())])
@ALL
def test_overflow_segments_fold_at_every_group_width(hip, cname, g2, launch):
    """buckets of seg, seg + 1, 2 seg, 2 seg + 1, 3 seg ... 258 seg entries: the largest number of overflow segments of the launch picks the
    lanes per bucket of k_fold_overflow (1, 4, 16, 64); the heavy buckets mix distinct points, P / -P pairs, a run of one point and zero rows"""
    g = _group(cname, g2)
    vals, bases = _overflow_input(hip, g, launch)
    Input(g, vals, bases).check(hip, f"overflow launch {launch}", reference=launch == 1, c=D.OVERFLOW_C)


@ALL
def test_overflow_segments_of_the_second_msm_of_a_batch_with_its_own_bases(hip, cname, g2):
    """an overflow thread finds its MSM's bases from its bucket's window (k_accumulate: bases += (wp / wpf) * bases_stride)"""
    g = _group(cname, g2)
    vals, bases = _overflow_input(hip, g, 2, batch_size=2, are_points_shared_in_batch=False)
    n = len(vals)
    first = rand_scalars(np.random.default_rng(9140), n, g.r)
    both = np.ascontiguousarray(np.concatenate([np.roll(g.bases_fn(n), 7, axis=0), bases]))
    Input(g, first + vals, both, batch=2, shared=False).check(hip, "overflow in the second MSM", c=D.OVERFLOW_C)


@ALL
def test_overflow_segments_on_a_base_table(hip, cname, g2):
    """precompute_factor 2: the windows 0 and wpf of a scalar share one bucket set, the list entries carry the table index"""
    from icicle_amd import msm as M

    g = _group(cname, g2)
    vals, bases = _overflow_input(hip, g, 2, precompute_factor=2)
    table = M.precompute_bases(cname, bases, _config(hip, precompute_factor=2, c=D.OVERFLOW_C), g2=g2)
    assert np.array_equal(table[::2], bases)
    Input(g, vals, bases).check(hip, "overflow on a base table", bases=table, precompute_factor=2, c=D.OVERFLOW_C)


# ---- 2. directed bucket patterns through the one-lane reduction ----
def _one_lane_runs(hip, g, c, n):
    """(what, windows, config) of the one-lane launches of window size c, each with the plan msm() will make asserted"""
    runs = []
    nb = 1 << (c - 1)
    if not g.quad_ok:
        p = _plan(hip, g, n, c=c)
        assert (p["c"], p["n_lo"], p["nb"]) == (c, 0, nb), p
        runs.append(("uniform", 0, dict(c=c)))
    W = D.mixed_windows(g.bits, c)
    p = _plan(hip, g, n, windows=W)
    assert (p["c"], p["nwin"], p["negate"], p["nb"]) == (c, W, 1, nb) and 0 < p["n_lo"] < W, p
    runs.append(("mixed", W, {}))
    return runs


@pytest.mark.parametrize("pattern", range(6), ids=D.PATTERN_IDS)
@pytest.mark.parametrize("cname,g2", D.NEVER_ONE_LANE, ids=[D.gid(*g) for g in D.NEVER_ONE_LANE])
def test_directed_buckets_through_the_one_lane_reduction(hip, cname, g2, pattern):
    g = _group(cname, g2)
    if pattern < 5:
        vals, bases = D.PATTERNS[pattern](*g.fns())
        one = Input(g, vals, bases)
        two = Input(g, vals + vals[::-1], bases, batch=2) if g.quad_ok else None
        for c in D.ONE_LANE_CS:
            for k, (what, windows, kw) in enumerate(_one_lane_runs(hip, g, c, one.n)):
                one.check(hip, f"{D.PATTERN_IDS[pattern]} {what} c={c}", windows=windows, reference=pattern == 1 and c == 8 and k == 0, **kw)
            if two and c in D.BATCH_CS:
                two.check(hip, f"{D.PATTERN_IDS[pattern]} batch of two c={c}", c=c)
        return
    # the top bucket only: the scalars follow the window plan, so every plan has its own input
    for c in D.ONE_LANE_CS:
        for what, windows, kw in _one_lane_runs(hip, g, c, 1 << 10):
            wins = D._plan_widths(g.bits, windows) if windows else D.uniform_widths(g.bits, c)
            vals, bases = D.in_top_bucket_only(g.r, g.bases_fn, wins)
            Input(g, vals, bases).check(hip, f"top bucket {what} c={c}", windows=windows, **kw)
        if g.quad_ok and c in D.BATCH_CS:
            vals, bases = D.in_top_bucket_only(g.r, g.bases_fn, D.uniform_widths(g.bits, c))
            Input(g, vals + vals[::-1], bases, batch=2).check(hip, f"top bucket batch of two c={c}", c=c)


# ---- 3. k_reduce_small at every lane width ----
@pytest.mark.parametrize("c,batch,bitsize", D.SMALL_SHAPES, ids=[f"c{c}_batch{b}" + (f"_bits{bs}" if bs else "") for c, b, bs in D.SMALL_SHAPES])
@pytest.mark.parametrize("cname,g2", D.SMALL_GROUPS, ids=[D.gid(*g) for g in D.SMALL_GROUPS])
def test_small_windows_share_a_wave(hip, cname, g2, c, batch, bitsize):
    """batch * wpf >= 64 windows of 2^(c - 1) <= 512 buckets on shared bases: random scalars, one full bucket among identities, the top
    bucket only, cancelling pairs; MSM b of the batch takes the scalars rotated by 101 b places (and b + 1 times the one scalar)"""
    g = _group(cname, g2)
    mask = (1 << bitsize) - 1 if bitsize else -1
    wins = D.uniform_widths(bitsize or g.bits, c)
    inputs = [("random", D.in_random(*g.fns(), n=700)), ("one full bucket", D.in_all_scalars_equal(*g.fns(), n=300)),
              ("top bucket", D.in_top_bucket_only(g.r, g.bases_fn, wins[:-1] if bitsize else wins)), ("cancelling pairs", D.in_cancelling_pairs(*g.fns(), n=1024))]
    for k, (what, (vals, bases)) in enumerate(inputs):
        n = len(vals)
        p = _plan(hip, g, n, c=c, batch_size=batch, **(dict(bitsize=bitsize) if bitsize else {}))
        assert (p["c"], p["nb"], p["n_lo"]) == (c, 1 << (c - 1), 0) and batch * p["wpf"] >= 64 and p["nb"] <= 512, p
        allv = []
        for b in range(batch):
            scale = b + 1 if what == "one full bucket" else 1
            allv += [(v * scale % g.r) & mask for v in vals[n - (101 * b) % n:] + vals[:n - (101 * b) % n]]
        Input(g, allv, bases, batch=batch, bitsize=bitsize).check(hip, f"{what} c={c}", reference=k == 0 and c == 5, c=c)


# ---- 4. the window kernel at its full 128 lanes ----
@pytest.mark.parametrize("c", D.FULL_WINDOW_CS)
def test_window_kernel_with_all_128_chunks(hip, c):
    """bls12_381 G2, 1024 terms in windows of 2^17 / 2^18 buckets (c = 19: 1.2 GB of buckets): k_reduce_wave with 16 / 32 rows per lane,
    k_reduce_window with a chunk for every one of its 128 threads. "top bucket only" puts the last row of lane 63 of chunk 127 to use."""
    g = _group(*D.FULL_WINDOW_GROUP)
    p = _plan(hip, g, 1024, c=c)
    assert (p["c"], p["nb"], p["n_lo"]) == (c, 1 << (c - 1), 0), p
    for k, (what, (vals, bases)) in enumerate([("random", D.in_random(*g.fns(), n=1024)), ("top bucket", D.in_top_bucket_only(g.r, g.bases_fn, D.uniform_widths(g.bits, c))),
                                               ("all scalars equal", D.in_all_scalars_equal(*g.fns(), n=1024))]):
        Input(g, vals, bases).check(hip, f"{what} c={c}", reference=k == 0 and c == 18, c=c)
