"""GPU parity of the one-lane bucket reduction (msm_impl.hpp k_reduce_wave / k_reduce_window), whose additions run on the signed
limb layer for bn254 and grumpkin (ec.hpp add_signed: 12 products, 9 reductions) and on EC::add for every other curve.

A uniform single MSM of 2^10 .. 2^13 terms reduces its buckets with the four-lane kernels, so the one-lane kernels are reached the
way the large MSMs reach them: with a mixed-width window plan (MSMConfig.ext "hip_msm_windows": narrow and wide windows in one
launch) or as a batch of two. Window sizes: c = 8 (128 buckets: one chunk per window, the chunk kernel stores the window sum
itself), c = 13 and c = 16 (4 and 32 chunks per window: k_reduce_window runs). The inputs put the corners of the complete addition
into the reduction's own sums: a single full bucket among identities, neighbouring buckets holding multiples of one point (the
running sums meet: an addition that is a doubling), cancelled buckets between full ones, only the first or only the last bucket.
Every result is compared on affine limbs with the reference CPU backend; one reference run per input. The environment knobs are
read once per process, hence a child process for ICICLE_HIP_MSM_REDUCE_QUAD=0 (uniform plans on the one-lane kernels) and one for
ICICLE_HIP_MSM_REDUCE_SIGNED=0 (the additions of the parent)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import pyref, ref
from tests.msm_directed import (_plan_widths, in_all_scalars_equal, in_cancelling_pairs, in_equal_bases_under_scalars_k_and_k_plus_one,  # noqa: F401
                                in_identity_bases, in_scalars_one_and_r_minus_one, in_top_bucket_only)
from tests.util import cached_points, points_to_array, rand_scalars, to_words

pytestmark = pytest.mark.gpu
SIGNED = ["bn254", "grumpkin"]
# forced mixed plans of a 254-bit scalar: W windows -> widths (254 // W) and one more
WINDOWS = {8: 36, 13: 21, 16: 16}


def _mixed(hip, cname, sc, bases, nwin):
    from icicle_amd import msm as M
    from icicle_amd._lib import lib

    ext = lib.create_config_extension()
    lib.config_extension_set_int(ext, b"hip_msm_windows", nwin)
    try:
        cfg = hip.MSMConfig.default()
        cfg.ext = ext
        return M.msm(cname, sc, bases, cfg)
    finally:
        lib.destroy_config_extension(ext)


def _check(hip, cname, sc, bases, plans=(8, 13, 16)):
    refc = ref.RefCurve(cname)
    exp = refc.to_affine(refc.msm(sc, bases))
    for c in plans:
        got = _mixed(hip, cname, sc, bases, WINDOWS[c])
        assert np.array_equal(refc.to_affine(got), exp), f"{cname} mixed plan c={c}"
        assert refc.is_on_curve(got[0])


def _bases(C, n, period=1024):
    pts = points_to_array(C, cached_points(C, min(n, period)))
    return np.ascontiguousarray(np.tile(pts, ((n + period - 1) // period, 1))[:n])


def _neg_rows(C, arr):
    L = C.limbs_q
    out = arr.copy()
    for i in range(len(arr)):
        y = sum(int(v) << (32 * k) for k, v in enumerate(arr[i, L:]))
        out[i, L:] = to_words([(C.q - y) % C.q], L)[0]
    return out


# ---- the directed inputs live in tests/msm_directed.py (in_*, _plan_widths), shared with tests/test_gpu_msm_quad_reduce.py (the same bucket
# patterns through the four-lane kernels) and tests/test_gpu_msm_groups_directed.py (every group).
# r: the scalar modulus; bases_fn(n, period=1024): n base rows; neg_fn(rows): the rows of the negated points. Each returns (scalars, bases).
def _g1_fns(C):
    return C.r, functools.partial(_bases, C), functools.partial(_neg_rows, C)


@pytest.mark.parametrize("cname", SIGNED)
def test_spread_scalars(hip, cname):
    C = pyref.CURVES[cname]
    rng = np.random.default_rng(9101)
    n = (1 << 13) - 3
    _check(hip, cname, to_words(rand_scalars(rng, n, C.r), 8), _bases(C, n))


@pytest.mark.parametrize("cname", SIGNED)
def test_all_scalars_equal(hip, cname):
    """one full bucket per window, every other bucket the identity: line and tri0 stay the identity until that row"""
    vals, bases = in_all_scalars_equal(*_g1_fns(pyref.CURVES[cname]))
    _check(hip, cname, to_words(vals, 8), bases)


@pytest.mark.parametrize("cname", SIGNED)
def test_equal_bases_under_scalars_k_and_k_plus_one(hip, cname):
    """every bucket holds a multiple of ONE point and neighbouring buckets are full: column sums and running sums that are equal
    or negatives of each other meet in the lane scans (an addition that is a doubling, one that gives the identity)"""
    vals, bases = in_equal_bases_under_scalars_k_and_k_plus_one(*_g1_fns(pyref.CURVES[cname]))
    _check(hip, cname, to_words(vals, 8), bases)


@pytest.mark.parametrize("cname", SIGNED)
def test_cancelling_pairs_leave_identity_buckets_between_full_ones(hip, cname):
    vals, bases = in_cancelling_pairs(*_g1_fns(pyref.CURVES[cname]))
    _check(hip, cname, to_words(vals, 8), bases)


@pytest.mark.parametrize("cname", SIGNED)
def test_scalars_one_and_r_minus_one(hip, cname):
    """only bucket 1 of window 0 is populated, with both signs: every other chunk sums identities"""
    vals, bases = in_scalars_one_and_r_minus_one(*_g1_fns(pyref.CURVES[cname]))
    _check(hip, cname, to_words(vals, 8), bases)


@pytest.mark.parametrize("cname", SIGNED)
@pytest.mark.parametrize("c", [8, 13, 16])
def test_top_bucket_only(hip, cname, c):
    """every second window's digit is 2^(width - 1), the largest a signed digit takes: the last bucket of the last chunk (row 0 of
    lane 63), with the identity everywhere else but for what a carry leaves in bucket 1 of the window above"""
    C = pyref.CURVES[cname]
    r, bases_fn, _ = _g1_fns(C)
    vals, bases = in_top_bucket_only(r, bases_fn, _plan_widths(C.r.bit_length(), WINDOWS[c]))
    _check(hip, cname, to_words(vals, 8), bases, plans=(c,))


@pytest.mark.parametrize("cname", SIGNED)
def test_identity_bases(hip, cname):
    vals, bases = in_identity_bases(*_g1_fns(pyref.CURVES[cname]))
    _check(hip, cname, to_words(vals, 8), bases)


@pytest.mark.parametrize("cname", SIGNED)
@pytest.mark.parametrize("c", [13, 16])
def test_batch_of_two(hip, cname, c):
    """a batch folds into one launch sequence with twice the windows: uniform windows on the one-lane kernels (4 and 32 chunks each)"""
    from icicle_amd import msm as M

    C = pyref.CURVES[cname]
    refc = ref.RefCurve(cname)
    rng = np.random.default_rng(9108 + c)
    n = (1 << 11) + 5
    bases = _bases(C, n)
    vals = rand_scalars(rng, 2 * n, C.r)
    vals[n:n + 200] = [vals[n]] * 200  # the second MSM: one heavy bucket per window
    sc = to_words(vals, 8)
    cfg = hip.MSMConfig.default()
    cfg.batch_size = 2
    cfg.are_points_shared_in_batch = True
    cfg.c = c
    got = M.msm(cname, sc, bases, cfg)
    assert np.array_equal(refc.to_affine(got), refc.to_affine(refc.msm(sc, bases, batch=2, shared=True)))


def test_bls12_381_keeps_its_path(hip):
    """a 14-limb curve has no signed addition: the same kernels with EC::add, a mixed plan and a batch of two"""
    from icicle_amd import msm as M

    C = pyref.BLS12_381
    refc = ref.RefCurve("bls12_381")
    rng = np.random.default_rng(9109)
    n = (1 << 11) + 1
    bases = _bases(C, n)
    sc = to_words(rand_scalars(rng, 2 * n, C.r), 8)
    exp = refc.to_affine(refc.msm(sc[:n], bases))
    assert np.array_equal(refc.to_affine(_mixed(hip, "bls12_381", sc[:n], bases, 21)), exp)  # 255 bits: 18 x 12 + 3 x 13
    cfg = hip.MSMConfig.default()
    cfg.batch_size = 2
    cfg.are_points_shared_in_batch = True
    cfg.c = 13
    got = M.msm("bls12_381", sc, bases, cfg)
    assert np.array_equal(refc.to_affine(got), refc.to_affine(refc.msm(sc, bases, batch=2, shared=True)))


_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, %r)
import icicle_amd as hip
from icicle_amd import msm as M, runtime
from icicle_amd._lib import lib
from oracle import pyref, ref
from tests.util import cached_points, points_to_array, rand_scalars, to_words
runtime.set_device(0)
for cname in ("bn254", "grumpkin"):
    C = pyref.CURVES[cname]
    refc = ref.RefCurve(cname)
    rng = np.random.default_rng(9110)
    n = (1 << 12) - 1
    pts = points_to_array(C, cached_points(C, 1024))
    bases = np.ascontiguousarray(np.tile(pts, (4, 1))[:n])
    bases[7::50] = 0
    vals = rand_scalars(rng, n, C.r)
    vals[100:400] = [vals[100]] * 300
    sc = to_words(vals, 8)
    exp = refc.to_affine(refc.msm(sc, bases))
    for c in (8, 13, 16):  # uniform plans
        cfg = hip.MSMConfig.default()
        cfg.c = c
        assert np.array_equal(refc.to_affine(M.msm(cname, sc, bases, cfg)), exp), (cname, "uniform", c)
    for nwin in (36, 21, 16):  # mixed plans
        ext = lib.create_config_extension()
        lib.config_extension_set_int(ext, b"hip_msm_windows", nwin)
        cfg = hip.MSMConfig.default()
        cfg.ext = ext
        got = M.msm(cname, sc, bases, cfg)
        lib.destroy_config_extension(ext)
        assert np.array_equal(refc.to_affine(got), exp), (cname, "mixed", nwin)
print("REDUCE OK")
"""


@pytest.mark.parametrize("knob", ["ICICLE_HIP_MSM_REDUCE_QUAD", "ICICLE_HIP_MSM_REDUCE_SIGNED"])
def test_knobs_off_in_a_child_process(hip, knob):
    """REDUCE_QUAD=0: uniform single MSMs take the one-lane kernels too (c = 8: the direct store, c = 13 and 16: the window kernel).
    REDUCE_SIGNED=0: the same kernels with EC::add, as before the signed addition; it must agree as well."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    env[knob] = "0"
    r = subprocess.run([sys.executable, "-c", _CHILD % root], capture_output=True, text=True, env=env, timeout=600, cwd=root)
    assert r.returncode == 0 and "REDUCE OK" in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]
