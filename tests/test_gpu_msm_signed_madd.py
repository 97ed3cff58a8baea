"""GPU parity of the bucket accumulation on inputs that lean on the mixed addition's corners (ec.hpp madd; the signed-limb form for the
9-limb base fields of bn254 and grumpkin, the carry-normalised form for the 14-limb fields and for G2).

The window size is forced small through MSMConfig.c (4 and 8): a window then has 8 or 128 buckets, so at 2^10 .. 2^14 terms a bucket holds
hundreds of points -- long chains on one accumulator -- and the heaviest buckets are cut into overflow segments. The inputs put the
exceptional cases of the addition inside those chains: equal points meeting (doubling), a point meeting its negative (cancel, then the
first-point path again), negated operands (top scalar bit set: every digit's sign flips), identity bases. Every result is compared on
affine limbs with the reference CPU backend, as tests/test_gpu_msm_passb_owned.py does; one reference run per input."""
import numpy as np
import pytest

from oracle import pyref, ref
from tests.util import cached_points, points_to_array, rand_scalars, to_words

pytestmark = pytest.mark.gpu
CURVES = ["bn254", "grumpkin", "bls12_381", "bls12_377"]
CS = (4, 8)


def _check(hip, cname, sc, bases, g2=False):
    """MSMConfig.c = 4 and 8 against ONE reference result"""
    from icicle_amd import msm as M

    refc = ref.RefCurve(cname, g2=g2)
    exp = refc.to_affine(refc.msm(sc, bases))
    for c in CS:
        cfg = hip.MSMConfig.default()
        cfg.c = c
        got = M.msm(cname, sc, bases, cfg, g2=g2)
        assert np.array_equal(refc.to_affine(got), exp), f"{cname} c={c}"
        assert refc.is_on_curve(got[0])
    return exp


def _bases(C, n, period=1024):
    pts = points_to_array(C, cached_points(C, min(n, period)))
    return np.ascontiguousarray(np.tile(pts, ((n + period - 1) // period, 1))[:n])


def _neg_rows(C, arr):
    """(x, y) -> (x, q - y) on an array of affine words"""
    L = C.limbs_q
    out = arr.copy()
    for i in range(len(arr)):
        y = sum(int(v) << (32 * k) for k, v in enumerate(arr[i, L:]))
        out[i, L:] = to_words([(C.q - y) % C.q], L)[0]
    return out


@pytest.mark.parametrize("cname", CURVES)
def test_all_scalars_equal(hip, cname):
    """one bucket per window takes every point: the longest chains and the most overflow segments a launch can see"""
    C = pyref.CURVES[cname]
    rng = np.random.default_rng(8101)
    n = (1 << 12) + 3
    s = rand_scalars(rng, 1, C.r)[0]
    _check(hip, cname, to_words([s] * n, 8), _bases(C, n))


@pytest.mark.parametrize("cname", CURVES)
def test_all_bases_equal(hip, cname):
    """every bucket holds copies of one point or of its negative: the second addition of a bucket is a doubling or a cancellation,
    and a cancelled bucket starts again through the first-point path"""
    C = pyref.CURVES[cname]
    rng = np.random.default_rng(8102)
    n = (1 << 10) + 1
    bases = np.ascontiguousarray(np.tile(points_to_array(C, cached_points(C, 1)), (n, 1)))
    _check(hip, cname, to_words(rand_scalars(rng, n, C.r), 8), bases)


@pytest.mark.parametrize("cname", CURVES)
def test_bases_in_cancelling_pairs(hip, cname):
    """bases 2i and 2i + 1 are P_i and -P_i. The first half of the pairs share a scalar (the two meet in every bucket they visit and
    cancel, next to each other in a stable sort or with other points between them), the second half have independent scalars."""
    C = pyref.CURVES[cname]
    rng = np.random.default_rng(8103)
    n = 1 << 12
    half = _bases(C, n // 2)
    bases = np.empty((n, half.shape[1]), dtype=np.uint32)
    bases[0::2] = half
    bases[1::2] = _neg_rows(C, half)
    vals = rand_scalars(rng, n, C.r)
    for i in range(0, n // 2, 2):
        vals[i + 1] = vals[i]
    _check(hip, cname, to_words(vals, 8), bases)


@pytest.mark.parametrize("cname", CURVES)
def test_scalars_with_the_top_bit_set(hip, cname):
    """scalars in [2^(bits - 1), r): the signed-digit recoding negates such a scalar, so every digit arrives with its sign flipped"""
    C = pyref.CURVES[cname]
    rng = np.random.default_rng(8104)
    n = (1 << 12) - 5
    top = 1 << (C.r.bit_length() - 1)
    vals = [top + v % (C.r - top) for v in rand_scalars(rng, n, C.r)]
    assert all(top <= v < C.r for v in vals)
    _check(hip, cname, to_words(vals, 8), _bases(C, n))


@pytest.mark.parametrize("cname", CURVES)
def test_scalars_r_minus_one_and_one(hip, cname):
    """r - 1 and 1 alternate: the two values are negatives of each other, every point lands in bucket 1 of window 0 with either sign"""
    C = pyref.CURVES[cname]
    n = (1 << 11) + 7
    vals = [C.r - 1 if i % 2 else 1 for i in range(n)]
    _check(hip, cname, to_words(vals, 8), _bases(C, n, period=300))


@pytest.mark.parametrize("cname", CURVES)
def test_identity_bases_inside_the_chains(hip, cname):
    """(0, 0) at the start of a bucket's list, in runs and at its end: skipped without touching the accumulator or its empty flag"""
    C = pyref.CURVES[cname]
    rng = np.random.default_rng(8106)
    n = 1 << 12
    bases = _bases(C, n)
    bases[0:3] = 0
    bases[100:400:3] = 0
    bases[1000:1100] = 0
    bases[-1] = 0
    vals = rand_scalars(rng, n, C.r)
    vals[0] = vals[1] = vals[2] = vals[5]
    _check(hip, cname, to_words(vals, 8), bases)


def test_largest_size_with_mixed_corners(hip):
    """2^14 terms on bn254: equal scalars in runs, repeated bases, negatives and identities together"""
    C = pyref.BN254
    rng = np.random.default_rng(8107)
    n = 1 << 14
    bases = _bases(C, n, period=512)
    bases[1::7] = _neg_rows(C, bases[0::7][: len(bases[1::7])])
    bases[5::97] = 0
    vals = rand_scalars(rng, n, C.r)
    for i in range(0, n, 16):
        vals[i:i + 8] = [vals[i]] * 8
    _check(hip, "bn254", to_words(vals, 8), bases)


def test_g2_is_untouched(hip):
    """bn254 G2 (Fq2 coordinates) keeps the carry-normalised addition: equal scalars in runs and repeated bases at c = 4 and 8"""
    from icicle_amd import msm as M

    C = pyref.BN254
    rng = np.random.default_rng(8108)
    n = 1 << 10
    g = M.generate_affine_points("bn254", 64, k0=4711, g2=True)
    bases = np.ascontiguousarray(np.tile(g, (n // 64, 1)))
    vals = rand_scalars(rng, n, C.r)
    for i in range(0, n, 8):
        vals[i:i + 4] = [vals[i]] * 4
    _check(hip, "bn254", to_words(vals, 8), bases, g2=True)
