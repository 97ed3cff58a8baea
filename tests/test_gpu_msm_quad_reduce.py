"""GPU parity of the FOUR-LANE bucket reduction (msm_impl.hpp k_reduce_wave_quad + k_reduce_window_quad: every addition is
ec_dbl_quad.hpp's EcQuadAdd::add over a DPP quad, every doubling dbl_quad) on DIRECTED bucket patterns.

tests/test_gpu_msm_signed_reduce.py steers the same patterns onto the one-lane kernels (mixed plans, a batch of two, REDUCE_QUAD=0);
the default route of a uniform single MSM saw random scalars only. Here its input builders run as uniform single MSMs with
config.c = 8, 13, 16 and default knobs -- one full bucket among identities, neighbouring buckets holding k P and (k + 1) P (the
running sums meet: an addition that is a doubling, one that gives the identity), cancelled buckets between full ones, scalars 1 and
r - 1, the top bucket only, identity bases -- for bn254, grumpkin and bls12_381 G1 and for BN254 G2, the one G2 whose point fits the
registers four lanes deep (c = 8, 13). 2^10 .. 2^12 terms; every result is compared on affine limbs with the reference CPU backend, one
reference run per input. That these shapes take the four-lane kernels is asserted on the CPU, from the same msm_plan.h code:
tests/test_plan.py test_directed_quad_reduce_shapes_take_the_four_lane_kernels."""
import functools

import numpy as np
import pytest

from oracle import pyref, ref
from tests import test_gpu_msm_signed_reduce as S
from tests.test_gpu_msm_g2 import g2_array, g2_points
from tests.util import to_words

pytestmark = pytest.mark.gpu
G1 = ["bn254", "grumpkin", "bls12_381"]
CS = {False: (8, 13, 16), True: (8, 13)}  # config.c per group kind (g2)
CASES = [(cname, False) for cname in G1] + [("bn254", True)]
IDS = [f"{cname}{'_g2' if g2 else ''}" for cname, g2 in CASES]
INPUTS = [S.in_all_scalars_equal, S.in_equal_bases_under_scalars_k_and_k_plus_one, S.in_cancelling_pairs, S.in_scalars_one_and_r_minus_one, S.in_identity_bases]


def _g2_bases(C, n, period=512):
    pts = g2_array(C, g2_points(C.name, min(n, period)))
    return np.ascontiguousarray(np.tile(pts, ((n + period - 1) // period, 1))[:n])


def _g2_neg_rows(C, arr):
    L, q = C.base.limbs_q, C.base.q
    out = arr.copy()
    for col in (2, 3):  # rows are x0 | x1 | y0 | y1
        ys = [sum(int(v) << (32 * k) for k, v in enumerate(row)) for row in arr[:, col * L:(col + 1) * L]]
        out[:, col * L:(col + 1) * L] = to_words([(q - y) % q for y in ys], L)
    return out


def _fns(cname, g2):
    if g2:
        C = pyref.G2_CURVES[cname]
        return C.base.r, functools.partial(_g2_bases, C), functools.partial(_g2_neg_rows, C)
    return S._g1_fns(pyref.CURVES[cname])


@functools.lru_cache(maxsize=None)
def _ref(cname, g2):
    return ref.RefCurve(cname, g2=True) if g2 else ref.RefCurve(cname)


def _check(hip, cname, g2, vals, bases, cs):
    from icicle_amd import msm as M

    refc = _ref(cname, g2)
    sc = to_words(vals, 8)
    exp = refc.to_affine(refc.msm(sc, bases))
    for c in cs:
        cfg = hip.MSMConfig.default()
        cfg.c = c
        got = M.msm(cname, sc, bases, cfg, g2=True) if g2 else M.msm(cname, sc, bases, cfg)
        assert np.array_equal(refc.to_affine(got), exp), f"{cname}{' G2' if g2 else ''} uniform plan c={c}"
        assert refc.is_on_curve(got[0])


@pytest.mark.parametrize("build", INPUTS, ids=[f.__name__[3:] for f in INPUTS])
@pytest.mark.parametrize("cname,g2", CASES, ids=IDS)
def test_directed_buckets_through_the_four_lane_reduction(hip, cname, g2, build):
    vals, bases = build(*_fns(cname, g2))
    _check(hip, cname, g2, vals, bases, CS[g2])


@pytest.mark.parametrize("cname,g2", CASES, ids=IDS)
def test_top_bucket_only(hip, cname, g2):
    """every second window's digit is 2^(c - 1), the largest a signed digit takes: the last bucket of the window's last chunk, the
    identity everywhere else but for what a carry leaves in bucket 1 of the window above. The scalars depend on c: one reference run each."""
    r, bases_fn, _ = _fns(cname, g2)
    bits = r.bit_length()
    for c in CS[g2]:
        nw = (bits + 1 + c - 1) // c  # msm_plan.h make_plan
        vals, bases = S.in_top_bucket_only(r, bases_fn, [(c * w, c) for w in range(nw)])
        _check(hip, cname, g2, vals, bases, (c,))
