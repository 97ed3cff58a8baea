"""GPU parity of pass B's two routes (msm_impl.hpp): a partition of at most `own_max` elements is sorted whole by one block
(k_b_owned: histogram, scan and write cursors in LDS, count[] / offs[] written by the block), a larger one in sub-chunks
(k_b_plan / k_b_count / k_b_scan_part / k_b_scatter). MSMConfig.ext "hip_msm_passb_own_max" moves the boundary to sizes the
reference CPU backend finishes at once: 0 = nothing owned (the sequence before this route existed), absent = the default 2^18.
Every result is compared on affine limbs with the reference, as tests/test_gpu_msm.py::_check does; one reference run per input."""
import numpy as np
import pytest

from oracle import pyref, ref
from tests.util import cached_points, points_to_array, rand_scalars, to_words

pytestmark = pytest.mark.gpu
TS = 16384  # elements per tile of a 1024-thread sort block


def _run(hip, cname, sc, bases, own_max=None, windows=0, g2=False, **cfgkw):
    from icicle_amd import msm as M
    from icicle_amd._lib import lib

    cfg = hip.MSMConfig.default()
    for k, v in cfgkw.items():
        setattr(cfg, k, v)
    ext = lib.create_config_extension()
    if own_max is not None:
        lib.config_extension_set_int(ext, b"hip_msm_passb_own_max", own_max)
    if windows:
        lib.config_extension_set_int(ext, b"hip_msm_windows", windows)
    try:
        cfg.ext = ext
        return M.msm(cname, sc, bases, cfg, g2=g2)
    finally:
        lib.destroy_config_extension(ext)


def _routes(hip, refc, cname, sc, bases, own_maxes, exp=None, **kw):
    """every own_max of `own_maxes` (None = the default) against ONE reference result"""
    if exp is None:
        exp = refc.to_affine(refc.msm(sc, bases))
    for om in own_maxes:
        got = _run(hip, cname, sc, bases, own_max=om, **kw)
        assert np.array_equal(refc.to_affine(got), exp), f"{cname} own_max={om} {kw}"
        for g in got:
            assert refc.is_on_curve(g)
    return exp


def _tiled_bases(C, n, period=4096):
    pts = points_to_array(C, cached_points(C, min(n, period)))
    return np.ascontiguousarray(np.tile(pts, ((n + period - 1) // period, 1))[:n])


@pytest.mark.parametrize("cname", ["bn254", "bls12_381"])
def test_three_routes_give_the_same_answer(hip, cname):
    """c = 16: hb = 8, 256 partitions of ~256 elements per window. own_max 0: sub-chunks only; default: every partition owned;
    256: about half the partitions of every window on either route."""
    C = pyref.CURVES[cname]
    refc = ref.RefCurve(cname)
    rng = np.random.default_rng(7001)
    n = (1 << 16) - 5
    sc = to_words(rand_scalars(rng, n, C.r), 8)
    _routes(hip, refc, cname, sc, _tiled_bases(C, n), (0, None, 256), c=16)


def test_partition_of_exactly_own_max_elements_is_owned_and_one_more_is_not(hip):
    """c = 12 (hb = 6, lb = 5), scalars below 2^11: only window 0 is populated (but for the one r - 1), the digit is the scalar,
    partition h = (s - 1) >> 5. Partition 3 holds exactly K elements, partition 5 K + 1, partition 4 none; own_max = K."""
    C = pyref.BN254
    refc = ref.RefCurve("bn254")
    rng = np.random.default_rng(7002)
    K = 5000
    vals = [int(v) for v in rng.integers(3 * 32 + 1, 4 * 32 + 1, size=K)] + [int(v) for v in rng.integers(5 * 32 + 1, 6 * 32 + 1, size=K + 1)]
    assert all((v - 1) >> 5 == 3 for v in vals[:K]) and all((v - 1) >> 5 == 5 for v in vals[K:])
    vals = [vals[i] for i in rng.permutation(len(vals))] + [1, 0, C.r - 1]
    sc = to_words(vals, 8)
    _routes(hip, refc, "bn254", sc, _tiled_bases(C, len(vals)), (K, 0, None), c=12)


@pytest.mark.parametrize("spread", [False, True])
def test_tile_edges_inside_one_owned_partition(hip, spread):
    """partitions of exactly one tile, one tile + 1 and three tiles + 1 (c = 12 as above), all of a partition in ONE bin (one
    bucket list of that length) or spread over its 32 bins; default own_max: each is sorted whole by one block."""
    C = pyref.BN254
    refc = ref.RefCurve("bn254")
    rng = np.random.default_rng(7003)
    vals = []
    for h, size in ((2, TS), (7, TS + 1), (40, 3 * TS + 1)):
        lo = h * 32 + 1
        vals += [int(v) for v in rng.integers(lo, lo + 32, size=size)] if spread else [lo + 13] * size
    n = len(vals)
    assert n <= 1 << 17
    sc = to_words([vals[i] for i in rng.permutation(n)], 8)
    _routes(hip, refc, "bn254", sc, _tiled_bases(C, n), (None,), c=12)


@pytest.mark.parametrize("cname", ["bn254", "bls12_381"])
def test_2048_bins_two_per_thread(hip, cname):
    """c = 22: pass B ranks into 2^11 bins, two per thread of the block; uniform scalars, then half of them in {1, 2} (two hot
    buckets of one partition: with own_max = 64 that partition takes the sub-chunk route beside owned ones)."""
    from icicle_amd import msm as M

    C = pyref.CURVES[cname]
    refc = ref.RefCurve(cname)
    rng = np.random.default_rng(7004)
    n = (1 << 18) - 7
    bases = M.generate_affine_points(cname, n, k0=31337)
    sc = to_words(rand_scalars(rng, n, C.r), 8)
    _routes(hip, refc, cname, sc, bases, (None, 64), c=22)
    sc[: n // 2, 1:] = 0
    sc[: n // 2, 0] = rng.integers(1, 3, size=n // 2)
    _routes(hip, refc, cname, sc, bases, (None, 64), c=22)


@pytest.mark.parametrize("nwin", [12, 13])
def test_mixed_window_widths_own_the_empty_upper_halves(hip, nwin):
    """a narrow window uses the lower half of its bucket slot: the partitions of the upper half are empty and go through the
    owned route, which must still write their count[] / offs[]. Edge scalars of test_msm_mixed_window_widths, one identity base."""
    C = pyref.BN254
    refc = ref.RefCurve("bn254")
    rng = np.random.default_rng(7005 + nwin)
    n = 5000
    pts = list(cached_points(C, n))
    pts[3] = pyref.INF
    bases = points_to_array(C, pts)
    vals = rand_scalars(rng, n, C.r)
    top = C.r.bit_length() - 1
    edge = [C.r - 1, C.r - 2, (1 << top), (1 << top) - 1, (1 << top) + 1, 0, 1, 2, (1 << (top - 1)), C.r // 2, C.r // 2 + 1, ((1 << top) - 1) // 3]
    for k, v in enumerate(edge):
        vals[10 + k] = v % C.r
    _routes(hip, refc, "bn254", to_words(vals, 8), bases, (None, 8), windows=nwin)


@pytest.mark.parametrize("kind", ["all_equal", "half_equal", "all_zero"])
def test_skewed_scalars(hip, kind):
    C = pyref.BN254
    refc = ref.RefCurve("bn254")
    rng = np.random.default_rng(7006)
    n = (1 << 14) + 3
    vals = rand_scalars(rng, n, C.r)
    hot = vals[0]
    if kind == "all_equal":
        vals = [hot] * n
    elif kind == "half_equal":
        vals = [hot if i % 2 else v for i, v in enumerate(vals)]
    else:
        vals = [0] * n
    _routes(hip, refc, "bn254", to_words(vals, 8), _tiled_bases(C, n), (None, 0, 100), c=13)


def test_hot_partition_above_the_default_own_max_beside_owned_ones(hip):
    """n = 2^19 + 3, c = 16: every second scalar is the same, so one partition of every window holds more than 2^18 elements --
    not owned with the default own_max, cut into sub-chunks, its bucket into overflow segments -- beside 255 owned ones."""
    from icicle_amd import msm as M

    C = pyref.BN254
    refc = ref.RefCurve("bn254")
    rng = np.random.default_rng(7007)
    n = (1 << 19) + 3
    sc = to_words(rand_scalars(rng, n, C.r), 8)
    sc[1::2] = sc[1]
    assert (n // 2) > (1 << 18)
    bases = M.generate_affine_points("bn254", n, k0=2718)
    _routes(hip, refc, "bn254", sc, bases, (None,), c=16)


def test_batches_index_partitions_through_the_folded_windows(hip):
    """batch 3 at n = 2^13, c = 13, shared and per-MSM bases: the MSMs of a batch are folded into the window dimension"""
    C = pyref.BN254
    refc = ref.RefCurve("bn254")
    rng = np.random.default_rng(7008)
    n, batch = 1 << 13, 3
    sc = to_words(rand_scalars(rng, n * batch, C.r), 8)
    bases = _tiled_bases(C, n * batch)
    for shared in (True, False):
        b = np.ascontiguousarray(bases[:n]) if shared else bases
        exp = refc.to_affine(refc.msm(sc, b, batch=batch, shared=shared))
        _routes(hip, refc, "bn254", sc, b, (None, 40), exp=exp, c=13, batch_size=batch, are_points_shared_in_batch=shared)


def test_precompute_factor_two(hip):
    from icicle_amd import msm as M

    C = pyref.BN254
    refc = ref.RefCurve("bn254")
    rng = np.random.default_rng(7009)
    n = 1 << 14
    bases = _tiled_bases(C, n)
    sc = to_words(rand_scalars(rng, n, C.r), 8)
    cfg = hip.MSMConfig.default()
    cfg.precompute_factor, cfg.c = 2, 14
    table = M.precompute_bases("bn254", bases, cfg)
    exp = refc.to_affine(refc.msm(sc, bases))
    _routes(hip, refc, "bn254", sc, table, (None, 300), exp=exp, c=14, precompute_factor=2)


def test_device_resident_async_twice_on_one_stream(hip):
    from icicle_amd import msm as M
    from icicle_amd.runtime import DeviceVec, Stream

    C = pyref.BN254
    refc = ref.RefCurve("bn254")
    rng = np.random.default_rng(7010)
    n = 1 << 14
    bases = _tiled_bases(C, n)
    sc = [to_words(rand_scalars(rng, n, C.r), 8) for _ in range(2)]
    d_b = DeviceVec.from_host(bases)
    d_sc = [DeviceVec.from_host(s) for s in sc]
    d_res = [DeviceVec(3 * C.limbs_q * 4) for _ in range(2)]
    st = Stream()
    cfg = hip.MSMConfig.default()
    cfg.stream, cfg.is_async, cfg.c = st.handle, True, 14
    for i in range(2):  # back to back, no synchronisation between them
        M.msm("bn254", d_sc[i], d_b, cfg, results=d_res[i], msm_size=n)
    st.synchronize()
    for i in range(2):
        got = d_res[i].to_host(shape=(1, 3 * C.limbs_q))
        assert np.array_equal(refc.to_affine(got), refc.to_affine(refc.msm(sc[i], bases))), i
    st.destroy()


def test_g2(hip):
    from icicle_amd import msm as M

    C = pyref.BN254
    refc = ref.RefCurve("bn254", g2=True)
    rng = np.random.default_rng(7011)
    n = 1 << 12
    bases = M.generate_affine_points("bn254", n, k0=4711, g2=True)
    sc = to_words(rand_scalars(rng, n, C.r), 8)
    _routes(hip, refc, "bn254", sc, bases, (None, 70), c=12, g2=True)


def test_two_window_groups_in_a_child_process(hip):
    """ICICLE_HIP_MSM_GROUPS is read once per process: a child runs the pipelined schedule with two window groups, whose
    stand-alone sorts reach k_b_owned through the group's first partition and partition count"""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r"""
import sys, numpy as np
sys.path.insert(0, %r)
import icicle_amd as hip
from icicle_amd import msm as M, runtime
from oracle import pyref, ref
from tests.util import cached_points, points_to_array, rand_scalars, to_words
runtime.set_device(0)
C = pyref.BN254
refc = ref.RefCurve("bn254")
rng = np.random.default_rng(7012)
n = (1 << 15) - 3
pts = points_to_array(C, cached_points(C, 4096))
bases = np.ascontiguousarray(np.tile(pts, (8, 1))[:n])
sc = to_words(rand_scalars(rng, n, C.r), 8)
cfg = hip.MSMConfig.default()
cfg.c = 14
got = M.msm("bn254", sc, bases, cfg)
assert np.array_equal(refc.to_affine(got), refc.to_affine(refc.msm(sc, bases)))
print("GROUPS OK")
""" % root
    env = dict(os.environ)
    env["ICICLE_HIP_MSM_GROUPS"] = "2"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300, cwd=root)
    assert r.returncode == 0 and "GROUPS OK" in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]
