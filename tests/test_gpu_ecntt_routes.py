"""GPU parity of <curve>_ecntt on the routes that large transforms take (icicle_amd/csrc/ecntt.hip ecntt_run, decided by
ntt_plan.h ecntt_route): the radix-2 kernel k_ecntt_stage in its natural band, with its tables in LDS and in global memory, and
k_ecntt_scale with its tables in global memory -- on bn254, bls12_381 and bls12_377, each at the smallest shape that reaches the route:
16-point transforms, and an odd batch that leaves the last block partly filled.

Inputs: the 37 distinct transforms of tests/ecntt_inputs.py tiled over the batch (transform b = distinct[b % 37]); the reference CPU
backend computes the 37 once per configuration and the expectation is that result tiled in the call's layout. Every output is compared
as a group element, on to_affine() limbs; transforms 0..10 also against NTT(k)_i G in Python integers. Every test asserts the route it
means to reach with icicle_hip_ecntt_plan_info before it compares anything."""
import ctypes

import numpy as np
import pytest

from oracle import pyref, ref
from tests import ecntt_inputs as EI

pytestmark = pytest.mark.gpu
CURVES = ["bn254", "bls12_381", "bls12_377"]
POINT_BYTES = {"bn254": 108, "bls12_381": 168, "bls12_377": 168}  # a point in the kernels' form: 3 x 9 / 3 x 14 words
N = EI.N
ORD, FORWARD_CALL, INVERSE_CALL = EI.ORD, EI.FORWARD_CALL, EI.INVERSE_CALL


def plan_info(hip, cname, size, batch, inverse, coset):
    """icicle_hip_ecntt_plan_info as a dict: what this process would launch for the call"""
    from icicle_amd._lib import lib

    out = (ctypes.c_int * 40)()
    assert lib.icicle_hip_ecntt_plan_info(POINT_BYTES[cname], size, batch, inverse, coset, out) == 0
    return dict(widths=list(out[5:5 + out[0]]), rmax=out[1], stage_gtab=out[2], scale_runs=out[3], scale_gtab=out[4])


MATRIX = dict(widths=[4], rmax=4, stage_gtab=0, scale_runs=1, scale_gtab=0)
RADIX2_LDS = dict(widths=[1, 1, 1, 1], rmax=1, stage_gtab=0, scale_runs=1, scale_gtab=0)
RADIX2_GLOBAL = dict(widths=[1, 1, 1, 1], rmax=1, stage_gtab=1, scale_runs=1, scale_gtab=1)


def shapes(cname):
    """(batch, expected route): tot = 592, 11216 (the radix-2 band below 2^14 points), 32816 / 40976 (more quads than LDS tables allow)"""
    return {"matrix": (37, MATRIX), "radix2_lds": (701, RADIX2_LDS), "radix2_global": (2561 if cname == "bn254" else 2051, RADIX2_GLOBAL)}


@pytest.fixture(scope="module", params=CURVES)
def env(request, hip):
    from icicle_amd import ntt as NT

    cname = request.param
    C = pyref.CURVES[cname]
    sf = ref.RefScalarNttField(cname)
    refc = ref.RefCurve(cname)
    root = NT.get_root_of_unity(cname, N)
    NT.init_domain(cname, root)
    sf.init_domain(root)
    slots, scalars = EI.transforms(cname)
    x = np.stack([EI.words(C, s) for s in slots])  # [37, 16, 3 L]
    L = C.limbs_q
    e = dict(cname=cname, C=C, L=L, refc=refc, NT=NT, x=x, scalars=scalars,
             x_affine=np.stack([EI.affine_words(C, [p for p, _ in s]) for s in slots]), expected={})

    def expected(call):
        """the 37 transforms under one call configuration, computed once: (reference [37, 16, 2 L], Python ground truth [11, 16, 2 L])"""
        if call not in e["expected"]:
            direction, ordering, columns, coset = call
            xin = EI.tile(x, EI.COUNT, columns).reshape(-1)
            y = refc.ecntt(xin, N, direction, batch=EI.COUNT, columns_batch=columns, ordering=ordering, coset_gen=coset)
            aff = refc.to_affine(y.reshape(-1, 3 * L)).reshape((N, EI.COUNT, 2 * L) if columns else (EI.COUNT, N, 2 * L))
            if columns:
                aff = aff.transpose(1, 0, 2)
            truth = np.stack([EI.expected_from_scalars(cname, ks, bool(direction), ORD[ordering], coset) for ks in scalars])
            assert np.array_equal(aff[:EI.KNOWN], truth)  # the two ground truths agree (tests/test_oracle.py, on the CPU, says the same)
            e["expected"][call] = (np.ascontiguousarray(aff), truth)
        return e["expected"][call]

    e["expect"] = expected
    yield e
    NT.release_domain(cname)
    sf.release_domain()


def check_outputs(e, got_words, call, batch):
    """every output of the call, as a group element, against the reference's 37 tiled in the call's layout; transforms 0..10 also
    against NTT(k)_i G"""
    _, _, columns, _ = call
    exp, truth = e["expect"](call)
    got = e["refc"].to_affine(got_words.reshape(-1, 3 * e["L"]))
    want = EI.tile(exp, batch, columns)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (e["cname"], call, batch, "first wrong points (memory index):", bad[:8].tolist(), "of", bad.size)
    per_t = got.reshape((N, batch, -1)).transpose(1, 0, 2) if columns else got.reshape(batch, N, -1)
    known = np.flatnonzero(np.arange(batch) % EI.COUNT < EI.KNOWN)
    assert np.array_equal(per_t[known], truth[known % EI.COUNT])


def config(hip, call, batch):
    direction, ordering, columns, coset = call
    cfg = hip.NTTConfigU256.default()
    cfg.batch_size, cfg.columns_batch, cfg.ordering = batch, columns, ordering
    cfg.set_coset_gen(coset)
    return cfg


@pytest.mark.parametrize("shape", ["matrix", "radix2_lds", "radix2_global"])
def test_ecntt_forward_coset_rows_on_route(env, hip, shape):
    """forward, kNR, rows, coset generator != 1 (k_ecntt_scale mode 1 in front of the stages). Routes, asserted: `matrix` -- one
    matrix-form stage of width 4 (k_ecntt_terms / k_ecntt_sums), the structured inputs on the default route; `radix2_lds` -- tot = 11216,
    k_ecntt_stage in its natural band below 2^14 points, stage and scale tables in LDS; `radix2_global` -- tot = 32816 (BLS) / 40976
    (bn254), k_ecntt_stage and k_ecntt_scale with their quads' tables in global memory (gtabs)."""
    e = env
    batch, route = shapes(e["cname"])[shape]
    assert plan_info(hip, e["cname"], N, batch, False, True) == route
    x = EI.tile(e["x"], batch, False).reshape(-1)
    got = e["NT"].ecntt(e["cname"], x, e["NT"].FORWARD, config(hip, FORWARD_CALL, batch))
    check_outputs(e, got, FORWARD_CALL, batch)


@pytest.mark.parametrize("shape", ["matrix", "radix2_lds", "radix2_global"])
def test_ecntt_inverse_coset_columns_on_route(env, hip, shape):
    """inverse, kRN, columns_batch, coset generator != 1 (k_ecntt_scale mode 2 behind the stages: 1 / N with the coset folded in), on
    the same three routes, asserted: one matrix-form stage of width 4; k_ecntt_stage with LDS tables (tot = 11216); k_ecntt_stage and
    k_ecntt_scale with global tables (tot = 32816 / 40976). On the last the call is device resident and in place (output pointer = input
    pointer), is_async on a created stream that is synchronised before the copy back; the opposite call -- forward, kNR, the same coset --
    applied to the device output must then give the input back as group elements for every point, which needs no reference."""
    from icicle_amd.runtime import DeviceVec, Stream

    e = env
    NT = e["NT"]
    batch, route = shapes(e["cname"])[shape]
    assert plan_info(hip, e["cname"], N, batch, True, True) == route
    x = EI.tile(e["x"], batch, True).reshape(-1)
    cfg = config(hip, INVERSE_CALL, batch)
    if shape != "radix2_global":
        check_outputs(e, NT.ecntt(e["cname"], x, NT.INVERSE, cfg), INVERSE_CALL, batch)
        return
    stream = Stream()
    d = DeviceVec.from_host(x)
    try:
        cfg.stream, cfg.is_async = stream.handle, True
        NT.ecntt(e["cname"], d, NT.INVERSE, cfg, out=d, size=N)
        stream.synchronize()
        check_outputs(e, d.to_host(), INVERSE_CALL, batch)
        # back: forward kNR with the same coset undoes inverse kRN; the same route (asserted), the scale pass now in front
        assert plan_info(hip, e["cname"], N, batch, False, True) == route
        back = config(hip, (0, 1, True, INVERSE_CALL[3]), batch)
        back.stream, back.is_async = stream.handle, True
        NT.ecntt(e["cname"], d, NT.FORWARD, back, out=d, size=N)
        stream.synchronize()
        got = e["refc"].to_affine(d.to_host().reshape(-1, 3 * e["L"]))
        assert np.array_equal(got, EI.tile(e["x_affine"], batch, True))
    finally:
        d.free()
        stream.destroy()
