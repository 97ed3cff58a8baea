"""GPU: the device field arithmetic element by element on DIRECTED operands (tests/directed_operands.py) against Python integers.

tests/test_host_math.py checks the arithmetic headers as the HOST compiler builds them. On the device FieldOps::mul / sqr / mul_add /
mul_inplace / mul_add_inplace_c of the 9- and 14-limb fields are the generated inline-asm blocks of mont_asm.hpp and goldilocks
multiplies with __umul64hi: code no host test reaches, and that the GPU suite otherwise sees only through whole MSMs / NTTs on random
data. Here tests/device_math_harness.hip runs the same case bodies as the host harness (tests/math_cases.hpp), one operand tuple per
thread, in two builds -- as shipped ("asm") and with -DBIGFIELD_NO_ASM ("noasm") -- and each is compared with the integers:
asm wrong and noasm right points at tools/gen_mont_asm.py or an operand list, both wrong and the host right at the compiler or a
device-only path, all three wrong at the header. Every launch writes its compiled-in variant tag, asserted on every call, so the
two libraries cannot silently be the same code.

  * canonical mode: every op x every directed pair (none left out) + 2000 seeded random pairs per field, exact, both builds;
  * raw mode: lazy representatives a0 + j*p with stated bounds; the header's written contract (limbs below 2^29, congruence, the bound
    computed with the tracker's r_over_p, exact reduce / cond_sub / is_zero / eq), and asm limbs == noasm limbs;
  * Fq2 (TIGHT mode for BN254), goldilocks, BabyBear / KoalaBear, and the EC tier (XYZZ accumulation, complete add / dbl, mul_small,
    the dbl_jac / dbl_jac_lazy chains) for the four G1 and three G2 curves; for bn254 and grumpkin the bucket-reduction loop on the
    signed layer (add_signed / signed_to_unsigned, ec_case op 7);
  * the quad tier: the four-lane (DPP quad) operations EcQuadAdd::add, EcDblSmallB::dbl_quad, EC::add_quad and EC::dbl_jac_quad, which
    no host build reaches, one sequence per quad and only for the curves the product instantiates each for -- the identity as an
    operand and as a sum, P + P, P + (-P), 2 O, the Horner walk of k_final_horner with cancelling window sums; every lane's result,
    every position of a quad in its wave, raw operands up to the bounds the headers state, and the one-lane twin each function's
    comment claims "the same values" for. Triage: both builds wrong and the one-lane twin right points at the quad schedule
    (a lane_select chain or a quad_bcast<SRC>), all wrong at the formula.
A missing library that cannot be built is a failure, not a skip.

Time: see MEASURED below; the Python integer reference is the cost, not the GPU."""
import ctypes
import os
import shutil
import subprocess

import pytest

from tests import math_expect as X

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
BUILD = os.path.join(HERE, "_build")
LIBS = {"asm": (os.path.join(BUILD, "libdevice_math_asm.so"), X.TAG_ASM), "noasm": (os.path.join(BUILD, "libdevice_math_noasm.so"), X.TAG_NOASM)}
# MEASURED on one MI355X: this module alone 12 s (27 tests, both builds). Inside the whole GPU suite, where it shares the host cores with
# the background reference jobs: 51 s of a 604 s suite (the other added tests: 3 s); the suite without the added tests took
# 570 s on the same machine that day (497 s at the last recorded run), so the 600 s budget is met only when the
# machine runs the old suite at its recorded speed. The integers are the cost (the kernels take milliseconds): expectations are computed once per field
# and shared by both builds, and a build whose raw-mode output is bit-identical to one already checked is not checked again.
# build(): the two harness libraries compile beside the product (a clean build() went from 5 min 27 s to 6 min 39 s on eight cores).
# With the quad tier, ec_case ops 7 / 8 and tests/test_gpu_msm_quad_reduce.py (parent commit and branch measured on the same day,
# an MI355X each, one run each): this module alone 13 s -> 15 s wall (27 tests, 10.9 s -> 46 tests, 12.6 s in pytest; the 19 added tests take under 2 s, none
# more than 0.5 s); the whole GPU suite 689 s -> 690 s wall
# (1297 tests, 686.7 s -> 1340 tests, 687.2 s in pytest). tests/test_gpu_msm_quad_reduce.py: 24 tests, 2 s. The added expectations are
# a few hundred integer group operations per curve, computed once (functools.lru_cache) and shared by both builds and every placement.
# build(): the harness gained one kernel per (curve, quad op) the product has -- a clean build() went from 6 min 45 s to 7 min 54 s -- and now
# also compiles the host twin with the bound tracker (g++, two minutes on one core, beside the rest).


def _stale(so):
    deps = [os.path.join(HERE, f) for f in ("device_math_harness.hip", "math_cases.hpp", "device_math.mk")]
    deps += [os.path.join(HERE, "..", "icicle_amd", "csrc", f) for f in ("bigfield.hpp", "mont_asm.hpp", "fq2.hpp", "ec.hpp", "ec_dbl_quad.hpp", "goldfield.hpp", "smallfield.hpp", "field_consts.h")]
    return not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps)


@pytest.fixture(scope="module")
def backends(hip):
    """both builds loaded into this process (after the product library: one HIP runtime), rebuilt when stale and a compiler is present"""
    if any(_stale(so) for so, _ in LIBS.values()) and (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        subprocess.check_call(["make", "-f", os.path.join(HERE, "device_math.mk"), "-j2"])
    out = {}
    for name, (so, tag) in LIBS.items():
        assert os.path.exists(so), f"{so} is missing and could not be built: run build() of __graft_entry__.py"
        out[name] = X.Backend(ctypes.CDLL(so), device=True, tag=tag, name=name)
    assert out["asm"].lib.dm_variant_tag() != out["noasm"].lib.dm_variant_tag()
    return out


def _both(backends, check, *args):
    """run one check on both builds; each must have had its own tag written by its own kernels"""
    res = {}
    for name, be in backends.items():
        before = be.tags_seen
        res[name] = check(be, *args)
        assert be.tags_seen > before, (name, "no launch carried the variant tag")
    return res


@pytest.mark.parametrize("f", list(range(11)))
def test_canonical(backends, f):
    """device (asm) == Python integers, then device (noasm) == Python integers, on all directed pairs and the random pairs, every op"""
    res = _both(backends, X.check_canon, f)
    if f == X.GOLD:
        extra = _both(backends, X.check_gold_noncanonical)
        res = {k: res[k] + extra[k] for k in res}
    ndir = X.canon_operands(f)[0]
    print(f"{X.FIELD_NAME[f]}: {ndir} directed pairs + {len(X.canon_operands(f)[1]) - ndir} random; (op, tuple) comparisons per build: {res}")
    assert res["asm"] == res["noasm"] > 0


@pytest.mark.parametrize("f", list(range(7)))
def test_raw(backends, f):
    """the lazy contract on the device: outputs of single ops on raw representatives near K*p, for every admissible stated bound"""
    res = _both(backends, X.check_raw, f)
    (na, oa), (nn, on) = res["asm"], res["noasm"]
    print(f"{X.FIELD_NAME[f]}: {na} raw tuples per build")
    assert na == nn > 0
    plan = X.raw_plan(f)
    for idx in oa:
        assert oa[idx] == on[idx], (X.FIELD_NAME[f], X.RAW_NAMES[plan[idx][0]], "K", plan[idx][1], "bounds", plan[idx][2], "asm and noasm limbs differ")


@pytest.mark.parametrize("fi", [0, 1])
def test_small_fields(backends, fi):
    res = _both(backends, X.check_small, fi)
    print(f"{X.SMALL[fi].name}: {res}")
    assert res["asm"] == res["noasm"] > 0


@pytest.mark.parametrize("ci", [0, 1, 2, 3, 4, 5, 6])
def test_ec_tier(backends, ci):
    """XYZZ accumulation (doubling, cancellation, identity branches), complete add / dbl, mul_small, the Jacobian doubling chains: one
    sequence per thread, against oracle/pyref.py's integer group law; op 7 (bn254, grumpkin): the loop of k_reduce_wave on the signed
    layer, add_signed from two identities and signed_to_unsigned, over directed bucket rows; op 8: EcDblSmallB::dbl chains"""
    res = _both(backends, X.check_ec, ci)
    print(f"curve {ci}: {res}")
    assert res["asm"] == res["noasm"] > 0
    assert (7 in X.ec_plan(ci)) == (ci in X.SIGNED_ADD) and (8 in X.ec_plan(ci)) == (ci in X.SMALL_B3)
    for be in backends.values():
        for op in X.ec_unsupported(ci):
            assert be.refuses("ec", ci, op), (ci, op, be.name, "a curve without this operation must answer -1")


@pytest.mark.parametrize("ci", [0, 1, 2, 3, 4, 5, 6])
def test_ec_quad_tier(backends, ci):
    """the four-lane operations on directed sequences, one per DPP quad: all four lanes store identical words, every coordinate is
    below q, the affine point is the integers', the identity comes out as (0 : y != 0 : 0), the words are those of the one-lane
    twin, both builds return identical words, and a (curve, op) pair the product does not instantiate answers -1"""
    res = _both(backends, X.check_ec_quad, ci)
    (na, oa, ta), (nn, on, tn) = res["asm"], res["noasm"]
    print(f"curve {ci}: (sequence) comparisons per build {({X.QUAD_NAME[op]: n for op, n in na.items()})}; words equal to the one-lane twin: "
          f"{({X.QUAD_NAME[op]: ok for op, ok in ta.items()})}")
    assert na == nn and sum(na.values()) > 0 and set(na) == {op for op in range(5) if ci in X.QUAD_CURVES[op]}
    assert all(ta.values()) and all(tn.values())
    for op in oa:
        assert oa[op] == on[op], (ci, X.QUAD_NAME[op], "asm and noasm words differ")


@pytest.mark.parametrize("ci", [0, 1, 2, 3, 4, 5, 6])
def test_ec_quad_placement(backends, ci):
    """a sequence gives the same words in each of the 16 quad positions of a wave, whatever its neighbours run, also in a launch whose last wave is partly empty"""
    res = _both(backends, X.check_ec_quad_placement, ci)
    print(f"curve {ci}: (sequence, placement) comparisons per build {({X.QUAD_NAME[op]: n for op, n in res['asm'].items()})}")
    assert res["asm"] == res["noasm"] and all(n == 256 + 261 for n in res["asm"].values())


@pytest.mark.parametrize("ci", [0, 1, 2, 4, 5])
def test_ec_quad_raw_bounds(backends, ci):
    """raw Montgomery representatives a0 + j p up to the bounds the headers state (additions <= 4 p, the doubling <= 8 p), each first
    accepted by the bound tracker on the one-lane twin of the host harness: integers, the host twin's words, asm == noasm"""
    res = _both(backends, X.check_ec_quad_raw, ci)
    (ra, oa), (rn, on) = res["asm"], res["noasm"]
    print(f"curve {ci}: (accepted bound, stated bound, cases) {({X.QUAD_NAME[op]: v for op, v in ra.items()})}")
    assert ra == rn and ra
    for op, (K, stated, n) in ra.items():
        assert K == stated and n > 0, (ci, X.QUAD_NAME[op], "the tracker refuses part of the range the header states", X.accepted_raw_bound(ci, op)[2])
        assert oa[op] == on[op], (ci, X.QUAD_NAME[op], "asm and noasm words differ")
