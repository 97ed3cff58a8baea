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
    the dbl_jac / dbl_jac_lazy chains) for the four G1 and three G2 curves.
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


def _stale(so):
    deps = [os.path.join(HERE, f) for f in ("device_math_harness.hip", "math_cases.hpp", "device_math.mk")]
    deps += [os.path.join(HERE, "..", "icicle_amd", "csrc", f) for f in ("bigfield.hpp", "mont_asm.hpp", "fq2.hpp", "ec.hpp", "goldfield.hpp", "smallfield.hpp", "field_consts.h")]
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
    sequence per thread, against oracle/pyref.py's integer group law"""
    res = _both(backends, X.check_ec, ci)
    print(f"curve {ci}: {res}")
    assert res["asm"] == res["noasm"] > 0
