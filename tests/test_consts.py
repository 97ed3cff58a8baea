"""CPU: the generated device constants (icicle_amd/csrc/field_consts.h) are derived from the published
moduli; every modulus / generator / root of unity is cross-checked against the values the reference headers
hold. Those values are stored in tests/golden/reference_constants.json (read from the headers by
`python -m tests.test_consts`), so the check runs without the reference tree; where the tree is present the
fixture is first checked against the headers themselves."""
import json
import os
import re

from oracle import pyref

REF = os.path.join(os.environ.get("ICICLE_REFERENCE_DIR", "/root/reference"), "icicle", "include", "icicle")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_constants.json")


def _limbs(text, name):
    m = re.search(name + r"\s*=\s*\{([^}]*)\}", text)
    vals = [int(v, 16) for v in re.findall(r"0x[0-9a-fA-F]+", m.group(1))]
    return sum(v << (32 * i) for i, v in enumerate(vals))


def _header_constants(ref):
    """the constants this test pins, read from the reference headers under `ref`: name -> int or bool"""
    def rd(path):
        with open(os.path.join(ref, path)) as f:
            return f.read()

    k = {}
    t = rd("fields/snark_fields/bn254_base.h")
    k["bn254.q"] = _limbs(t, r"storage<8> modulus")
    t = rd("fields/snark_fields/bn254_scalar.h")
    k["bn254.r"] = _limbs(t, r"storage<8> modulus")
    k["bn254.fr_rou"] = _limbs(t, r"storage<8> rou")
    t = rd("fields/snark_fields/bls12_381_base.h")
    k["bls12_381.q"] = _limbs(t, r"storage<12> modulus")
    t = rd("fields/snark_fields/bls12_381_scalar.h")
    k["bls12_381.r"] = _limbs(t, r"storage<8> modulus")
    t = rd("curves/params/bls12_381.h")
    k["bls12_381.gx"] = _limbs(t, r"point_field_t gen_x")
    k["bls12_381.gy"] = _limbs(t, r"point_field_t gen_y")
    t = rd("curves/params/bn254.h")
    k["bn254.gx"] = _limbs(t, r"point_field_t gen_x")
    k["bn254.gy"] = _limbs(t, r"point_field_t gen_y")
    k["bn254.b"] = _limbs(t, r"point_field_t weierstrass_b")
    t = rd("fields/snark_fields/bls12_377_base.h")
    k["bls12_377.q"] = _limbs(t, r"storage<12> modulus")
    k["bls12_377.fq2_nonresidue_is_5"] = bool(re.search(r"nonresidue = 5;", t))
    k["bls12_377.fq2_nonresidue_is_negative"] = bool(re.search(r"nonresidue_is_negative = true", t))
    t = rd("fields/snark_fields/bls12_377_scalar.h")
    k["bls12_377.r"] = _limbs(t, r"storage<8> modulus")
    k["bls12_377.fr_rou"] = _limbs(t, r"storage<8> rou")
    t = rd("curves/params/bls12_377.h")
    k["bls12_377.gx"] = _limbs(t, r"point_field_t gen_x")
    k["bls12_377.gy"] = _limbs(t, r"point_field_t gen_y")
    k["bls12_377.b"] = _limbs(t, r"point_field_t weierstrass_b")
    for n in ("g2_gen_x_re", "g2_gen_x_im", "g2_gen_y_re", "g2_gen_y_im", "weierstrass_b_g2_re", "weierstrass_b_g2_im"):
        k[f"bls12_377.{n}"] = _limbs(t, r"point_field_t " + n)
    t = rd("curves/params/grumpkin.h")  # base field = bn254's scalar field and vice versa (grumpkin_{base,scalar}.h)
    k["grumpkin.gx"] = _limbs(t, r"point_field_t gen_x")
    k["grumpkin.gy"] = _limbs(t, r"point_field_t gen_y")
    k["grumpkin.b_is_negative"] = bool(re.search(r"is_b_neg = true", t))
    k["grumpkin.b_magnitude"] = _limbs(t, r"\n\s*static constexpr point_field_t weierstrass_b")
    k["grumpkin.base_is_bn254_fr"] = "bn254::fp_config fq_config" in rd("fields/snark_fields/grumpkin_base.h")
    k["grumpkin.scalar_is_bn254_fq"] = "bn254::fq_config fp_config" in rd("fields/snark_fields/grumpkin_scalar.h")
    t = rd("fields/stark_fields/stark252.h")
    k["stark252.p"] = _limbs(t, r"storage<8> modulus")
    k["stark252.rou"] = _limbs(t, r"storage<8> rou")
    for h in ("babybear", "koalabear"):
        t = rd(f"fields/stark_fields/{h}.h")
        k[f"{h}.p"] = _limbs(t, r"storage<1> modulus")
        k[f"{h}.rou"] = _limbs(t, r"storage<1> rou")
    return k


def _load_golden():
    with open(GOLDEN) as f:
        return {n: v if isinstance(v, bool) else int(v, 16) for n, v in json.load(f).items()}


def test_constants_match_reference_headers():
    k = _load_golden()
    if os.path.isdir(REF):  # the fixture must still say what the headers say
        assert _header_constants(REF) == k
    assert k["bn254.q"] == pyref.BN254.q
    assert k["bn254.r"] == pyref.BN254.r
    assert k["bn254.fr_rou"] == pyref.BN254_FR.rou
    assert k["bls12_381.q"] == pyref.BLS12_381.q
    assert k["bls12_381.r"] == pyref.BLS12_381.r
    assert k["bls12_381.gx"] == pyref.BLS12_381.gx
    assert k["bls12_381.gy"] == pyref.BLS12_381.gy
    assert k["bn254.gx"] == 1 and k["bn254.gy"] == 2
    assert k["bn254.b"] == 3
    assert k["bls12_377.q"] == pyref.BLS12_377.q
    assert k["bls12_377.fq2_nonresidue_is_5"] and k["bls12_377.fq2_nonresidue_is_negative"]  # Fq2 = Fq[u]/(u^2 + 5)
    assert k["bls12_377.r"] == pyref.BLS12_377.r
    assert k["bls12_377.fr_rou"] == pyref.BLS12_377_FR.rou
    assert k["bls12_377.gx"] == pyref.BLS12_377.gx and k["bls12_377.gy"] == pyref.BLS12_377.gy
    assert k["bls12_377.b"] == pyref.BLS12_377.b == 1
    g2 = pyref.BLS12_377_G2
    assert (k["bls12_377.g2_gen_x_re"], k["bls12_377.g2_gen_x_im"]) == g2.gx
    assert (k["bls12_377.g2_gen_y_re"], k["bls12_377.g2_gen_y_im"]) == g2.gy
    assert (k["bls12_377.weierstrass_b_g2_re"], k["bls12_377.weierstrass_b_g2_im"]) == g2.b
    assert k["grumpkin.gx"] == pyref.GRUMPKIN.gx and k["grumpkin.gy"] == pyref.GRUMPKIN.gy
    assert k["grumpkin.b_is_negative"] and k["grumpkin.b_magnitude"] == pyref.GRUMPKIN.q - pyref.GRUMPKIN.b == 17
    assert k["grumpkin.base_is_bn254_fr"] and k["grumpkin.scalar_is_bn254_fq"]
    assert k["stark252.p"] == pyref.STARK252.p and k["stark252.rou"] == pyref.STARK252.rou
    for f, h in ((pyref.BABYBEAR, "babybear"), (pyref.KOALABEAR, "koalabear")):
        assert k[f"{h}.p"] == f.p
        assert k[f"{h}.rou"] == f.rou


def test_generated_header_is_current(tmp_path):
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "field_consts.h"
    subprocess.check_call([sys.executable, os.path.join(root, "tools", "gen_consts.py"), str(out)])
    assert out.read_text() == open(os.path.join(root, "icicle_amd", "csrc", "field_consts.h")).read()


def test_curve_and_field_parameters_are_consistent():
    for c in (pyref.BN254, pyref.BLS12_381, pyref.BLS12_377, pyref.GRUMPKIN):
        g = (c.gx, c.gy)
        assert pyref.on_curve(c, g)
        assert pyref.ec_mul(c, c.r - 1, g) == pyref.ec_neg(c, g)  # r*G = identity
    g2 = pyref.BLS12_377_G2
    assert pyref.g2_on_curve(g2, (g2.gx, g2.gy)) and pyref.g2_mul(g2, g2.base.r - 1, (g2.gx, g2.gy)) == pyref.g2_neg(g2, (g2.gx, g2.gy))
    for f in (pyref.BABYBEAR, pyref.KOALABEAR, pyref.BN254_FR, pyref.BLS12_377_FR, pyref.STARK252):
        assert pow(f.rou, 1 << f.two_adicity, f.p) == 1 and pow(f.rou, 1 << (f.two_adicity - 1), f.p) == f.p - 1


if __name__ == "__main__":  # (re)mint tests/golden/reference_constants.json from the reference headers
    with open(GOLDEN, "w") as f:
        json.dump({n: v if isinstance(v, bool) else hex(v) for n, v in _header_constants(REF).items()}, f, indent=1)
        f.write("\n")
