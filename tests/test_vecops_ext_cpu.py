"""CPU: the extension-field vector operations (babybear, koalabear, goldilocks; twelve functions each).

* tests/vecops_ext_model.py, the fields in Python integers, inverts two ways and equals the reference's recorded results
  (tests/golden/vecops_ext_vectors.json, minted by tests/golden/mint_vecops_ext_vectors.py) on every case of all 36 functions;
* icicle_amd/csrc/vecops_ext_elem.hpp, the code a lane runs, compiled with g++ into a program of its own
  (tests/vecops_ext_host_harness.cpp), reproduces every recorded case and 10^4 seeded random identities per field, plainly and under
  -fsanitize=address,undefined;
* the C ABI's surface: header, library, binding, argument checks before any device call, the tile query, no fall-back."""
import ctypes
import functools
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests import vecops_ext_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIXTURE = os.path.join(HERE, "golden", "vecops_ext_vectors.json")
NARGS = {"vector_add": 5, "vector_sub": 5, "vector_mul": 5, "vector_div": 5, "vector_mixed_mul": 5, "vector_inv": 4, "vector_sum": 4,
         "vector_product": 4, "scalar_add_vec": 5, "scalar_sub_vec": 5, "scalar_mul_vec": 5, "bit_reverse": 4}
INVALID_POINTER, INVALID_ARGUMENT = 3, 11


@functools.lru_cache(maxsize=None)
def fixture():
    with open(FIXTURE) as fh:
        return json.load(fh)


def model_out(c):
    f, op = c["field"], c["op"]
    a = M.from_hex(f, c["a"])
    if c["b"] is None:
        b = None
    elif op == "vector_mixed_mul":
        raw = bytes.fromhex(c["b"])
        cb = 4 * M.BASE_WORDS[f]
        b = [int.from_bytes(raw[i:i + cb], "little") for i in range(0, len(raw), cb)]
    else:
        b = M.from_hex(f, c["b"])
    return M.to_hex(f, M.run(f, op, a, b, c["size"], c["batch"], c["columns"]))


# ---- the model ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", M.FIELDS)
def test_model_inverts_the_same_two_ways(f):
    p, d = M.modulus(f), M.DEGREE[f]
    rng = np.random.default_rng(77)
    elems = [M.one(f), tuple([p - 1] * d), (0, 1) + (0,) * (d - 2), (0,) * (d - 1) + (1,), (2,) + (0,) * (d - 1)]
    elems += [tuple(int(v) % p for v in rng.integers(0, 1 << 63, size=d)) for _ in range(4)]
    for a in elems:
        ia = M.inv(f, a)
        assert M.mul(f, a, ia) == M.one(f), a
        assert ia == M.inv_fermat(f, a), a
    assert M.inv(f, M.zero(f)) == M.zero(f) == M.inv_fermat(f, M.zero(f))
    assert M.mul(f, (0, 1) + (0,) * (d - 2), (0,) * (d - 1) + (1,)) == M.embed(f, M.NONRES[f])  # x * x^(d-1) = W


def test_fixture_covers_all_36_functions_and_records_the_zero_rule():
    doc = fixture()
    assert {(c["field"], c["op"]) for c in doc["cases"]} == {(f, op) for f in M.FIELDS for op in NARGS}
    assert all(doc["rules"][f]["inverse_of_zero_is_zero"] is True for f in M.FIELDS)
    assert os.path.getsize(FIXTURE) < 512 * 1024
    for c in doc["cases"]:
        assert set(c) == {"field", "op", "size", "batch", "columns", "a", "b", "out"}  # data only
        assert 5 <= len(c["a"]) // 32 <= 40 or c["op"].startswith("scalar_"), (c["field"], c["op"])
    for f in M.FIELDS:  # batch_size 3 with and without columns_batch for sum, product and the scalar operations
        for op in ("vector_sum", "vector_product", "scalar_add_vec", "scalar_sub_vec", "scalar_mul_vec"):
            assert {c["columns"] for c in doc["cases"] if (c["field"], c["op"], c["batch"]) == (f, op, 3)} == {False, True}, (f, op)


@pytest.mark.parametrize("f", M.FIELDS)
def test_model_equals_the_reference_on_every_recorded_case(f):
    cases = [c for c in fixture()["cases"] if c["field"] == f]
    assert len(cases) >= 30
    for c in cases:
        assert model_out(c) == c["out"], (f, c["op"], c["size"], c["batch"], c["columns"])


# ---- vecops_ext_elem.hpp on the host ------------------------------------------------------------------------------------------------
def build_harness(name, flags):
    exe = os.path.join(HERE, "_build", name)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    src = os.path.join(HERE, "vecops_ext_host_harness.cpp")
    deps = [src] + [os.path.join(ROOT, "icicle_amd", "csrc", h) for h in ("vecops_ext_elem.hpp", "smallfield.hpp", "goldfield.hpp", "bigfield.hpp", "field_consts.h")]
    if not os.path.exists(exe) or max(os.path.getmtime(d) for d in deps) > os.path.getmtime(exe):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wno-unknown-pragmas", *flags, src, "-o", exe])
    return exe


def run_harness(exe, tmp_path):
    path = os.path.join(str(tmp_path), "cases.txt")
    with open(path, "w") as fh:
        for c in fixture()["cases"]:
            fh.write(f"{c['field']} {c['op']} {c['size']} {c['batch']} {int(c['columns'])} {c['a']} {c['b'] or '-'} {c['out']}\n")
    r = subprocess.run([exe, "cases", path], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip().endswith(f"cases {len(fixture()['cases'])} mismatches 0"), r.stdout[-500:]
    r = subprocess.run([exe, "random", "20251", "10000", "50"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == "random 10000 per field, failures 0"
    assert len(lines) == 151
    for line in lines[:-1]:  # the pairs the program printed, against the model
        f, *hexes = line.split()
        a, b, ab, ia = (M.from_words(f, np.array([int(h[8 * k:8 * k + 8], 16) for k in range(4)], np.uint32))[0] for h in hexes)
        assert M.mul(f, a, b) == ab and M.inv(f, a) == ia, line


def test_lane_code_reproduces_the_fixture_and_the_random_identities(tmp_path):
    run_harness(build_harness("vecops_ext_host_harness", []), tmp_path)


def test_lane_code_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """the same program, instrumented: a finding makes it exit non-zero with a report on stderr"""
    run_harness(build_harness("vecops_ext_host_harness_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan"]), tmp_path)


# ---- header, library, binding ------------------------------------------------------------------------------------------------------
def test_functions_are_declared_exported_and_bound():
    from icicle_amd import _lib
    import icicle_amd

    text = re.sub(r"\s+", " ", subprocess.check_output(["gcc", "-E", "-P", os.path.join(ROOT, "include", "icicle_hip.h")], text=True))
    assert set(NARGS) == set(_lib.EXT_VEC_OPS_2 + _lib.EXT_VEC_OPS_1)
    for f in M.FIELDS:
        for name, n in NARGS.items():
            m = re.search(r"icicle_error_t %s_extension_%s\s*\(([^)]*)\)\s*;" % (f, name), text)
            assert m and len(m.group(1).split(",")) == n, (f, name)
            assert f"{f}_extension_{name}" in _lib.API_SYMBOLS and len(getattr(_lib.lib, f"{f}_extension_{name}").argtypes) == n
            assert f"icicle_hip_{f}_extension_{name}" not in text and not hasattr(_lib.lib, f"icicle_hip_{f}_extension_{name}")  # no aliases
    for absent in ("vector_accumulate", "slice", "execute_program", "generate_program"):
        assert not re.search(r"\w+_extension_%s\b" % absent, text), absent
    for f in ("bn254", "bls12_381", "bls12_377", "stark252", "grumpkin"):
        assert f"{f}_extension_vector" not in text and not hasattr(_lib.lib, f"{f}_extension_vector_add")
    m = re.search(r"int icicle_hip_extension_vector_inv_tile\s*\(([^)]*)\)\s*;", text)
    assert m and len(m.group(1).split(",")) == 1
    assert "icicle_hip_extension_vector_inv_tile" in _lib.API_SYMBOLS and len(_lib.lib.icicle_hip_extension_vector_inv_tile.argtypes) == 1
    assert callable(icicle_amd.vector_mixed_mul) and icicle_amd.vector_mixed_mul is icicle_amd.vecops.vector_mixed_mul
    assert "vector_mixed_mul" in icicle_amd.__all__


def test_tile_query():
    from icicle_amd import vecops as V
    from icicle_amd._lib import lib

    for words in (1, 2):
        assert lib.icicle_hip_extension_vector_inv_tile(words) >= 64, words
    for words in (0, 3, 4, -1):
        assert lib.icicle_hip_extension_vector_inv_tile(words) == 0, words
    for f in M.FIELDS:
        assert V.extension_vector_inv_tile(f) == lib.icicle_hip_extension_vector_inv_tile(M.BASE_WORDS[f])
    assert lib.icicle_hip_vector_inv_tile(4) == 0  # the base query keeps its answer


@pytest.mark.parametrize("f", M.FIELDS)
def test_argument_checks_need_no_device(f):
    """NULL config, then size == 0 (success, nothing written), then a NULL vector; extension_bit_reverse follows bit_reverse: NULL
    config, NULL vectors, then a size that is no power of two"""
    from icicle_amd._lib import lib, VecOpsConfig

    a = np.ones((4, 4), np.uint32)
    b = np.ones((4, 4), np.uint32)
    sentinel = 0xA5A5A5A5
    for name, n in NARGS.items():
        fn = getattr(lib, f"{f}_extension_{name}")
        out = np.full((4, 4), sentinel, np.uint32)
        cfg = VecOpsConfig.default()

        def call(size, cfg_ref, a_ptr=a.ctypes.data, b_ptr=b.ctypes.data, o_ptr=out.ctypes.data):
            args = (a_ptr, b_ptr) if n == 5 else (a_ptr,)
            return fn(*args, size, cfg_ref, o_ptr)

        assert call(4, None) == INVALID_POINTER, name
        assert call(0, None) == INVALID_POINTER, name  # the config is looked at first
        if name == "bit_reverse":
            assert call(4, ctypes.byref(cfg), a_ptr=None) == INVALID_POINTER
            assert call(4, ctypes.byref(cfg), o_ptr=None) == INVALID_POINTER
            assert call(0, ctypes.byref(cfg)) == INVALID_ARGUMENT and call(3, ctypes.byref(cfg)) == INVALID_ARGUMENT
        else:
            assert call(0, ctypes.byref(cfg)) == 0 and (out == sentinel).all(), name
            assert call(0, ctypes.byref(cfg), a_ptr=None, o_ptr=None) == 0, name  # size == 0 answers before the vectors are looked at
            assert call(4, ctypes.byref(cfg), a_ptr=None) == INVALID_POINTER, name
            assert call(4, ctypes.byref(cfg), o_ptr=None) == INVALID_POINTER, name
            if n == 5:
                assert call(4, ctypes.byref(cfg), b_ptr=None) == INVALID_POINTER, name
        assert (out == sentinel).all(), name


def test_extension_of_a_field_without_one_raises_before_the_library():
    from icicle_amd import vecops as V

    a = np.ones((4, 8), np.uint32)
    for fn in (V.vector_add, V.vector_sub, V.vector_mul, V.vector_div, V.scalar_add_vec, V.scalar_sub_vec, V.scalar_mul_vec):
        with pytest.raises(ValueError):
            fn("bn254", a, a, extension=True)
    for fn in (V.vector_inv, V.vector_sum, V.vector_product, V.bit_reverse):
        with pytest.raises(ValueError):
            fn("bn254", a, extension=True)
    with pytest.raises(ValueError):
        V.vector_mixed_mul("bn254", a, a)
    with pytest.raises(ValueError):
        V.extension_vector_inv_tile("stark252")


def test_no_gpu_means_loud_failure_not_fallback():
    import icicle_amd
    from icicle_amd import runtime, vecops as V

    if runtime.get_device_count() > 0:
        pytest.skip("GPU present")
    for f in M.FIELDS:
        a = M.to_words(f, [M.one(f)] * 4)
        base = M.base_to_words(f, [1] * 4)
        for fn in (V.vector_add, V.vector_sub, V.vector_mul, V.vector_div):
            with pytest.raises(icicle_amd.IcicleError):
                fn(f, a, a, extension=True)
        for fn in (V.scalar_add_vec, V.scalar_sub_vec, V.scalar_mul_vec):
            with pytest.raises(icicle_amd.IcicleError):
                fn(f, a[:1], a, extension=True)
        for fn in (V.vector_inv, V.vector_sum, V.vector_product, V.bit_reverse):
            with pytest.raises(icicle_amd.IcicleError):
                fn(f, a, extension=True)
        with pytest.raises(icicle_amd.IcicleError):
            V.vector_mixed_mul(f, a, base)


@pytest.mark.parametrize("f", ["babybear", "koalabear"])
def test_the_vectorised_reductions_equal_the_model(f):
    """M.reduce_np, which the GPU tests of 65539 entries compare with, against vsum / vproduct on small shapes, p - 1 and 0 among the values"""
    p = M.modulus(f)
    rng = np.random.default_rng(2251)
    for size, batch in ((1, 1), (3, 5), (65, 3), (2, 70)):
        a = rng.integers(0, p, size=(size * batch, 4), dtype=np.uint32)
        a[0], a[-1] = p - 1, (0, p - 1, 0, 1)
        ea = M.from_words(f, a)
        for columns in (False, True):
            for op in ("vector_sum", "vector_product"):
                assert M.from_words(f, M.reduce_np(f, op, a, size, batch, columns)) == M.run(f, op, ea, None, size, batch, columns), (f, op, size, batch, columns)
