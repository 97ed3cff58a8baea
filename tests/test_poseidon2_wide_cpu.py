"""CPU: Poseidon2 over the scalar fields of BN254, BLS12-381, BLS12-377 and Grumpkin and over stark252 without a GPU -- the test
model (tests/poseidon2_model_wide.py: derivation and hash in Python integers) against the digests recorded from the reference
(tests/golden/poseidon2_vectors_wide.json) and the reference's round numbers; the library's own derivation
(icicle_amd/csrc/poseidon2_wide_params.h) and the code a lane runs (poseidon2_wide.hpp), compiled with g++ into a stand-alone
program (tests/poseidon2_wide_host_harness.cpp), against the model's parameters and the recorded digests, once more with the bound
tracker of bigfield.hpp and once more under AddressSanitizer and UBSan; and the argument checks of the C ABI that need no
device."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests import poseidon2_model_wide as pw

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INVALID_ARGUMENT = 11
TAG = 7
PAIRS = [(f, t) for f in pw.FIELDS for t in pw.WIDTHS]


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "poseidon2_vectors_wide.json")) as f:
        return json.load(f)


def ints(hexes):
    return [int(v, 16) for v in hexes]


# ---- the model -----------------------------------------------------------------------------------------------------------------
def test_fixture_holds_the_cases_of_every_pair_and_no_constant(golden):
    cases = golden["cases"]
    for field, t in PAIRS:
        have = {(c["tag"], c["size"], c["batch"]) for c in cases if (c["field"], c["t"]) == (field, t)}
        want = {(None, t, 1), (TAG, t - 1, 1), (None, 1, 1), (TAG, 1, 1), (None, t + 1, 1), (TAG, t + 1, 1), (None, 2 * t - 1, 3), (None, 3 * (t - 1) + 1, 1)}
        assert have == want, (field, t)
    for c in cases:
        vals, p = ints(c["input"]), pw.FIELDS[c["field"]]
        assert len(vals) == c["size"] * c["batch"] and len(c["digests"]) == c["batch"] and max(vals) < p
        if len(vals) >= 3:
            assert {0, 1, p - 1} <= set(vals)
    assert set(json.dumps(cases)) <= set('0123456789abcdefghijklmnopqrstuvwxyz"[]{}:,_ ')
    assert os.path.getsize(os.path.join(HERE, "golden", "poseidon2_vectors_wide.json")) < 200_000
    # no constant and no matrix entry: nothing recorded is a round constant or an entry of a drawn diagonal
    recorded = {v for c in cases for v in c["input"] + c["digests"]}
    for field, t in PAIRS:
        P = pw.params(field, t)
        assert not recorded & {f"{v:x}" for v in P.rc + (P.diag if t > 3 else [])}


def test_model_derives_the_round_numbers_of_the_reference():
    for field, (alpha, r_f, r_ps) in pw.EXPECTED_ROUNDS.items():
        for t, r_p in zip(pw.WIDTHS, r_ps):
            P = pw.params(field, t)
            assert (P.alpha, P.r_f, P.r_p) == (alpha, r_f, r_p), (field, t)
            assert len(P.rc) == r_f * t + r_p and max(P.rc) < P.p and len(P.diag) == t
            if t <= 3:
                assert P.diag == [2, 2, 3][3 - t:] and P.draws == 0
            else:
                assert max(P.diag) < P.p and 1 <= P.draws <= 31


def test_model_reproduces_every_recorded_digest(golden):
    for c in golden["cases"]:
        got = pw.hash_batch(c["field"], c["t"], ints(c["input"]), c["size"], c["tag"])
        assert got == ints(c["digests"]), (c["field"], c["t"], c["tag"], c["size"])


# ---- the library's derivation and lane code, on the host ---------------------------------------------------------------------------
def build_harness(name, extra):
    exe = os.path.join(HERE, "_build", name)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    src = os.path.join(HERE, "poseidon2_wide_host_harness.cpp")
    hdrs = [os.path.join(ROOT, "icicle_amd", "csrc", h) for h in ("poseidon2_wide.hpp", "poseidon2_wide_params.h", "poseidon2_params.h", "poseidon.hpp", "poseidon_params.h",
                                                                  "bigfield.hpp", "mont_asm.hpp", "hash_readers.hpp", "field_consts.h")]
    if not os.path.exists(exe) or max(os.path.getmtime(f) for f in [src] + hdrs) > os.path.getmtime(exe):
        subprocess.check_call(["g++", "-std=c++17", "-Wno-unknown-pragmas", *extra, src, "-o", exe])
    return exe


def case_file(cases, tmp_path):
    path = os.path.join(tmp_path, "cases.txt")
    with open(path, "w") as f:
        for c in cases:
            tag = "-" if c["tag"] is None else f"{c['tag']:x}"
            f.write(" ".join([c["field"], str(c["t"]), tag, str(c["size"]), str(c["batch"])] + c["input"]) + "\n")
    return path


def check_params(text):
    lines = text.splitlines()
    assert len(lines) == 3 * len(PAIRS)
    for at, (field, t) in enumerate(PAIRS):
        P = pw.params(field, t)
        assert lines[3 * at] == f"params {field} {t} {P.alpha} {P.r_f} {P.r_p} {P.draws}"
        assert lines[3 * at + 1].split() == ["rc"] + [f"{v:x}" for v in P.rc], (field, t)
        assert lines[3 * at + 2].split() == ["diag"] + [f"{v:x}" for v in P.diag], (field, t)


def check_digests(text, cases):
    lines = text.splitlines()
    assert len(lines) == 2 * len(cases)
    for i, c in enumerate(cases):
        assert lines[2 * i].split() == c["digests"], ("word reader", c["field"], c["t"], c["tag"], c["size"])
        assert lines[2 * i + 1].split() == c["digests"], ("padded reader", c["field"], c["t"], c["tag"], c["size"])


def test_host_build_derives_the_models_parameters_and_hashes_to_the_recorded_digests(golden, tmp_path):
    exe = build_harness("poseidon2_wide_host_harness", ["-O2"])
    check_params(subprocess.check_output([exe, "params"], text=True))
    check_digests(subprocess.check_output([exe, "hash", case_file(golden["cases"], tmp_path)], text=True), golden["cases"])


def test_host_build_stays_within_the_operand_bounds_of_the_lazy_field_operations(golden, tmp_path):
    """-DBIGFIELD_BOUNDS: every element carries its bound in units of p and every operation asserts its precondition (the bounds do not
    depend on the values, so one pass over every field, width and message shape proves where the conditional subtractions stand)"""
    exe = build_harness("poseidon2_wide_host_harness_bounds", ["-O1", "-DBIGFIELD_BOUNDS"])
    run = subprocess.run([exe, "hash", case_file(golden["cases"], tmp_path)], text=True, capture_output=True)
    assert run.returncode == 0 and "bound violation" not in run.stderr, run.stderr[-2000:]
    check_digests(run.stdout, golden["cases"])


def test_host_build_is_clean_under_address_and_undefined_behaviour_sanitizers(golden, tmp_path):
    """a stand-alone program: nothing of it is loaded into this interpreter"""
    # the sanitizers' runtimes are linked into the program itself
    exe = build_harness("poseidon2_wide_host_harness_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    cases = golden["cases"]
    for args, check in ((["params"], check_params), (["hash", case_file(cases, tmp_path)], lambda out: check_digests(out, cases))):
        run = subprocess.run([exe] + args, env=env, text=True, capture_output=True)
        assert run.returncode == 0 and "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr[-2000:]
        check(run.stdout)


# ---- header, library, binding, and the argument checks that need no device ------------------------------------------------------------
def test_factories_are_declared_exported_and_bound():
    from icicle_amd import _lib
    from icicle_amd.hash import Hasher

    text = re.sub(r"\s+", " ", subprocess.check_output(["gcc", "-E", "-P", os.path.join(ROOT, "include", "icicle_hip.h")], text=True))
    assert _lib.POSEIDON2_WIDE_FIELDS == list(pw.FIELDS) and _lib.POSEIDON2_FIELDS == ["babybear", "koalabear"]
    for field in _lib.POSEIDON2_WIDE_FIELDS:
        name = f"{field}_create_poseidon2_hasher"
        assert re.search(r"icicle_hasher_handle_t %s\s*\(\s*unsigned t, const uint32_t\s*\* domain_tag, unsigned input_size\s*\)\s*;" % name, text)
        fn = getattr(_lib.lib, name)
        assert fn.restype is ctypes.c_void_p and len(fn.argtypes) == 3 and name in _lib.POSEIDON2_WIDE_HANDLE_SYMBOLS
    assert callable(Hasher.poseidon2)


def words_of(value):
    return (ctypes.c_uint32 * 8)(*[value >> (32 * i) & 0xFFFFFFFF for i in range(8)])


def test_widths_tags_and_sizes_need_no_gpu():
    from icicle_amd._lib import lib
    from icicle_amd.hash import Hasher

    for field, p in pw.FIELDS.items():
        make = getattr(lib, f"{field}_create_poseidon2_hasher")
        for t in (0, 1, 5, 12, 16):
            assert make(t, None, 0) is None and make(t, words_of(TAG), 0) is None, t
            with pytest.raises(ValueError):
                Hasher.poseidon2(field, t)
        for t in pw.WIDTHS:
            for tag in (p, (1 << 256) - 1):
                assert make(t, words_of(tag), 0) is None
                with pytest.raises(ValueError):
                    Hasher.poseidon2(field, t, domain_tag=tag)
            for h, elems in ((Hasher.poseidon2(field, t), t), (Hasher.poseidon2(field, t, domain_tag=TAG), t - 1), (Hasher.poseidon2(field, t, input_size=9), 9),
                             (Hasher.poseidon2(field, t, domain_tag=np.array([TAG] + [0] * 7, dtype=np.uint32), input_size=5), 5),
                             (Hasher.poseidon2(field, t, domain_tag=p - 1), t - 1)):
                assert h.output_size == 32 and h.chunk == 32 * elems
                h.close()
    with pytest.raises(ValueError):
        Hasher.poseidon2("goldilocks", 8)
    with pytest.raises(ValueError):
        Hasher.poseidon2("bn254", 3, domain_tag=1 << 256)
    babybear = Hasher.poseidon2("babybear", 8, domain_tag=TAG)  # the 31-bit hashers keep their element size
    assert babybear.output_size == 4 and babybear.chunk == 28
    babybear.close()


def test_argument_errors_need_no_gpu():
    from icicle_amd import PowConfig
    from icicle_amd._lib import lib, HashConfig
    from icicle_amd.hash import Hasher

    cfg = HashConfig.default()
    for h in (Hasher.poseidon2("bn254", 3), Hasher.poseidon2("stark252", 8, domain_tag=TAG), Hasher.poseidon2("bls12_381", 4, input_size=4)):
        inp, out = np.zeros(8 * 12, dtype=np.uint32), np.zeros(8, dtype=np.uint32)
        for nbytes in (1, 4, 31, 33, 36, 60, 96 - 4, 96 + 16):  # not whole elements: refused in front of any device call
            assert lib.icicle_hasher_hash(h.handle, inp.ctypes.data, nbytes, ctypes.byref(cfg), out.ctypes.data) == INVALID_ARGUMENT, nbytes
        assert not out.any()
        # a digest of one element is no proof-of-work candidate
        pcfg = PowConfig.default()
        found, nonce, mined, ok = ctypes.c_bool(False), ctypes.c_uint64(77), ctypes.c_uint64(78), ctypes.c_bool(False)
        challenge = (ctypes.c_uint8 * 32)()
        assert lib.proof_of_work(h.handle, challenge, 32, 4, ctypes.byref(pcfg), ctypes.byref(found), ctypes.byref(nonce), ctypes.byref(mined)) == INVALID_ARGUMENT
        assert lib.proof_of_work_verify(h.handle, challenge, 32, 4, ctypes.byref(pcfg), 5, ctypes.byref(ok), ctypes.byref(mined)) == INVALID_ARGUMENT
        assert (found.value, nonce.value, mined.value, ok.value) == (False, 77, 78, False)
        h.close()


def test_trees_of_wide_poseidon2_layers_need_no_gpu_to_be_made():
    from icicle_amd._lib import lib
    from icicle_amd.hash import Hasher
    from icicle_amd.merkle import MerkleTree

    for field in pw.FIELDS:
        for leaf, node in ((Hasher.poseidon2(field, 4, input_size=4), Hasher.poseidon2(field, 2)),
                           (Hasher.poseidon2(field, 8, input_size=8), Hasher.poseidon2(field, 3, domain_tag=TAG))):
            tree = MerkleTree([leaf] + [node] * 4, 32)
            leaf.close(), node.close()  # the tree keeps what it needs
            size = ctypes.c_size_t(0)
            assert lib.icicle_merkle_tree_get_root(tree.handle, ctypes.byref(size)) is None  # not built yet
            del tree
    # a byte hasher above a Poseidon2 layer, where the sizes fit, and a layer whose input is no whole number of digests
    leaf = Hasher.poseidon2("bn254", 4, input_size=4)
    tree = MerkleTree([leaf, Hasher.keccak256(64)], 32)
    del tree
    with pytest.raises(Exception):
        MerkleTree([leaf, Hasher.poseidon2("bn254", 2), Hasher.keccak256(48)], 32)
