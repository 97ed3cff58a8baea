"""CPU: Poseidon2 over BabyBear and KoalaBear without a GPU -- the test model (tests/poseidon2_model.py: derivation and hash in Python
integers) against the digests recorded from the reference (tests/golden/poseidon2_vectors.json); the library's own derivation
(icicle_amd/csrc/poseidon2_params.h) and the code a lane runs (poseidon2.hpp), compiled with g++ into a stand-alone program
(tests/poseidon2_host_harness.cpp), against the model and the recorded digests, once more under AddressSanitizer and UBSan; and
the argument checks of the C ABI that need no device."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests import poseidon2_model as pm

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INVALID_ARGUMENT = 11
# (t, R_F, R_P) of the published instances
ROUNDS = {
    "babybear": (7, [(2, 12, 24), (3, 12, 17), (4, 8, 21), (8, 8, 12), (12, 8, 10), (16, 8, 13), (20, 8, 18), (24, 8, 21)]),
    "koalabear": (3, [(2, 12, 34), (3, 12, 24), (4, 8, 27), (8, 8, 19), (12, 8, 20), (16, 8, 20), (20, 8, 20), (24, 8, 23)]),
}


@pytest.fixture(scope="module")
def vectors():
    with open(os.path.join(HERE, "golden", "poseidon2_vectors.json")) as f:
        return json.load(f)["cases"]


def ints(hexes):
    return [int(v, 16) for v in hexes]


# ---- the model -----------------------------------------------------------------------------------------------------------------
def test_model_round_numbers():
    for field, (alpha, rows) in ROUNDS.items():
        p = pm.FIELDS[field]
        assert pm.alpha_of(p) == alpha
        assert [(t,) + pm.round_numbers(p, t)[1:] for t in pm.WIDTHS] == rows, field


def test_model_matrices():
    assert pm.external_matrix(8)[0] == [10, 14, 2, 6, 5, 7, 1, 3] and pm.external_matrix(8)[5] == [4, 6, 1, 1, 8, 12, 2, 2]
    assert pm.external_matrix(3) == [[2, 1, 1], [1, 2, 1], [1, 1, 2]]
    assert pm.params("babybear", 2).m_i == [[2, 1], [1, 3]] and pm.params("koalabear", 3).m_i == [[2, 1, 1], [1, 2, 1], [1, 1, 3]]
    # the polynomial tools on cases with known answers: x^2 + 1 splits mod 5 and not mod 7; the characteristic polynomial of a companion matrix
    assert not pm.is_irreducible([1, 0, 1], 5) and pm.is_irreducible([1, 0, 1], 7)
    assert pm.charpoly([[0, 0, 3], [1, 0, 5], [0, 1, 6]], 11) == [8, 6, 5, 1]  # x^3 - 6 x^2 - 5 x - 3


def test_fixture_holds_the_cases_per_field_and_width(vectors):
    have = {(c["field"], c["t"], c["tag"], c["size"], c["batch"]) for c in vectors}
    for field, p in pm.FIELDS.items():
        for t in pm.WIDTHS:
            want = {(None, t, 1), (7, t - 1, 1), (None, t - 1, 1), (None, 2 * t - 1, 3)}
            want |= {(tag, s, 1) for tag in (None, 7) for s in (1, t + 1, 2 * t - 1, 2 * t, 3 * (t - 1) + 1)}
            assert {(field, t) + w for w in want} <= have, (field, t)
    for c in vectors:
        assert len(c["input"]) == c["size"] * c["batch"] and len(c["digests"]) == c["batch"]
        vals, p = ints(c["input"]), pm.FIELDS[c["field"]]
        assert max(vals) < p and p - 1 in vals and (len(vals) < 3 or {0, 1} <= set(vals))
    assert set(json.dumps(vectors)) <= set('0123456789abcdefghijklmnopqrstuvwxyz"[]{}:,_ ')  # inputs and digests, nothing else


def test_model_reproduces_every_recorded_digest(vectors):
    for c in vectors:
        got = pm.hash_batch(c["field"], c["t"], ints(c["input"]), c["size"], c["tag"])
        assert got == ints(c["digests"]), (c["field"], c["t"], c["tag"], c["size"], c["batch"])


# ---- the library's derivation and lane code, on the host ---------------------------------------------------------------------------
def build_harness(name, extra):
    exe = os.path.join(HERE, "_build", name)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    src = os.path.join(HERE, "poseidon2_host_harness.cpp")
    hdrs = [os.path.join(ROOT, "icicle_amd", "csrc", h) for h in ("poseidon2.hpp", "poseidon2_params.h", "smallfield.hpp", "hash_readers.hpp", "field_consts.h")]
    if not os.path.exists(exe) or max(os.path.getmtime(f) for f in [src] + hdrs) > os.path.getmtime(exe):
        subprocess.check_call(["g++", "-std=c++17", *extra, src, "-o", exe])
    return exe


def case_file(vectors, tmp_path):
    path = os.path.join(tmp_path, "cases.txt")
    with open(path, "w") as f:
        for c in vectors:
            tag = "-" if c["tag"] is None else f"{c['tag']:x}"
            f.write(" ".join([c["field"], str(c["t"]), tag, str(c["size"]), str(c["batch"])] + c["input"]) + "\n")
    return path


def check_params(text):
    lines = text.splitlines()
    assert len(lines) == 3 * 16
    at = 0
    for field in pm.FIELDS:
        for t in pm.WIDTHS:
            P = pm.params(field, t)
            assert lines[at] == f"params {field} {t} {P.alpha} {P.r_f} {P.r_p}"
            assert lines[at + 1].split() == ["rc"] + [f"{v:x}" for v in P.rc], (field, t)
            assert lines[at + 2].split() == ["diag"] + [f"{v:x}" for v in P.diag], (field, t)
            at += 3


def check_digests(text, vectors):
    lines = text.splitlines()
    assert len(lines) == 2 * len(vectors)
    for i, c in enumerate(vectors):
        assert lines[2 * i].split() == c["digests"], ("word reader", c["field"], c["t"], c["tag"], c["size"])
        assert lines[2 * i + 1].split() == c["digests"], ("padded reader", c["field"], c["t"], c["tag"], c["size"])


def test_host_build_derives_the_models_parameters_and_hashes_to_the_recorded_digests(vectors, tmp_path):
    exe = build_harness("poseidon2_host_harness", ["-O2"])
    check_params(subprocess.check_output([exe, "params"], text=True))
    check_digests(subprocess.check_output([exe, "hash", case_file(vectors, tmp_path)], text=True), vectors)


def test_host_build_is_clean_under_address_and_undefined_behaviour_sanitizers(vectors, tmp_path):
    """a stand-alone program: nothing of it is loaded into this interpreter"""
    # the sanitizers' runtimes are linked into the program itself
    exe = build_harness("poseidon2_host_harness_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    for args, check in ((["params"], check_params), (["hash", case_file(vectors, tmp_path)], lambda out: check_digests(out, vectors))):
        run = subprocess.run([exe] + args, env=env, text=True, capture_output=True)
        assert run.returncode == 0 and "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr[-2000:]
        check(run.stdout)


# ---- header, library, binding, and the argument checks that need no device ------------------------------------------------------------
def test_factories_are_declared_exported_and_bound():
    from icicle_amd import _lib
    from icicle_amd.hash import Hasher

    text = re.sub(r"\s+", " ", subprocess.check_output(["gcc", "-E", "-P", os.path.join(ROOT, "include", "icicle_hip.h")], text=True))
    for field in ("babybear", "koalabear"):
        name = f"{field}_create_poseidon2_hasher"
        assert re.search(r"icicle_hasher_handle_t %s\s*\(\s*unsigned t, const uint32_t\s*\* domain_tag, unsigned input_size\s*\)\s*;" % name, text)
        fn = getattr(_lib.lib, name)
        assert fn.restype is ctypes.c_void_p and len(fn.argtypes) == 3 and name in _lib.POSEIDON2_HANDLE_SYMBOLS
    assert callable(Hasher.poseidon2)


def test_widths_and_sizes_need_no_gpu():
    from icicle_amd._lib import lib
    from icicle_amd.hash import Hasher

    tag = ctypes.c_uint32(7)
    for field in ("babybear", "koalabear"):
        make = getattr(lib, f"{field}_create_poseidon2_hasher")
        for t in (0, 1, 5, 6, 7, 9, 28, 32):
            assert make(t, None, 0) is None and make(t, ctypes.byref(tag), 0) is None, t
            with pytest.raises(ValueError):
                Hasher.poseidon2(field, t)
        for t in pm.WIDTHS:
            for h, chunk in ((Hasher.poseidon2(field, t), 4 * t), (Hasher.poseidon2(field, t, domain_tag=7), 4 * (t - 1)), (Hasher.poseidon2(field, t, input_size=9), 36)):
                assert h.output_size == 4 and h.chunk == chunk
                h.close()
    with pytest.raises(ValueError):
        Hasher.poseidon2("goldilocks", 8)


def test_argument_errors_need_no_gpu():
    from icicle_amd import PowConfig
    from icicle_amd._lib import lib, HashConfig
    from icicle_amd.hash import Hasher

    h = Hasher.poseidon2("babybear", 16)
    cfg = HashConfig.default()
    inp, out = np.zeros(64, dtype=np.uint32), np.zeros(4, dtype=np.uint32)
    for nbytes in (1, 2, 3, 5, 63, 66):  # not whole elements: refused in front of any device call
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


def test_trees_of_poseidon2_layers_need_no_gpu_to_be_made():
    from icicle_amd.hash import Hasher
    from icicle_amd.merkle import MerkleTree

    for field in ("babybear", "koalabear"):
        leaf, node = Hasher.poseidon2(field, 16, input_size=8), Hasher.poseidon2(field, 2)
        tree = MerkleTree([leaf] + [node] * 6, 4)
        leaf.close(), node.close()  # the tree keeps what it needs
        del tree
