"""CPU: Poseidon2 over Goldilocks without a GPU -- the test model (tests/poseidon2_model_gold.py: derivation and hash in Python
integers) against the digests recorded from the reference (tests/golden/poseidon2_vectors_gold.json) and the reference's round
numbers; the library's own derivation (icicle_amd/csrc/poseidon2_gold_params.h) and the code a lane runs (poseidon2_gold.hpp),
compiled with g++ into a stand-alone program (tests/poseidon2_gold_host_harness.cpp), against the model's parameters and the
recorded digests, once more under AddressSanitizer and UBSan; and the argument checks of the C ABI that need no device."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests import poseidon2_model_gold as pg

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INVALID_ARGUMENT = 11
TAG = 7
P = pg.P


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "poseidon2_vectors_gold.json")) as f:
        return json.load(f)


def ints(hexes):
    return [int(v, 16) for v in hexes]


def tag_of(c):
    return None if c["tag"] is None else int(c["tag"], 16)


# ---- the model -----------------------------------------------------------------------------------------------------------------
def test_model_derives_the_round_numbers_of_the_reference():
    for t in pg.WIDTHS:
        Q = pg.params(t)
        assert Q.alpha == pg.EXPECTED_ALPHA == 7 and (Q.r_f, Q.r_p) == pg.EXPECTED_ROUNDS[t], t
        assert len(Q.rc) == Q.r_f * t + Q.r_p and max(Q.rc) < P and len(Q.diag) == t
        if t <= 3:
            assert Q.diag == [2, 2, 3][3 - t:] and Q.draws == 0
        else:
            assert max(Q.diag) < P and Q.draws >= 1
    assert {t: pg.EXPECTED_ROUNDS[t] for t in (2, 3, 4)} == {2: (8, 27), 3: (8, 23), 4: (8, 21)}
    assert all(pg.EXPECTED_ROUNDS[t] == (8, 22) for t in (8, 12, 16, 20, 24))


def test_fixture_holds_the_cases_of_every_width_and_nothing_but_hex(golden):
    cases = golden["cases"]
    edges = {(1 << 32) - 1, 1 << 32, (1 << 64) - (1 << 32)}
    for t in pg.WIDTHS:
        mine = [c for c in cases if c["t"] == t]
        have = {(tag_of(c), c["size"], c["batch"]) for c in mine}
        want = {(None, t, 1), (TAG, t - 1, 1), (None, t - 1, 1), (None, 2 * t - 1, 3)}
        for size in (1, t + 1, 2 * t - 1, 2 * t, 3 * (t - 1) + 1):
            want |= {(None, size, 1), (TAG, size, 1)}
        assert want <= have, t
        assert any(tag is not None and tag >= 1 << 32 for tag, _, _ in have - want), t  # the tag's upper word is read
        assert any(edges <= set(ints(c["input"])) for c in mine), t  # where the fix-ups of the 128-bit reduction change branch
    for c in cases:
        vals = ints(c["input"])
        assert len(vals) == c["size"] * c["batch"] and len(c["digests"]) == c["batch"] and max(vals) < P and max(ints(c["digests"])) < P
        assert c["tag"] is None or isinstance(c["tag"], str)
        if len(vals) >= 3 and not edges <= set(vals):
            assert {0, 1, P - 1} <= set(vals)
    assert set(json.dumps(cases)) <= set('0123456789abcdefghijklmnopqrstuvwxyz"[]{}:,_ ')
    assert os.path.getsize(os.path.join(HERE, "golden", "poseidon2_vectors_gold.json")) < 82_000  # well under the wide fixture
    # no constant and no matrix entry: nothing recorded is a round constant or an entry of a drawn diagonal
    recorded = {v for c in cases for v in c["input"] + c["digests"]}
    for t in pg.WIDTHS:
        Q = pg.params(t)
        assert not recorded & {f"{v:x}" for v in Q.rc + (Q.diag if t > 3 else [])}


def test_model_reproduces_every_recorded_digest(golden):
    for c in golden["cases"]:
        got = pg.hash_batch(c["t"], ints(c["input"]), c["size"], tag_of(c))
        assert got == ints(c["digests"]), (c["t"], c["tag"], c["size"])


def test_model_counts_a_word_above_p_as_its_residue():
    msg = [P, P + 5, (1 << 64) - 1, 3]
    assert pg.hash_one(3, msg) == pg.hash_one(3, [0, 5, (1 << 64) - 1 - P, 3])


# ---- the library's derivation and lane code, on the host ---------------------------------------------------------------------------
def build_harness(name, extra):
    exe = os.path.join(HERE, "_build", name)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    src = os.path.join(HERE, "poseidon2_gold_host_harness.cpp")
    hdrs = [os.path.join(ROOT, "icicle_amd", "csrc", h) for h in ("poseidon2_gold.hpp", "poseidon2_gold_params.h", "poseidon2_params.h", "goldfield.hpp", "bigfield.hpp",
                                                                  "mont_asm.hpp", "hash_readers.hpp", "field_consts.h")]
    if not os.path.exists(exe) or max(os.path.getmtime(f) for f in [src] + hdrs) > os.path.getmtime(exe):
        subprocess.check_call(["g++", "-std=c++17", "-Wno-unknown-pragmas", *extra, src, "-o", exe])
    return exe


def case_file(cases, tmp_path):
    path = os.path.join(tmp_path, "cases.txt")
    with open(path, "w") as f:
        for c in cases:
            f.write(" ".join([str(c["t"]), c["tag"] or "-", str(c["size"]), str(c["batch"])] + c["input"]) + "\n")
    return path


def check_params(text):
    lines = text.splitlines()
    assert len(lines) == 3 * len(pg.WIDTHS)
    for at, t in enumerate(pg.WIDTHS):
        Q = pg.params(t)
        assert lines[3 * at] == f"params {t} {Q.alpha} {Q.r_f} {Q.r_p} {Q.draws}"
        assert lines[3 * at + 1].split() == ["rc"] + [f"{v:x}" for v in Q.rc], t
        assert lines[3 * at + 2].split() == ["diag"] + [f"{v:x}" for v in Q.diag], t


def check_digests(text, cases):
    lines = text.splitlines()
    assert len(lines) == 2 * len(cases)
    for i, c in enumerate(cases):
        assert lines[2 * i].split() == c["digests"], ("word reader", c["t"], c["tag"], c["size"])
        assert lines[2 * i + 1].split() == c["digests"], ("padded reader", c["t"], c["tag"], c["size"])


def with_words_above_p(cases):
    """the recorded cases and, behind them, those of t = 3 and 8 with p added to every input below 2^64 - p: the same digests"""
    more = []
    for c in cases:
        if c["t"] in (3, 8) and any(v < (1 << 64) - P for v in ints(c["input"])):
            more.append(dict(c, input=[f"{v + P if v < (1 << 64) - P else v:x}" for v in ints(c["input"])]))
    assert more
    return cases + more


def test_host_build_derives_the_models_parameters_and_hashes_to_the_recorded_digests(golden, tmp_path):
    exe = build_harness("poseidon2_gold_host_harness", ["-O2"])
    check_params(subprocess.check_output([exe, "params"], text=True))
    cases = with_words_above_p(golden["cases"])
    check_digests(subprocess.check_output([exe, "hash", case_file(cases, tmp_path)], text=True), cases)


def test_host_build_is_clean_under_address_and_undefined_behaviour_sanitizers(golden, tmp_path):
    """a stand-alone program: nothing of it is loaded into this interpreter"""
    # the sanitizers' runtimes are linked into the program itself
    exe = build_harness("poseidon2_gold_host_harness_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    cases = with_words_above_p(golden["cases"])
    for args, check in ((["params"], check_params), (["hash", case_file(cases, tmp_path)], lambda out: check_digests(out, cases))):
        run = subprocess.run([exe] + args, env=env, text=True, capture_output=True)
        assert run.returncode == 0 and "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr[-2000:]
        check(run.stdout)


# ---- header, library, binding, and the argument checks that need no device ------------------------------------------------------------
def test_factory_is_declared_exported_and_bound():
    from icicle_amd import _lib
    from icicle_amd.hash import Hasher

    text = re.sub(r"\s+", " ", subprocess.check_output(["gcc", "-E", "-P", os.path.join(ROOT, "include", "icicle_hip.h")], text=True))
    assert _lib.POSEIDON2_GOLD_FIELDS == ["goldilocks"] and _lib.POSEIDON2_FIELDS == ["babybear", "koalabear"] and "goldilocks" not in _lib.POSEIDON2_WIDE_FIELDS
    name = "goldilocks_create_poseidon2_hasher"
    assert re.search(r"icicle_hasher_handle_t %s\s*\(\s*unsigned t, const uint32_t\s*\* domain_tag, unsigned input_size\s*\)\s*;" % name, text)
    fn = getattr(_lib.lib, name)
    assert fn.restype is ctypes.c_void_p and len(fn.argtypes) == 3 and list(_lib.POSEIDON2_GOLD_HANDLE_SYMBOLS) == [name]
    assert callable(Hasher.poseidon2_goldilocks)


def words_of(value):
    return (ctypes.c_uint32 * 2)(value & 0xFFFFFFFF, value >> 32)


def test_widths_tags_and_sizes_need_no_gpu():
    from icicle_amd._lib import lib
    from icicle_amd.hash import Hasher

    make = lib.goldilocks_create_poseidon2_hasher
    for t in (0, 1, 5, 6, 7, 9, 28, 32):
        assert make(t, None, 0) is None and make(t, words_of(TAG), 0) is None, t
        with pytest.raises(ValueError):
            Hasher.poseidon2_goldilocks(t)
    for t in pg.WIDTHS:
        for tag in (P, P + 1, (1 << 64) - 1):
            assert make(t, words_of(tag), 0) is None
            with pytest.raises(ValueError):
                Hasher.poseidon2_goldilocks(t, domain_tag=tag)
        for h, elems in ((Hasher.poseidon2_goldilocks(t), t), (Hasher.poseidon2_goldilocks(t, domain_tag=TAG), t - 1), (Hasher.poseidon2_goldilocks(t, input_size=9), 9),
                         (Hasher.poseidon2_goldilocks(t, domain_tag=P - 1, input_size=5), 5), (Hasher.poseidon2_goldilocks(t, domain_tag=1 << 40), t - 1)):
            assert h.output_size == 8 and h.chunk == 8 * elems
            h.close()
    with pytest.raises(ValueError):
        Hasher.poseidon2_goldilocks(8, domain_tag=1 << 64)
    with pytest.raises(ValueError):
        Hasher.poseidon2_goldilocks(8, domain_tag=-1)
    with pytest.raises(ValueError, match="poseidon2_goldilocks"):
        Hasher.poseidon2("goldilocks", 8)  # the call by field name keeps refusing it and says where to go
    babybear = Hasher.poseidon2("babybear", 8, domain_tag=TAG)  # the 31-bit hashers keep their element size
    assert babybear.output_size == 4 and babybear.chunk == 28
    babybear.close()


def test_argument_errors_need_no_gpu():
    from icicle_amd import PowConfig
    from icicle_amd._lib import lib, HashConfig
    from icicle_amd.hash import Hasher

    cfg = HashConfig.default()
    for h in (Hasher.poseidon2_goldilocks(3), Hasher.poseidon2_goldilocks(8, domain_tag=TAG), Hasher.poseidon2_goldilocks(12, input_size=8)):
        inp, out = np.zeros(32, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
        for nbytes in (1, 4, 7, 9, 12, 20, 60, 64 - 4, 64 + 4):  # not whole elements: refused in front of any device call
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


def test_trees_of_goldilocks_poseidon2_layers_need_no_gpu_to_be_made():
    from icicle_amd._lib import lib
    from icicle_amd.hash import Hasher
    from icicle_amd.merkle import MerkleTree

    for leaf, node in ((Hasher.poseidon2_goldilocks(2, input_size=1), Hasher.poseidon2_goldilocks(2)),
                       (Hasher.poseidon2_goldilocks(12, input_size=8), Hasher.poseidon2_goldilocks(8, input_size=2)),
                       (Hasher.poseidon2_goldilocks(8, input_size=1), Hasher.poseidon2_goldilocks(3, domain_tag=TAG))):
        tree = MerkleTree([leaf] + [node] * 4, 8)
        leaf.close(), node.close()  # the tree keeps what it needs
        size = ctypes.c_size_t(0)
        assert lib.icicle_merkle_tree_get_root(tree.handle, ctypes.byref(size)) is None  # not built yet
        del tree
    # a byte hasher above a Poseidon2 layer, where the sizes fit, and a layer whose input is no whole number of digests
    leaf = Hasher.poseidon2_goldilocks(12, input_size=8)
    tree = MerkleTree([leaf, Hasher.keccak256(16)], 8)
    del tree
    with pytest.raises(Exception):
        MerkleTree([leaf, Hasher.poseidon2_goldilocks(2), Hasher.keccak256(12)], 8)
