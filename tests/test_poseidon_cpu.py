"""CPU: Poseidon over the scalar fields of BN254, BLS12-381, BLS12-377 and Grumpkin without a GPU -- the test model
(tests/poseidon_model.py: the textbook permutation in Python integers) against the digests, roots and paths recorded from the
reference (tests/golden/poseidon_vectors.json); the library's own derivation of the optimized schedule
(icicle_amd/csrc/poseidon_params.h) and the code a lane runs (poseidon.hpp), compiled with g++ into a stand-alone program
(tests/poseidon_host_harness.cpp), against a derivation of the same tables written here and against the recorded digests, once more
with the bound tracker of bigfield.hpp and once more under AddressSanitizer and UBSan; and the argument checks of the C ABI that
need no device."""
import ctypes
import functools
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests import poseidon_model as pm

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INVALID_ARGUMENT = 11
TAG = 7


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "poseidon_vectors.json")) as f:
        return json.load(f)


def ints(hexes):
    return [int(v, 16) for v in hexes]


# ---- the model -----------------------------------------------------------------------------------------------------------------
def test_fixture_holds_every_built_pair_with_and_without_a_tag(golden):
    cases = golden["cases"]
    assert {(c["field"], c["t"], c["tag"]) for c in cases} == {(f, t, tag) for f, t in pm.BUILT for tag in (None, TAG)}
    for c in cases:
        vals, p = ints(c["input"]), pm.FIELDS[c["field"]]
        assert c["batch"] == 3 and len(vals) == 3 * pm.arity(c["t"], c["tag"]) and len(c["digests"]) == 3
        assert max(vals) < p and {0, 1, p - 1} <= set(vals)
    shapes = {(t["field"], t["t"], t["tag"], t["layers"], len(t["leaves"])) for t in golden["trees"]}
    assert {("bn254", 3, TAG, 3, 8), ("bn254", 3, TAG, 3, 5), ("bn254", 5, TAG, 2, 16), ("bn254", 3, None, 2, 9)} <= shapes
    assert set(json.dumps(golden["cases"]) + json.dumps(golden["trees"])) <= set('0123456789abcdefghijklmnopqrstuvwxyz"[]{}:,_ ')
    assert os.path.getsize(os.path.join(HERE, "golden", "poseidon_vectors.json")) <= os.path.getsize(os.path.join(HERE, "golden", "poseidon2_vectors.json"))


def test_model_reproduces_every_recorded_digest(golden):
    for c in golden["cases"]:
        assert pm.hash_batch(c["field"], c["t"], ints(c["input"]), c["tag"]) == ints(c["digests"]), (c["field"], c["t"], c["tag"])


def test_model_reproduces_every_recorded_root_and_path(golden):
    for t in golden["trees"]:
        shape = pm.TreeShape([(t["field"], t["t"], t["tag"])] * t["layers"])
        leaves = pm.to_bytes(ints(t["leaves"]))
        leaf, path, root = pm.proof(shape, leaves, t["leaf_idx"], False, t["policy"])
        assert root == pm.to_bytes([int(t["root"], 16)]) and path == pm.to_bytes(ints(t["path"])), (t["field"], t["t"], len(t["leaves"]))
        assert pm.verify(shape, leaf, t["leaf_idx"], path, root, False)


# ---- the optimized schedule, derived here from the model's constants and matrix ------------------------------------------------------
def mat_mul(a, b, p):
    n = len(a)
    return [[sum(a[i][k] * b[k][j] for k in range(n)) % p for j in range(n)] for i in range(n)]


def mat_inv(a, p):
    n = len(a)
    m = [row[:] + [int(i == j) for j in range(n)] for i, row in enumerate(a)]
    for c in range(n):
        r = next(r for r in range(c, n) if m[r][c] % p)
        m[c], m[r] = m[r], m[c]
        iv = pow(m[c][c], -1, p)
        m[c] = [x * iv % p for x in m[c]]
        for r in range(n):
            if r != c and m[r][c]:
                f = m[r][c]
                m[r] = [(x - f * y) % p for x, y in zip(m[r], m[c])]
    return [row[n:] for row in m]


def row_times(v, a, p):
    return [sum(v[i] * a[i][j] for i in range(len(a))) % p for j in range(len(a))]


@functools.lru_cache(maxsize=None)
def optimized_tables(field, t):
    """(rc, mds, pre, sparse) as flat lists: the constants moved behind the matrices, the matrix in front of the partial rounds and
    the sparse factors of M = M' M'' (first column, then first row), in the order the schedule uses them"""
    p, grain, m = pm.params(field, t)
    half, r_p = pm.R_F // 2, pm.R_P[t]
    key = lambda r: grain[r * t:(r + 1) * t]  # noqa: E731
    mi = mat_inv(m, p)
    rc = list(key(0))
    for r in range(1, half):
        rc += row_times(key(r), mi, p)
    acc, partial = key(half + r_p), []
    for i in range(r_p):
        moved = row_times(acc, mi, p)
        partial.append(moved[0])
        moved[0] = 0
        acc = [(a + b) % p for a, b in zip(key(half + r_p - 1 - i), moved)]
    rc += row_times(acc, mi, p) + partial[::-1]
    for r in range(1, half):
        rc += row_times(key(half + r_p + r), mi, p)
    cur, sparse = m, []
    for _ in range(r_p):
        hat = [row[1:] for row in cur[1:]]
        w_hat = [sum(x * cur[k + 1][0] for k, x in enumerate(row)) % p for row in mat_inv(hat, p)]
        sparse.append([cur[0][0]] + w_hat + cur[0][1:])
        prime = [[1] + [0] * (t - 1)] + [[0] + row for row in hat]
        cur = mat_mul(m, prime, p)
    flat = lambda rows: [x for row in rows for x in row]  # noqa: E731
    return rc, flat(m), flat(cur), flat(sparse[::-1])


def optimized_permute(field, t, state):
    """the schedule the kernel runs, on the tables above"""
    p = pm.FIELDS[field]
    rc, mds, pre, sparse = optimized_tables(field, t)
    half, r_p = pm.R_F // 2, pm.R_P[t]
    times = lambda s, a: [sum(s[i] * a[i * t + j] for i in range(t)) % p for j in range(t)]  # noqa: E731
    s = [(x + c) % p for x, c in zip(state, rc[:t])]
    at = t
    for r in range(half):
        s = times([(pow(x, 5, p) + c) % p for x, c in zip(s, rc[at:at + t])], pre if r == half - 1 else mds)
        at += t
    for r in range(r_p):
        sp = sparse[r * (2 * t - 1):(r + 1) * (2 * t - 1)]
        s[0] = (pow(s[0], 5, p) + rc[at]) % p
        s = [sum(x * c for x, c in zip(s, sp[:t])) % p] + [(s[0] * sp[t + j - 1] + s[j]) % p for j in range(1, t)]
        at += 1
    for r in range(half - 1):
        s = times([(pow(x, 5, p) + c) % p for x, c in zip(s, rc[at:at + t])], mds)
        at += t
    assert at == len(rc) == t * pm.R_F + r_p
    return times([pow(x, 5, p) for x in s], mds)


def test_textbook_and_optimized_schedules_agree():
    for field, t in pm.BUILT:
        p = pm.FIELDS[field]
        state = [(p - 1 - 3 * i * i) % p for i in range(t)]
        assert optimized_permute(field, t, state) == pm.permute(field, t, state), (field, t)


# ---- the library's derivation and lane code, on the host ---------------------------------------------------------------------------
def build_harness(name, extra):
    exe = os.path.join(HERE, "_build", name)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    src = os.path.join(HERE, "poseidon_host_harness.cpp")
    hdrs = [os.path.join(ROOT, "icicle_amd", "csrc", h) for h in ("poseidon.hpp", "poseidon_params.h", "bigfield.hpp", "mont_asm.hpp", "hash_readers.hpp", "field_consts.h")]
    if not os.path.exists(exe) or max(os.path.getmtime(f) for f in [src] + hdrs) > os.path.getmtime(exe):
        subprocess.check_call(["g++", "-std=c++17", "-Wno-unknown-pragmas", *extra, src, "-o", exe])
    return exe


def case_file(cases, tmp_path):
    path = os.path.join(tmp_path, "cases.txt")
    with open(path, "w") as f:
        for c in cases:
            tag = "-" if c["tag"] is None else f"{c['tag']:x}"
            f.write(" ".join([c["field"], str(c["t"]), tag, str(c["batch"])] + c["input"]) + "\n")
    return path


def check_params(text):
    lines = text.splitlines()
    assert len(lines) == 5 * len(pm.BUILT)
    for at, (field, t) in enumerate(pm.BUILT):
        assert lines[5 * at] == f"params {field} {t} {pm.R_F} {pm.R_P[t]}"
        for line, name, want in zip(lines[5 * at + 1:5 * at + 5], ("rc", "mds", "pre", "sparse"), optimized_tables(field, t)):
            assert line.split() == [name] + [f"{v:x}" for v in want], (field, t, name)


def check_digests(text, cases):
    lines = text.splitlines()
    assert len(lines) == 2 * len(cases)
    for i, c in enumerate(cases):
        assert lines[2 * i].split() == c["digests"], ("word reader", c["field"], c["t"], c["tag"])
        assert lines[2 * i + 1].split() == c["digests"], ("padded reader", c["field"], c["t"], c["tag"])


def test_host_build_derives_these_tables_and_hashes_to_the_recorded_digests(golden, tmp_path):
    exe = build_harness("poseidon_host_harness", ["-O2"])
    check_params(subprocess.check_output([exe, "params"], text=True))
    check_digests(subprocess.check_output([exe, "hash", case_file(golden["cases"], tmp_path)], text=True), golden["cases"])


def test_host_build_stays_within_the_operand_bounds_of_the_lazy_field_operations(golden, tmp_path):
    """-DBIGFIELD_BOUNDS: every element carries its bound in units of p and every operation asserts its precondition (the bounds do not
    depend on the values, so one pass over every width proves them)"""
    exe = build_harness("poseidon_host_harness_bounds", ["-O1", "-DBIGFIELD_BOUNDS"])
    run = subprocess.run([exe, "hash", case_file(golden["cases"], tmp_path)], text=True, capture_output=True)
    assert run.returncode == 0 and "bound violation" not in run.stderr, run.stderr[-2000:]
    check_digests(run.stdout, golden["cases"])


def test_host_build_is_clean_under_address_and_undefined_behaviour_sanitizers(golden, tmp_path):
    """a stand-alone program: nothing of it is loaded into this interpreter"""
    # the sanitizers' runtimes are linked into the program itself
    exe = build_harness("poseidon_host_harness_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"])
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
    assert _lib.POSEIDON_FIELDS == ["bn254", "bls12_381", "bls12_377", "grumpkin"]
    for field in _lib.POSEIDON_FIELDS:
        name = f"{field}_create_poseidon_hasher"
        assert re.search(r"icicle_hasher_handle_t %s\s*\(\s*unsigned t, const uint32_t\s*\* domain_tag, unsigned input_size\s*\)\s*;" % name, text)
        fn = getattr(_lib.lib, name)
        assert fn.restype is ctypes.c_void_p and len(fn.argtypes) == 3 and name in _lib.POSEIDON_HANDLE_SYMBOLS
    assert callable(Hasher.poseidon)


def words_of(value):
    return (ctypes.c_uint32 * 8)(*[value >> (32 * i) & 0xFFFFFFFF for i in range(8)])


def test_widths_tags_and_sizes_need_no_gpu():
    from icicle_amd._lib import lib
    from icicle_amd.hash import Hasher

    for field, p in pm.FIELDS.items():
        make = getattr(lib, f"{field}_create_poseidon_hasher")
        for t in (0, 1, 2, 4, 6, 8, 10, 11, 13):
            assert make(t, None, 0) is None and make(t, words_of(TAG), 0) is None, t
            with pytest.raises(ValueError):
                Hasher.poseidon(field, t)
        for t in pm.WIDTHS:
            if (field, t) not in pm.BUILT:
                assert make(t, None, 0) is None and make(t, words_of(TAG), 0) is None and make(t, None, t) is None
                with pytest.raises(ValueError):
                    Hasher.poseidon(field, t)
                continue
            for tag in (p, (1 << 256) - 1):
                assert make(t, words_of(tag), 0) is None
                with pytest.raises(ValueError):
                    Hasher.poseidon(field, t, domain_tag=tag)
            for tag_words, arity in ((None, t), (words_of(TAG), t - 1)):
                for size in (arity - 1, arity + 1):
                    assert make(t, tag_words, size) is None, (t, size)
            for h, arity in ((Hasher.poseidon(field, t), t), (Hasher.poseidon(field, t, domain_tag=TAG), t - 1), (Hasher.poseidon(field, t, input_size=t), t),
                             (Hasher.poseidon(field, t, domain_tag=np.array([TAG] + [0] * 7, dtype=np.uint32), input_size=t - 1), t - 1),
                             (Hasher.poseidon(field, t, domain_tag=p - 1), t - 1)):
                assert h.output_size == 32 and h.chunk == 32 * arity
                h.close()
    with pytest.raises(ValueError):
        Hasher.poseidon("stark252", 3)
    with pytest.raises(ValueError):
        Hasher.poseidon("babybear", 3)


def test_argument_errors_need_no_gpu():
    from icicle_amd import PowConfig
    from icicle_amd._lib import lib, HashConfig
    from icicle_amd.hash import Hasher

    cfg = HashConfig.default()
    for h, arity in ((Hasher.poseidon("bn254", 3), 3), (Hasher.poseidon("bls12_377", 5, domain_tag=TAG), 4)):
        inp, out = np.zeros(8 * (arity + 2), dtype=np.uint32), np.zeros(8, dtype=np.uint32)
        for nbytes in (32 * arity - 32, 32 * arity + 32, 32 * arity - 1):  # not one permutation's worth: refused in front of any device call
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


def test_trees_of_poseidon_layers_need_no_gpu_to_be_made():
    from icicle_amd._lib import lib
    from icicle_amd.hash import Hasher
    from icicle_amd.merkle import MerkleTree

    for field, t in pm.BUILT:
        for tag in (None, TAG):
            node = Hasher.poseidon(field, t, domain_tag=tag)
            tree = MerkleTree([node] * 3, 32)
            node.close()  # the tree keeps what it needs
            size = ctypes.c_size_t(0)
            assert lib.icicle_merkle_tree_get_root(tree.handle, ctypes.byref(size)) is None  # not built yet
            del tree
    # a byte hasher above a Poseidon layer and the reverse, where the sizes fit
    leaf, top = Hasher.poseidon("bn254", 5, domain_tag=TAG), Hasher.keccak256(64)
    tree = MerkleTree([leaf, top], 32)
    del tree
    with pytest.raises(Exception):
        MerkleTree([leaf, Hasher.poseidon("bn254", 3), Hasher.keccak256(48)], 32)  # 48 bytes are no whole number of 32-byte digests
