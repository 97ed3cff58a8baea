"""CPU: Blake2s / Blake3 without a GPU -- the test model (tests/blake_model.py) against hashlib and the recorded Blake3 digests
(tests/golden/blake3_vectors.json), the two factories in header, library and binding, handle life cycle, trees of mixed hashers, loud
failure of the compute entry points, and the device code itself (icicle_amd/csrc/blake.hpp over the three readers, compiled with g++:
tests/blake_host_harness.cpp) against the model."""
import ctypes
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests import blake_model as bm

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BLAKE2S_LENGTHS = list(range(301)) + [1000]


@pytest.fixture(scope="module")
def vectors():
    with open(os.path.join(HERE, "golden", "blake3_vectors.json")) as f:
        return json.load(f)


def pattern(n):
    return bytes(i % 251 for i in range(n))


# ---- the model -----------------------------------------------------------------------------------------------------------------
def test_model_constants_are_the_derived_ones():
    assert [hex(v) for v in bm.IV] == ["0x6a09e667", "0xbb67ae85", "0x3c6ef372", "0xa54ff53a", "0x510e527f", "0x9b05688c", "0x1f83d9ab", "0x5be0cd19"]
    assert bm.SCHED3[1] == bm.PERM and bm.SCHED3[2] == [bm.PERM[i] for i in bm.PERM]


def test_model_blake2s_matches_hashlib():
    for n in BLAKE2S_LENGTHS:
        msg = bytes((7 * i + n) & 0xFF for i in range(n))
        assert bm.digest("blake2s", msg) == hashlib.blake2s(msg).digest(), n
    # batch form: every row is its own message
    for n in BLAKE2S_LENGTHS:
        rows = np.random.default_rng(n).integers(0, 256, (5, n), dtype=np.uint8)
        assert bm.hash_batch("blake2s", rows.tobytes(), n, 5) == b"".join(hashlib.blake2s(r.tobytes()).digest() for r in rows), n


def test_model_blake2s_known_answer():
    """the reference's own test (icicle/tests/test_hash_api.cpp:82-83)"""
    assert bm.digest("blake2s", b"Hello world I am blake2s").hex() == "291c4b3648438cc57d1e965ee52e5572e8dc4938bc960e22d6ebe3a280aea759"


def test_model_blake3_matches_recorded_digests(vectors):
    assert len(vectors["by_length"]) == 27
    for n, want in vectors["by_length"].items():
        assert bm.digest("blake3", pattern(int(n))).hex() == want, n
    ka = vectors["known_answer"]
    assert ka["digest"] == "4b71f2c5cb7c26da2ba67cc742228e55b66c8b64b2b250e7ccce6f7f6d17c9ae"  # test_hash_api.cpp:108
    assert bm.digest("blake3", ka["message"].encode()).hex() == ka["digest"]
    # batch form: the rows are shifted copies of the pattern, each its own message
    for n in (65, 1025, 3073):
        rows = np.stack([np.frombuffer(pattern(n + 3)[k:k + n], dtype=np.uint8) for k in range(3)])
        got = bm.hash_batch("blake3", rows.tobytes(), n, 3)
        assert got[:32].hex() == vectors["by_length"][str(n)]
        assert got[32:64] == bm.digest("blake3", rows[1].tobytes()) != got[:32]


def test_model_blake3_of_empty_string():
    assert bm.digest("blake3", b"").hex() == "af1349b9f5f9a1a6a0404dea36dcc9499bcb25c9adc112b7cc9a93cae41f3262"


MIXED6 = ([("blake2s", 100), ("blake3", 128), ("keccak512", 64), ("sha3_256", 128), ("sha3_512", 64), ("keccak256", 128)], 20)


def test_tree_model_over_all_six_hashers_is_self_consistent():
    layers, es = MIXED6
    shape = bm.TreeShape(layers, es)
    assert shape.out == [32, 32, 64, 32, 64, 32] and shape.count == [64, 16, 8, 4, 2, 1]
    rng = np.random.default_rng(4)
    for policy, size in ((bm.PAD_NONE, shape.capacity), (bm.PAD_ZERO, shape.capacity // 2 + 3), (bm.PAD_LAST, 7 * es)):
        leaves = rng.integers(0, 256, size, dtype=np.uint8).tobytes()
        for idx in (0, 1, shape.capacity // es // 2, shape.capacity // es - 1):
            for pruned in (False, True):
                leaf, path, root = bm.proof(shape, leaves, idx, pruned, policy)
                assert bm.verify(shape, leaf, idx, path, root, pruned)
                bad = bytearray(path)
                bad[len(bad) // 2] ^= 1
                assert not bm.verify(shape, leaf, idx, bytes(bad), root, pruned)


# ---- header, library, binding ------------------------------------------------------------------------------------------------------
def test_blake_factories_are_declared_exported_and_bound():
    from icicle_amd import _lib

    text = subprocess.check_output(["gcc", "-E", "-P", os.path.join(ROOT, "include", "icicle_hip.h")], text=True)
    for name in ("icicle_create_blake2s", "icicle_create_blake3"):
        assert re.search(r"icicle_hasher_handle_t\s+%s\s*\(\s*uint64_t\s+input_chunk_size\s*\)\s*;" % name, text), name
        fn = getattr(_lib.lib, name)  # exported
        assert fn.restype is ctypes.c_void_p and fn.argtypes == [ctypes.c_uint64]
    assert set(_lib.BLAKE_HANDLE_SYMBOLS) == {"icicle_create_blake2s", "icicle_create_blake3"}
    assert not set(_lib.BLAKE_HANDLE_SYMBOLS) & set(_lib.HASH_HANDLE_SYMBOLS)


def test_blake_handles_need_no_gpu():
    from icicle_amd.hash import Hasher

    for make in (Hasher.blake2s, Hasher.blake3):
        for chunk in (0, 64, 1536):
            h = make(chunk)
            assert h.output_size == 32 and h.chunk == chunk
            h.close()


def test_trees_of_mixed_hashers_are_accepted_and_non_trees_refused():
    import icicle_amd
    from icicle_amd.hash import Hasher
    from icicle_amd.merkle import MerkleTree

    layers, es = MIXED6
    t = MerkleTree([getattr(Hasher, name)(chunk) for name, chunk in layers], es, output_store_min_layer=2)
    assert t.root() is None  # not built
    t.close()
    MerkleTree([Hasher.blake3(1536), Hasher.blake3(2048), Hasher.blake2s(64)], 4).close()  # arity 64 above 1536-byte leaf chunks
    with pytest.raises(icicle_amd.IcicleError):
        MerkleTree([Hasher.keccak512(64), Hasher.blake3(96)], 32)  # 96 % 64 != 0
    with pytest.raises(icicle_amd.IcicleError):
        MerkleTree([Hasher.blake2s(64), Hasher.blake3(80)], 32)  # 80 % 32 != 0
    with pytest.raises(icicle_amd.IcicleError):
        MerkleTree([Hasher.blake3(0)], 32)  # a layer needs a chunk size
    MerkleTree([Hasher.blake2s(64), Hasher.keccak512(96)], 32).close()  # 96 % 32 == 0


def test_no_gpu_means_loud_failure():
    import icicle_amd
    from icicle_amd import runtime
    from icicle_amd.hash import Hasher
    from icicle_amd.merkle import MerkleTree

    for make in (Hasher.blake2s, Hasher.blake3):
        h = make()
        # argument errors come first, with or without a device
        with pytest.raises(icicle_amd.IcicleError) as e:
            h.hash(np.zeros(0, np.uint8), size=0)
        assert e.value.code == 11
        if runtime.get_device_count() > 0:
            continue  # with a device these calls succeed (tests/test_gpu_blake.py, tests/test_gpu_blake_merkle.py)
        with pytest.raises(icicle_amd.IcicleError):
            h.hash(np.zeros(64, np.uint8))
        with pytest.raises(icicle_amd.IcicleError):
            h.hash(np.zeros(4096, np.uint8))
        with pytest.raises(icicle_amd.IcicleError):
            MerkleTree([make(64)] * 2, 32).build(np.zeros(128, np.uint8))


# ---- blake.hpp on the host against the model -------------------------------------------------------------------------------------
KIND = {"blake2s": 1, "blake3": 2}


@pytest.fixture(scope="module")
def harness():
    so = os.path.join(HERE, "_build", "libblake_host.so")
    os.makedirs(os.path.dirname(so), exist_ok=True)
    src = os.path.join(HERE, "blake_host_harness.cpp")
    hdrs = [os.path.join(ROOT, "icicle_amd", "csrc", h) for h in ("blake.hpp", "hash_readers.hpp")]
    if not os.path.exists(so) or max(os.path.getmtime(f) for f in [src] + hdrs) > os.path.getmtime(so):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", src, "-o", so])
    lib = ctypes.CDLL(so)
    lib.bh_hash.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
    lib.bh_hash_padded.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
    return lib


def host_hash(lib, name, msg: bytes, reader, shift=0):
    """reader 0 = ReadAligned (shift 0: 16-aligned, 8: 8-aligned only), 1 = ReadBytes (from an odd address)"""
    buf = np.zeros(len(msg) + 64, dtype=np.uint8)
    at = -buf.ctypes.data % 16 + (shift if reader == 0 else 1)
    buf[at:at + len(msg)] = np.frombuffer(msg, dtype=np.uint8)
    out = np.zeros(32, dtype=np.uint8)
    assert lib.bh_hash(KIND[name], reader, buf.ctypes.data + at, len(msg), out.ctypes.data) == 0
    return out.tobytes()


def test_device_blake2s_code_on_the_host(harness):
    for n in BLAKE2S_LENGTHS:
        msg = bytes((7 * i + n) & 0xFF for i in range(n))
        want = hashlib.blake2s(msg).digest()
        assert host_hash(harness, "blake2s", msg, 0) == want, n
        assert host_hash(harness, "blake2s", msg, 0, shift=8) == want, n
        assert host_hash(harness, "blake2s", msg, 1) == want, n


def test_device_blake3_code_on_the_host(harness, vectors):
    for n, want in vectors["by_length"].items():
        msg = pattern(int(n))
        assert host_hash(harness, "blake3", msg, 0).hex() == want, n
        assert host_hash(harness, "blake3", msg, 0, shift=8).hex() == want, n
        assert host_hash(harness, "blake3", msg, 1).hex() == want, n
    for n in range(0, 301):  # every block edge of the first chunk, against the model
        msg = bytes((7 * i + n) & 0xFF for i in range(n))
        assert host_hash(harness, "blake3", msg, 1) == bm.digest("blake3", msg), n


@pytest.mark.parametrize("name,chunk,es", [("blake2s", 100, 20), ("blake3", 100, 20), ("blake3", 1536, 4), ("blake3", 3072, 8), ("blake2s", 1536, 4)])
def test_device_padded_leaf_reader_on_the_host(harness, name, chunk, es):
    """layer-0 chunks of a tree of four chunks whose leaves end in front of, inside and at the end of them, both padding policies"""
    shape = bm.TreeShape([(name, chunk), ("keccak256", 128)], es)
    assert shape.capacity == 4 * chunk
    rng = np.random.default_rng(chunk)
    sizes = sorted({es, chunk - es, chunk, chunk + es, 2 * chunk + min(1024, chunk) // es * es, shape.capacity - es} - {0})
    for policy in (bm.PAD_ZERO, bm.PAD_LAST):
        for size in sizes:
            leaves = rng.integers(0, 256, size, dtype=np.uint8)
            want = bm.build(shape, leaves.tobytes(), policy)[0]
            last = leaves.ctypes.data + size - es if policy == bm.PAD_LAST else None
            out = np.zeros(32, dtype=np.uint8)
            for c in range(4):
                harness.bh_hash_padded(KIND[name], leaves.ctypes.data, c * chunk, chunk, size, last, es, out.ctypes.data)
                assert out.tobytes() == want[32 * c:32 * c + 32], (policy, size, c)
