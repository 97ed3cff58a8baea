"""CPU: the hash / Merkle part of the C ABI without a GPU -- the test model against hashlib, struct layouts, exported and bound
symbols, handle life cycle, loud failure of the compute entry points, and the host-only tree arithmetic
(icicle_amd/csrc/merkle_plan.h and the leaf-index arithmetic of merkle_batch.h, compiled with g++) against the model
(tests/merkle_model.py)."""
import ctypes
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

from tests import merkle_model as mm

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# the shapes the model was first exercised on: (layers, leaf element size)
SHAPES = {
    "binary5": ([("keccak256", 64)] * 5, 32),
    "mixed": ([("sha3_512", 100), ("sha3_256", 256), ("sha3_256", 128), ("sha3_512", 64)], 20),
    "single": ([("sha3_256", 1000)], 8),
    "arity3": ([("keccak256", 96)] * 3, 32),
}


def test_model_sha3_matches_hashlib():
    for n in range(301):
        msg = bytes((7 * i + n) & 0xFF for i in range(n))
        assert mm.digest("sha3_256", msg) == hashlib.sha3_256(msg).digest(), n
        assert mm.digest("sha3_512", msg) == hashlib.sha3_512(msg).digest(), n
    # batch form: every row is its own message
    rows = np.arange(5 * 137, dtype=np.uint32).astype(np.uint8).reshape(5, 137)
    got = mm.hash_batch("sha3_256", rows.tobytes(), 137, 5)
    assert got == b"".join(hashlib.sha3_256(r.tobytes()).digest() for r in rows)
    for n in (0, 71, 72, 135, 136, 300):  # the array form is the same sponge as the one-message form
        for name in mm.VARIANTS:
            assert mm.hash_batch(name, rows.tobytes()[:2 * n], n, 2) == mm.digest(name, rows.tobytes()[:n]) + mm.digest(name, rows.tobytes()[n:2 * n])


def test_model_keccak256_of_empty_string():
    assert mm.digest("keccak256", b"").hex() == "c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470"
    assert mm.digest("keccak256", b"") != hashlib.sha3_256(b"").digest()  # the suffix matters
    assert len(mm.digest("keccak512", b"abc")) == 64


def test_model_is_self_consistent():
    """every proof of the model verifies under the reference's verify walk; path sizes follow the formulas"""
    rng = np.random.default_rng(11)
    for layers, es in SHAPES.values():
        shape = mm.TreeShape(layers, es)
        for policy, size in ((mm.PAD_NONE, shape.capacity), (mm.PAD_ZERO, 1), (mm.PAD_ZERO, shape.capacity // 2 + 3),
                             (mm.PAD_LAST, es), (mm.PAD_LAST, shape.capacity // 3 // es * es)):
            if shape.padding(size, policy) is None:
                assert policy == mm.PAD_LAST and shape.chunk[0] % es  # the deliberate narrowing (mixed: 100 % 20 == 0, so never)
                continue
            leaves = rng.integers(0, 256, size, dtype=np.uint8).tobytes()
            for idx in (0, 1, shape.capacity // es // 2, (shape.capacity - 1) // es):
                for pruned in (False, True):
                    leaf, path, root = mm.proof(shape, leaves, idx, pruned, policy)
                    assert len(path) == (shape.pruned_path if pruned else shape.full_path)
                    assert mm.verify(shape, leaf, idx, path, root, pruned)
                    if path:
                        bad = bytearray(path)
                        bad[len(bad) // 2] ^= 1
                        assert not mm.verify(shape, leaf, idx, bytes(bad), root, pruned)


def test_struct_layouts():
    from icicle_amd import _lib

    H = _lib.HashConfig
    assert ctypes.sizeof(H) == 32
    assert [getattr(H, f).offset for f, _ in H._fields_] == [0, 8, 16, 17, 18, 24]
    M = _lib.MerkleTreeConfig
    assert ctypes.sizeof(M) == 24
    assert [getattr(M, f).offset for f, _ in M._fields_] == [0, 8, 9, 10, 12, 16]
    from icicle_amd.merkle import PaddingPolicy
    assert (PaddingPolicy.NONE, PaddingPolicy.ZERO_PADDING, PaddingPolicy.LAST_VALUE) == (0, 1, 2)


def declared_hash_functions():
    """name -> return type of every function the header's hash / Merkle section declares (handle-returning ones included)"""
    text = subprocess.check_output(["gcc", "-E", "-P", os.path.join(ROOT, "include", "icicle_hip.h")], text=True)
    out = {}
    for ret, name in re.findall(r"(?:^|[;}])\s*((?:const\s+)?\w+(?:\s*\*)?)\s*\b(\w+)\s*\(", text):
        if re.match(r"icicle_(create_(keccak|sha3)|hasher_|merkle_)", name):
            out[name] = re.sub(r"\s+", " ", ret).strip()
    return out


def test_every_declared_hash_function_is_exported_and_bound():
    from icicle_amd import _lib

    decl = declared_hash_functions()
    assert len(decl) == 20, sorted(decl)
    plain = {n for n, r in decl.items() if r in ("icicle_error_t", "_Bool")}
    handles = set(decl) - plain
    assert handles == set(_lib.HASH_HANDLE_SYMBOLS)
    assert plain <= set(_lib.API_SYMBOLS)
    for name, ret in decl.items():
        fn = getattr(_lib.lib, name)  # exported
        assert fn.argtypes is not None, f"{name} has no argtypes"
        if name in handles:
            want = ctypes.c_uint64 if ret == "uint64_t" else ctypes.c_void_p
            assert fn.restype is want, (name, ret, fn.restype)


def test_handles_need_no_gpu():
    from icicle_amd.hash import Hasher
    from icicle_amd.merkle import MerkleProof, MerkleTree

    sizes = []
    for make in (Hasher.keccak256, Hasher.sha3_256, Hasher.keccak512, Hasher.sha3_512):
        h = make(64)
        sizes.append(h.output_size)
        h.close()
    assert sizes == [32, 32, 64, 64]
    t = MerkleTree([Hasher.keccak256(64)] * 4, 32, output_store_min_layer=2)
    assert t.root() is None  # not built
    t.close()
    p = MerkleProof.with_data(True, 5, b"leaf", b"root" * 8, b"path" * 16)
    assert (p.pruned, p.leaf_idx, p.leaf, p.root, p.path) == (True, 5, b"leaf", b"root" * 8, b"path" * 16)
    p.close()
    e = MerkleProof()
    assert (e.pruned, e.leaf, e.path, e.root) == (False, b"", b"", b"")


def test_layers_that_form_no_tree_are_refused():
    import icicle_amd
    from icicle_amd.hash import Hasher

    from icicle_amd.merkle import MerkleTree
    with pytest.raises(icicle_amd.IcicleError):
        MerkleTree([Hasher.keccak512(64), Hasher.keccak512(96)], 32)  # 96 % 64 != 0
    with pytest.raises(icicle_amd.IcicleError):
        MerkleTree([Hasher.keccak256(0)], 32)  # a layer needs a chunk size
    MerkleTree([Hasher.keccak256(64), Hasher.keccak256(96)], 32).close()  # 96 % 32 == 0


def test_no_gpu_means_loud_failure():
    import icicle_amd
    from icicle_amd import runtime
    from icicle_amd.hash import Hasher
    from icicle_amd.merkle import MerkleTree

    h = Hasher.sha3_256()
    # argument errors come first, with or without a device
    with pytest.raises(icicle_amd.IcicleError) as e:
        h.hash(np.zeros(0, np.uint8), size=0)
    assert e.value.code == 11
    if runtime.get_device_count() > 0:
        return  # with a device these calls succeed (tests/test_gpu_hash.py, tests/test_gpu_merkle.py)
    with pytest.raises(icicle_amd.IcicleError):
        h.hash(np.zeros(64, np.uint8))
    with pytest.raises(icicle_amd.IcicleError):
        MerkleTree([Hasher.keccak256(64)] * 2, 32).build(np.zeros(128, np.uint8))


# ---- merkle_plan.h and merkle_batch.h against the model -------------------------------------------------------------------------
def _plan_lib():
    so = os.path.join(HERE, "_build", "libmerkle_plan.so")
    os.makedirs(os.path.dirname(so), exist_ok=True)
    src = os.path.join(HERE, "merkle_plan_harness.cpp")
    hdrs = [os.path.join(ROOT, "icicle_amd", "csrc", h) for h in ("merkle_plan.h", "merkle_batch.h")]  # mp_proof walks merkle_batch.h
    if not os.path.exists(so) or max(os.path.getmtime(f) for f in [src] + hdrs) > os.path.getmtime(so):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", src, "-o", so])
    lib = ctypes.CDLL(so)
    u64p = ctypes.POINTER(ctypes.c_uint64)
    lib.mp_plan.argtypes = [u64p, u64p, ctypes.c_int, ctypes.c_uint64, u64p]
    lib.mp_padding.argtypes = [u64p, u64p, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int, u64p]
    lib.mp_proof.argtypes = [u64p, u64p, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int, ctypes.c_int, u64p]
    return lib


def _arrays(shape):
    L = len(shape.layers)
    return (ctypes.c_uint64 * L)(*shape.chunk), (ctypes.c_uint64 * L)(*shape.out), L


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_merkle_plan_header_matches_model(name):
    lib = _plan_lib()
    layers, es = SHAPES[name]
    shape = mm.TreeShape(layers, es)
    chunk, outsz, L = _arrays(shape)
    out = (ctypes.c_uint64 * (16 + 8 * L))()
    assert lib.mp_plan(chunk, outsz, L, es, out) == 0
    assert list(out[:3 + L]) == [shape.capacity, shape.full_path, shape.pruned_path] + shape.count
    cap = shape.capacity
    for policy in (mm.PAD_NONE, mm.PAD_ZERO, mm.PAD_LAST, 3):
        for size in (0, 1, es, es + 1, cap // 3, cap // 3 // es * es, cap // 2, cap - 35, cap - es, cap - 1, cap, cap + 1):
            want = shape.padding(size, policy) if size >= 0 else None
            rc = lib.mp_padding(chunk, outsz, L, es, size, policy, out)
            assert rc == (1 if want is None else 0), (policy, size)
            if want is not None:
                assert tuple(out[:3]) == want, (policy, size)
    n_elems = cap // es
    for idx in sorted({0, 1, n_elems // 2, n_elems - 1, (cap - 1) // es}):
        for pruned in (False, True):
            for store_min in range(L + 1):
                assert lib.mp_proof(chunk, outsz, L, es, idx, pruned, store_min, out) == 0
                steps, size = shape.proof_steps(idx, pruned)
                first, cnt = shape.subtree(idx, store_min)
                assert list(out[:4]) == [idx * es // shape.chunk[0], size, first, cnt]
                flat = [v for s in steps for v in s]
                assert list(out[4:4 + len(flat)]) == flat
                # verify()'s offsets from the byte position alone equal the proof's skip offsets
                assert list(out[4 + len(flat):4 + len(flat) + L - 1]) == [s[3] for s in steps]
    for idx in ((cap + es - 1) // es, cap // es + 7):  # at or beyond the capacity
        assert lib.mp_proof(chunk, outsz, L, es, idx, 0, 0, out) == 1


def test_merkle_plan_header_refuses_what_is_no_tree():
    lib = _plan_lib()
    out = (ctypes.c_uint64 * 80)()
    two = ctypes.c_uint64 * 2
    assert lib.mp_plan(two(64, 96), two(64, 64), 2, 32, out) == 1  # 96 % 64
    assert lib.mp_plan(two(64, 0), two(32, 32), 2, 32, out) == 1   # no chunk size
    assert lib.mp_plan(two(64, 64), two(32, 32), 2, 0, out) == 1   # no element size
    assert lib.mp_plan(two(64, 64), two(32, 32), 0, 32, out) == 1  # no layer
    many = ctypes.c_uint64 * 65
    assert lib.mp_plan(many(*[64] * 65), many(*[32] * 65), 65, 32, out) == 1  # more layers than the fused top takes
