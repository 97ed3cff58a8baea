#!/usr/bin/env python3
"""Mint tests/golden/poseidon_vectors.json: Poseidon digests and Merkle trees over the scalar fields of BN254, BLS12-381, BLS12-377
and Grumpkin from the reference's CPU backend, driven through its own C ABI (<field>_create_poseidon_hasher, icicle_hasher_hash,
icicle_merkle_tree_*).

The method of mint_poseidon2_vectors.py: the reference's sources are compiled where they lie, unmodified, into a temporary
directory that is deleted afterwards, one library per field (the tree code against oracle/shim, as the FRI mint does). Only data is
recorded. Per hash case: the width, the domain tag, the batch, the input elements and the digests. Per tree: the layers' widths and
tag, the leaves, the padding policy, the root and one opened path (the reference's C ABI has no call that hands out the stored
layers; the path holds one group of each). No round constant and no matrix entry goes into the file: the library and
tests/poseidon_model.py derive their own, and these digests prove them right. Needs the reference tree ($ICICLE_REFERENCE_DIR,
default /root/reference) and a C++17 compiler; the tests read only the JSON.
"""
import ctypes
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import poseidon_model as pm  # noqa: E402  (the primes and the list of built pairs; nothing of it is recorded)

REF = os.path.join(os.environ.get("ICICLE_REFERENCE_DIR", "/root/reference"), "icicle")
DEFINES = {
    "bn254": ["-DFIELD_ID=1", "-DFIELD=bn254", "-DCURVE_ID=1", "-DCURVE=bn254"],
    "bls12_381": ["-DFIELD_ID=2", "-DFIELD=bls12_381", "-DCURVE_ID=2", "-DCURVE=bls12_381"],
    "bls12_377": ["-DFIELD_ID=3", "-DFIELD=bls12_377", "-DCURVE_ID=3", "-DCURVE=bls12_377"],
    "grumpkin": ["-DFIELD_ID=5", "-DFIELD=grumpkin", "-DCURVE_ID=5", "-DCURVE=grumpkin"],
}
TAG = 7
BATCH = 3
SOURCES = [
    "src/device_api.cpp", "src/runtime.cpp", "src/config_extension.cpp", "backend/cpu/src/cpu_device_api.cpp",
    "src/hash/hash_c_api.cpp", "src/hash/keccak.cpp", "src/hash/blake2s.cpp", "src/hash/blake3.cpp",
    "src/hash/poseidon.cpp", "src/hash/poseidon_c_api.cpp", "backend/cpu/src/hash/cpu_poseidon.cpp",
    "src/hash/merkle_c_api.cpp", "src/hash/merkle_tree.cpp", "backend/cpu/src/hash/cpu_merkle_tree.cpp",
]
# field, (t, tagged) of every layer (all layers alike), layers, leaves given, padding policy (0 none, 1 zero)
TREES = [
    ("bn254", 3, True, 3, 8, 0), ("bn254", 3, True, 3, 5, 1), ("bn254", 5, True, 2, 16, 0), ("bn254", 3, False, 2, 9, 0),
    ("bls12_381", 5, True, 2, 16, 0), ("bls12_377", 3, True, 3, 8, 0), ("bls12_377", 3, True, 3, 5, 1),
    ("grumpkin", 3, True, 3, 8, 0), ("grumpkin", 5, True, 2, 16, 0),
]


class HashConfig(ctypes.Structure):
    _fields_ = [("stream", ctypes.c_void_p), ("batch", ctypes.c_uint64), ("are_inputs_on_device", ctypes.c_bool),
                ("are_outputs_on_device", ctypes.c_bool), ("is_async", ctypes.c_bool), ("ext", ctypes.c_void_p)]


class MerkleTreeConfig(ctypes.Structure):
    _fields_ = [("stream", ctypes.c_void_p), ("is_leaves_on_device", ctypes.c_bool), ("is_tree_on_device", ctypes.c_bool), ("is_async", ctypes.c_bool),
                ("padding_policy", ctypes.c_int), ("ext", ctypes.c_void_p)]


def build(field, tmp):
    cxx = os.environ.get("ORACLE_CXX", "/opt/rocm/lib/llvm/bin/clang++")
    if not os.path.exists(cxx):
        cxx = "g++"
    so = os.path.join(tmp, f"libref_poseidon_{field}.so")
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-fPIC", "-shared", "-pthread", "-w", f"-I{REF}/include", f"-I{REF}/backend/cpu/include",
                           f"-I{os.path.join(ROOT, 'oracle', 'shim')}", *DEFINES[field], f"-DICICLE_FFI_PREFIX={field}",
                           *[os.path.join(REF, s) for s in SOURCES], "-ldl", "-o", so])
    return so


def bind(lib, field):
    create = getattr(lib, f"{field}_create_poseidon_hasher")
    create.restype = ctypes.c_void_p
    create.argtypes = [ctypes.c_uint, ctypes.c_void_p, ctypes.c_uint]
    lib.icicle_hasher_hash.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(HashConfig), ctypes.c_void_p]
    lib.icicle_hasher_delete.argtypes = [ctypes.c_void_p]
    lib.icicle_merkle_tree_create.restype = ctypes.c_void_p
    lib.icicle_merkle_tree_create.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t, ctypes.c_uint64, ctypes.c_uint64]
    lib.icicle_merkle_tree_build.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(MerkleTreeConfig)]
    lib.icicle_merkle_tree_get_root.restype = ctypes.c_void_p
    lib.icicle_merkle_tree_get_root.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)]
    lib.icicle_merkle_tree_get_proof.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_bool,
                                                 ctypes.POINTER(MerkleTreeConfig), ctypes.c_void_p]
    lib.icicle_merkle_tree_verify.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_bool)]
    lib.icicle_merkle_tree_delete.argtypes = [ctypes.c_void_p]
    lib.icicle_merkle_proof_create.restype = ctypes.c_void_p
    lib.icicle_merkle_proof_delete.argtypes = [ctypes.c_void_p]
    for f in ("icicle_merkle_proof_get_path", "icicle_merkle_proof_get_root"):
        getattr(lib, f).restype = ctypes.c_void_p
        getattr(lib, f).argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)]
    return create


def inputs_of(p, n, seed):
    """n elements: random residues with 0, 1 and p - 1 among them"""
    rng = np.random.default_rng(seed)
    data = [int.from_bytes(rng.bytes(40), "little") % p for _ in range(n)]
    for k, v in enumerate((p - 1, 0, 1)):
        data[(seed + 5 * k) % n if n >= 16 else (n - 1 - k)] = v
    return data


def make_hasher(create, t, tag):
    tag_words = np.frombuffer(pm.to_bytes([tag or 0]), dtype=np.uint32).copy()
    h = create(t, tag_words.ctypes.data if tag is not None else None, 0)
    assert h
    return h


def run_case(lib, create, field, t, tag, seed):
    p, arity = pm.FIELDS[field], t - (tag is not None)
    h = make_hasher(create, t, tag)
    data = inputs_of(p, arity * BATCH, seed)
    inp = np.frombuffer(pm.to_bytes(data), dtype=np.uint8).copy()
    out = np.zeros(32 * BATCH, dtype=np.uint8)
    cfg = HashConfig(None, BATCH, False, False, False, None)
    assert lib.icicle_hasher_hash(h, inp.ctypes.data, 32 * arity, ctypes.byref(cfg), out.ctypes.data) == 0
    lib.icicle_hasher_delete(h)
    return {"field": field, "t": t, "tag": tag, "batch": BATCH, "input": [f"{v:x}" for v in data],
            "digests": [f"{v:x}" for v in pm.from_bytes(out.tobytes())]}


def read_bytes(fn, handle):
    n = ctypes.c_size_t()
    p = fn(handle, ctypes.byref(n))
    return ctypes.string_at(p, n.value)


def run_tree(lib, create, field, t, tagged, layers, given, policy, seed):
    p, tag = pm.FIELDS[field], TAG if tagged else None
    hashers = [make_hasher(create, t, tag) for _ in range(layers)]
    arr = (ctypes.c_void_p * layers)(*hashers)
    tree = lib.icicle_merkle_tree_create(arr, layers, 32, 0)
    assert tree
    data = inputs_of(p, given, seed)
    leaves = np.frombuffer(pm.to_bytes(data), dtype=np.uint8).copy()
    cfg = MerkleTreeConfig(None, False, False, False, policy, None)
    assert lib.icicle_merkle_tree_build(tree, leaves.ctypes.data, leaves.nbytes, ctypes.byref(cfg)) == 0
    root = read_bytes(lib.icicle_merkle_tree_get_root, tree)
    leaf_idx = given - 1
    proof = lib.icicle_merkle_proof_create()
    assert lib.icicle_merkle_tree_get_proof(tree, leaves.ctypes.data, leaves.nbytes, leaf_idx, False, ctypes.byref(cfg), proof) == 0
    ok = ctypes.c_bool(False)
    assert lib.icicle_merkle_tree_verify(tree, proof, ctypes.byref(ok)) == 0 and ok.value
    path = read_bytes(lib.icicle_merkle_proof_get_path, proof)
    assert read_bytes(lib.icicle_merkle_proof_get_root, proof) == root
    lib.icicle_merkle_proof_delete(proof)
    lib.icicle_merkle_tree_delete(tree)
    for h in hashers:
        lib.icicle_hasher_delete(h)
    return {"field": field, "t": t, "tag": tag, "layers": layers, "policy": policy, "leaves": [f"{v:x}" for v in data],
            "root": f"{pm.from_bytes(root)[0]:x}", "leaf_idx": leaf_idx, "path": [f"{v:x}" for v in pm.from_bytes(path)]}


def main():
    if not os.path.isdir(REF):
        sys.exit(f"reference tree not found ({REF}): nothing minted")
    cases, trees = [], []
    with tempfile.TemporaryDirectory() as tmp:
        for field in pm.FIELDS:
            lib = ctypes.CDLL(build(field, tmp))
            create = bind(lib, field)
            for f, t in pm.BUILT:
                if f == field:
                    for tag in (None, TAG):
                        cases.append(run_case(lib, create, field, t, tag, 9000 + len(cases)))
            for f, t, tagged, layers, given, policy in TREES:
                if f == field:
                    trees.append(run_tree(lib, create, field, t, tagged, layers, given, policy, 9500 + len(trees)))
            print(field, "ok")
            del lib
    doc = {"source": "reference CPU backend through its C ABI (tests/golden/mint_poseidon_vectors.py)", "cases": cases, "trees": trees}
    out = os.path.join(HERE, "poseidon_vectors.json")
    with open(out, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print(f"{len(cases)} cases, {len(trees)} trees, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
