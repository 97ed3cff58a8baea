#!/usr/bin/env python3
"""Mint tests/golden/poseidon2_vectors_wide.json: Poseidon2 digests over the scalar fields of BN254, BLS12-381, BLS12-377 and
Grumpkin and over stark252 from the reference's CPU backend, driven through its own C ABI (<field>_create_poseidon2_hasher,
icicle_hasher_hash).

The method of mint_poseidon2_vectors.py: the reference's sources are compiled where they lie, unmodified, into a temporary
directory that is deleted afterwards, one library per field. Only data is recorded, per case: the width, the domain tag, the message
size in elements, the batch, the input elements and the digests. No round constant and no matrix entry goes into the file: the
library and tests/poseidon2_model_wide.py derive their own, and these digests prove them right. Needs the reference tree
($ICICLE_REFERENCE_DIR, default /root/reference) and a C++17 compiler; the tests read only the JSON.
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

REF = os.path.join(os.environ.get("ICICLE_REFERENCE_DIR", "/root/reference"), "icicle")
# the FIELD_IDs of mint_poseidon_vectors.py and oracle/build_ref.sh, and the primes
FIELDS = {
    "bn254": (["-DFIELD_ID=1", "-DFIELD=bn254", "-DCURVE_ID=1", "-DCURVE=bn254"],
              0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001),
    "bls12_381": (["-DFIELD_ID=2", "-DFIELD=bls12_381", "-DCURVE_ID=2", "-DCURVE=bls12_381"],
                  0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001),
    "bls12_377": (["-DFIELD_ID=3", "-DFIELD=bls12_377", "-DCURVE_ID=3", "-DCURVE=bls12_377"],
                  0x12AB655E9A2CA55660B44D1E5C37B00159AA76FED00000010A11800000000001),
    "grumpkin": (["-DFIELD_ID=5", "-DFIELD=grumpkin", "-DCURVE_ID=5", "-DCURVE=grumpkin"],
                 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47),
    "stark252": (["-DFIELD_ID=1002", "-DFIELD=stark252"],
                 0x800000000000011000000000000000000000000000000000000000000000001),
}
WIDTHS = (2, 3, 4, 8)
TAG = 7
SOURCES = [
    "src/device_api.cpp", "src/runtime.cpp", "src/config_extension.cpp", "backend/cpu/src/cpu_device_api.cpp",
    "src/hash/hash_c_api.cpp", "src/hash/keccak.cpp", "src/hash/blake2s.cpp", "src/hash/blake3.cpp",
    "src/hash/poseidon2.cpp", "src/hash/poseidon2_c_api.cpp", "backend/cpu/src/hash/cpu_poseidon2.cpp",
]


class HashConfig(ctypes.Structure):
    _fields_ = [("stream", ctypes.c_void_p), ("batch", ctypes.c_uint64), ("are_inputs_on_device", ctypes.c_bool),
                ("are_outputs_on_device", ctypes.c_bool), ("is_async", ctypes.c_bool), ("ext", ctypes.c_void_p)]


def cases_of(t):
    """(tag or None, size in elements, batch), without repetitions (at t = 2 several of the sizes coincide)"""
    out = [(None, t, 1), (TAG, t - 1, 1)]
    for size in (1, t + 1):
        out += [(None, size, 1), (TAG, size, 1)]
    out += [(None, 2 * t - 1, 3), (None, 3 * (t - 1) + 1, 1)]  # the last: a complete last block without a tag
    seen, uniq = set(), []
    for c in out:
        if c not in seen:
            seen.add(c)
            uniq.append(c)
    return uniq


def build(field, tmp):
    cxx = os.environ.get("ORACLE_CXX", "/opt/rocm/lib/llvm/bin/clang++")
    if not os.path.exists(cxx):
        cxx = "g++"
    so = os.path.join(tmp, f"libref_poseidon2_{field}.so")
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-fPIC", "-shared", "-pthread", "-w", f"-I{REF}/include", f"-I{REF}/backend/cpu/include",
                           f"-I{os.path.join(ROOT, 'oracle', 'shim')}", *FIELDS[field][0], f"-DICICLE_FFI_PREFIX={field}",
                           *[os.path.join(REF, s) for s in SOURCES], "-ldl", "-o", so])
    return so


def to_bytes(values):
    return b"".join(int(v).to_bytes(32, "little") for v in values)


def inputs_of(p, n, seed):
    """n elements: random canonical residues with 0, 1 and p - 1 among them wherever they fit"""
    rng = np.random.default_rng(seed)
    data = [int.from_bytes(rng.bytes(40), "little") % p for _ in range(n)]
    for k, v in enumerate((p - 1, 0, 1)[:n]):
        data[n - 1 - k] = v
    return data


def run_case(lib, field, t, tag, size, batch, seed):
    p = FIELDS[field][1]
    create = getattr(lib, f"{field}_create_poseidon2_hasher")
    create.restype = ctypes.c_void_p
    create.argtypes = [ctypes.c_uint, ctypes.c_void_p, ctypes.c_uint]
    lib.icicle_hasher_hash.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(HashConfig), ctypes.c_void_p]
    lib.icicle_hasher_delete.argtypes = [ctypes.c_void_p]
    tag_words = np.frombuffer(to_bytes([tag or 0]), dtype=np.uint32).copy()
    h = create(t, tag_words.ctypes.data if tag is not None else None, 0)
    assert h
    data = inputs_of(p, size * batch, seed)
    inp = np.frombuffer(to_bytes(data), dtype=np.uint8).copy()
    out = np.zeros(32 * batch, dtype=np.uint8)
    cfg = HashConfig(None, batch, False, False, False, None)
    assert lib.icicle_hasher_hash(h, inp.ctypes.data, 32 * size, ctypes.byref(cfg), out.ctypes.data) == 0
    lib.icicle_hasher_delete(h)
    raw = out.tobytes()
    digests = [int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(batch)]
    return {"field": field, "t": t, "tag": tag, "size": size, "batch": batch, "input": [f"{v:x}" for v in data],
            "digests": [f"{v:x}" for v in digests]}


def main():
    if not os.path.isdir(REF):
        sys.exit(f"reference tree not found ({REF}): nothing minted")
    cases = []
    with tempfile.TemporaryDirectory() as tmp:
        for field in FIELDS:
            lib = ctypes.CDLL(build(field, tmp))
            for t in WIDTHS:
                for tag, size, batch in cases_of(t):
                    cases.append(run_case(lib, field, t, tag, size, batch, 7700 + len(cases)))
            print(field, "ok")
            del lib
    doc = {"source": "reference CPU backend through its C ABI (tests/golden/mint_poseidon2_wide_vectors.py)", "cases": cases}
    out = os.path.join(HERE, "poseidon2_vectors_wide.json")
    with open(out, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print(f"{len(cases)} cases, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
