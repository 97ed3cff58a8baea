#!/usr/bin/env python3
"""Mint tests/golden/poseidon2_vectors_gold.json: Poseidon2 digests over Goldilocks from the reference's CPU backend, driven
through its own C ABI (goldilocks_create_poseidon2_hasher, icicle_hasher_hash).

The method, the sources and the case list per width are those of mint_poseidon2_vectors.py, which is imported: the reference's
sources are compiled where they lie, unmodified, into a temporary directory that is deleted afterwards. Elements are 8 bytes, the
domain tag one element of two little-endian words. Beside the cases of cases_of(t), per width:
  * one case whose tag is above 2^32, so that the tag's upper word is read;
  * one whose inputs include 2^32 - 1, 2^32 and 2^64 - 2^32 (= p - 1), the values at which the fix-ups of the 128-bit reduction
    change branch.
Only data is recorded, as hex strings: the width, the tag, the message size in elements, the batch, the inputs and the digests. No
round constant and no matrix entry goes into the file. Needs the reference tree ($ICICLE_REFERENCE_DIR, default /root/reference)
and a C++17 compiler; the tests read only the JSON.
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
sys.path.insert(0, HERE)
import mint_poseidon2_vectors as base  # noqa: E402

REF = base.REF
FIELD, FIELD_ID, P = "goldilocks", 1005, (1 << 64) - (1 << 32) + 1
WIDTHS = base.WIDTHS
BIG_TAG = (1 << 63) + (5 << 32) + 11
EDGES = [(1 << 32) - 1, 1 << 32, (1 << 64) - (1 << 32)]


def build(tmp):
    cxx = os.environ.get("ORACLE_CXX", "/opt/rocm/lib/llvm/bin/clang++")
    if not os.path.exists(cxx):
        cxx = "g++"
    so = os.path.join(tmp, "libref_poseidon2_goldilocks.so")
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-fPIC", "-shared", "-pthread", "-w", f"-I{REF}/include", f"-I{REF}/backend/cpu/include",
                           f"-I{os.path.join(ROOT, 'oracle', 'shim')}", f"-DFIELD_ID={FIELD_ID}", f"-DFIELD={FIELD}",
                           f"-DICICLE_FFI_PREFIX={FIELD}", *[os.path.join(REF, s) for s in base.SOURCES], "-ldl", "-o", so])
    return so


def cases_of(t):
    """(tag or None, size in elements, batch, with the reduction's edge values)"""
    return [(tag, size, batch, False) for tag, size, batch in base.cases_of(t)] + [(BIG_TAG, 2 * t - 1, 1, False), (None, 2 * t + 1, 1, True)]


def inputs_of(n, seed, edges):
    data = base.inputs_of(P, n, seed)  # random residues with 0, 1 and p - 1 among them wherever they fit
    if edges:
        for k, v in enumerate(EDGES):  # n = 2 t + 1 >= 5: slots 0 .. 2; p - 1, 0, 1 sit at the end or are drawn again at n >= 16
            data[k] = v
    return data


def run_case(lib, t, tag, size, batch, edges, seed):
    create = lib.goldilocks_create_poseidon2_hasher
    create.restype = ctypes.c_void_p
    create.argtypes = [ctypes.c_uint, ctypes.c_void_p, ctypes.c_uint]
    lib.icicle_hasher_hash.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(base.HashConfig), ctypes.c_void_p]
    lib.icicle_hasher_delete.argtypes = [ctypes.c_void_p]
    lib.icicle_hasher_output_size.argtypes = [ctypes.c_void_p]
    lib.icicle_hasher_output_size.restype = ctypes.c_uint64
    tag_words = np.array([tag or 0], dtype=np.uint64)
    h = create(t, tag_words.ctypes.data if tag is not None else None, 0)
    assert h and lib.icicle_hasher_output_size(h) == 8
    data = inputs_of(size * batch, seed, edges)
    inp = np.array(data, dtype=np.uint64)
    out = np.zeros(batch, dtype=np.uint64)
    cfg = base.HashConfig(None, batch, False, False, False, None)
    assert lib.icicle_hasher_hash(h, inp.ctypes.data, 8 * size, ctypes.byref(cfg), out.ctypes.data) == 0
    lib.icicle_hasher_delete(h)
    return {"t": t, "tag": None if tag is None else f"{tag:x}", "size": size, "batch": batch, "input": [f"{v:x}" for v in data],
            "digests": [f"{int(v):x}" for v in out]}


def main():
    if not os.path.isdir(REF):
        sys.exit(f"reference tree not found ({REF}): nothing minted")
    cases = []
    with tempfile.TemporaryDirectory() as tmp:
        lib = ctypes.CDLL(build(tmp))
        for t in WIDTHS:
            for tag, size, batch, edges in cases_of(t):
                cases.append(run_case(lib, t, tag, size, batch, edges, 9000 + len(cases)))
        del lib
    doc = {"source": "reference CPU backend through its C ABI (tests/golden/mint_poseidon2_gold_vectors.py)", "field": FIELD, "cases": cases}
    out = os.path.join(HERE, "poseidon2_vectors_gold.json")
    with open(out, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print(f"{len(cases)} cases, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
