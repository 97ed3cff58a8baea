#!/usr/bin/env python3
"""Mint tests/golden/fri_vectors.json: FRI proofs from the reference's CPU backend, driven through its own C ABI.

The method of mint_blake3_vectors.py: the reference's sources are compiled where they lie, unmodified, into a temporary directory
that is deleted afterwards -- the recipe of oracle/build_ref.sh (device + field library against oracle/shim) extended by -DFRI=ON and
the hash, Merkle, proof-of-work and FRI sources (src/hash, backend/cpu/src/hash, src/fri, backend/cpu/src/field/cpu_fri.cpp), one
library per field. Only data is recorded, per case: the inputs, labels, seed and configuration, and from the proof every slot's
leaf index, leaf, root and path, the final polynomial and the nonce. Needs the reference tree ($ICICLE_REFERENCE_DIR, default
/root/reference), gcc and a C++17 compiler; the tests read only the JSON. One case asks for a query equal to n: its seed is searched
with the model (tests/fri_model.py), and the proof still comes from the reference.
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
from tests import fri_model as fm  # noqa: E402

REF = os.path.join(os.environ.get("ICICLE_REFERENCE_DIR", "/root/reference"), "icicle")
FIELD_IDS = {"babybear": 1001, "koalabear": 1004}
BLAKE3_FLAGS = ["-DBLAKE3_NO_SSE2", "-DBLAKE3_NO_SSE41", "-DBLAKE3_NO_AVX2", "-DBLAKE3_NO_AVX512", "-DBLAKE3_USE_NEON=0"]
SOURCES = [
    "src/device_api.cpp", "src/runtime.cpp", "src/config_extension.cpp", "backend/cpu/src/cpu_device_api.cpp",
    "src/fields/ffi_extern.cpp", "src/ntt.cpp", "backend/cpu/src/field/cpu_ntt.cpp",
    "src/hash/keccak.cpp", "src/hash/blake2s.cpp", "src/hash/blake3.cpp", "src/hash/hash_c_api.cpp", "src/hash/merkle_c_api.cpp", "src/hash/merkle_tree.cpp",
    "src/hash/pow.cpp", "backend/cpu/src/hash/cpu_keccak.cpp", "backend/cpu/src/hash/cpu_blake2s.cpp", "backend/cpu/src/hash/cpu_blake3.cpp",
    "backend/cpu/src/hash/cpu_merkle_tree.cpp", "backend/cpu/src/hash/cpu_pow.cpp",
    "src/fri/fri.cpp", "src/fri/fri_c_api.cpp", "backend/cpu/src/field/cpu_fri.cpp",
]
HASHERS = {"keccak256": "icicle_create_keccak_256", "keccak512": "icicle_create_keccak_512", "sha3_256": "icicle_create_sha3_256",
           "sha3_512": "icicle_create_sha3_512", "blake2s": "icicle_create_blake2s", "blake3": "icicle_create_blake3"}
OUT = {"keccak256": 32, "keccak512": 64, "sha3_256": 32, "sha3_512": 64, "blake2s": 32, "blake3": 32}
DEFAULT_LABELS = ["domain_separator_label", "round_challenge_label", "commit_phase_label", "nonce_label"]

# name, field, extension, log n, queries, pow bits, stopping degree, log of the domain, tree hashers (leaves, compress), transcript hasher, labels,
# public state, seed (None: searched so that a query equals n)
CASES = [
    ("bb_scalar_keccak", "babybear", False, 5, 4, 0, 0, 5, ("keccak256", "keccak256"), "keccak256", DEFAULT_LABELS, b"", [1]),
    ("bb_ext_sha3_pow", "babybear", True, 5, 4, 6, 1, 5, ("sha3_256", "sha3_256"), "sha3_256", ["ds", "round", "commit", "nonce"], b"public \x00 state", [7, 0, 3, 1]),
    ("kb_scalar_blake2s_pow_bigdomain", "koalabear", False, 6, 5, 6, 3, 9, ("blake2s", "blake2s"), "blake2s", DEFAULT_LABELS, b"\x01\x02\x03", [12345]),
    ("kb_ext_blake3_keccak512_transcript", "koalabear", True, 5, 4, 0, 0, 5, ("blake3", "blake3"), "keccak512", DEFAULT_LABELS, b"", [2, 4, 6, 8]),
    ("bb_scalar_query_equals_n", "babybear", False, 5, 5, 0, 0, 6, ("blake2s", "blake2s"), "sha3_512", DEFAULT_LABELS, b"state", None),
    ("kb_scalar_keccak_blake3_transcript_pow", "koalabear", False, 5, 4, 6, 1, 5, ("keccak256", "keccak256"), "blake3", ["", "r", "", "n"], b"", [0]),
    ("bb_ext_log7_mixed", "babybear", True, 7, 4, 6, 3, 7, ("keccak256", "sha3_256"), "blake2s", DEFAULT_LABELS, b"", [0x77FFFFFF, 1, 2, 3]),
    ("kb_ext_keccak512_trees", "koalabear", True, 5, 4, 0, 1, 8, ("sha3_512", "keccak512"), "keccak256", DEFAULT_LABELS, b"x", [5, 0, 0, 0]),
]


class FriConfig(ctypes.Structure):
    _fields_ = [("stream", ctypes.c_void_p), ("folding_factor", ctypes.c_size_t), ("stopping_degree", ctypes.c_size_t), ("pow_bits", ctypes.c_size_t),
                ("nof_queries", ctypes.c_size_t), ("are_inputs_on_device", ctypes.c_bool), ("is_async", ctypes.c_bool), ("ext", ctypes.c_void_p)]


class Transcript(ctypes.Structure):
    _fields_ = [("hasher", ctypes.c_void_p)] + [(f"{n}{s}", t) for n in ("ds", "round", "commit", "nonce", "public") for s, t in (("", ctypes.c_char_p), ("_len", ctypes.c_size_t))] \
        + [("seed", ctypes.c_void_p)]


class InitDomainConfig(ctypes.Structure):
    _fields_ = [("stream", ctypes.c_void_p), ("is_async", ctypes.c_bool), ("ext", ctypes.c_void_p)]


def build(field, tmp):
    cxx = os.environ.get("ORACLE_CXX", "/opt/rocm/lib/llvm/bin/clang++")
    if not os.path.exists(cxx):
        cxx = "g++"
    objs = []
    for f in ("blake3", "blake3_dispatch", "blake3_portable"):
        objs.append(os.path.join(tmp, f"{f}.o"))
        subprocess.check_call(["gcc", "-O2", "-fPIC", "-c", *BLAKE3_FLAGS, os.path.join(REF, "backend/cpu/src/hash", f + ".c"), "-o", objs[-1]])
    so = os.path.join(tmp, f"libref_fri_{field}.so")
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-fPIC", "-shared", "-pthread", "-w", f"-I{REF}/include", f"-I{REF}/backend/cpu/include",
                           f"-I{os.path.join(ROOT, 'oracle', 'shim')}", f"-DFIELD_ID={FIELD_IDS[field]}", f"-DFIELD={field}", f"-DICICLE_FFI_PREFIX={field}", "-DNTT=ON",
                           "-DEXT_FIELD=ON", "-DFRI=ON", *[os.path.join(REF, s) for s in SOURCES], *objs, "-ldl", "-o", so])
    return so


def read_bytes(fn, handle, with_idx=False):
    n, idx = ctypes.c_size_t(), ctypes.c_uint64()
    p = fn(handle, ctypes.byref(n), ctypes.byref(idx)) if with_idx else fn(handle, ctypes.byref(n))
    return ctypes.string_at(p, n.value), idx.value


def find_seed(case, data):
    """the smallest seed for which the model draws a query equal to n"""
    name, field, ext, logn, nq, pow_bits, sd, _, (lh, ch), th, labels, public, _ = case
    F = fm.Field(field, ext)
    elems = [tuple(int(v) for v in row) for row in data.reshape(-1, F.words)]
    for seed in range(1, 2000):
        pr = fm.prove(field, ext, elems, th, tuple(s.encode() for s in labels), public, (seed,) + (0,) * (F.words - 1), lh, ch, sd, pow_bits, nq)
        if (1 << logn) in pr["queries"]:
            return [seed] + [0] * (F.words - 1)
    sys.exit("no seed found")


def run_case(lib, case, index):
    name, field, ext, logn, nq, pow_bits, sd, log_domain, (lh, ch), th, labels, public, seed = case
    p = fm.FIELDS[field][0]
    words, n = (4 if ext else 1), 1 << logn
    pre = f"{field}_extension" if ext else field
    data = np.random.default_rng(1000 + index).integers(0, p, size=n * words, dtype=np.uint32)
    data[0], data[1] = 0, p - 1
    if seed is None:
        seed = find_seed(case, data)
    for f in ("icicle_create_keccak_256", "icicle_create_keccak_512", "icicle_create_sha3_256", "icicle_create_sha3_512", "icicle_create_blake2s", "icicle_create_blake3",
              f"{pre}_icicle_initialize_fri_proof", "icicle_merkle_proof_get_leaf", "icicle_merkle_proof_get_root", "icicle_merkle_proof_get_path"):
        getattr(lib, f).restype = ctypes.c_void_p
    for f in HASHERS.values():
        getattr(lib, f).argtypes = [ctypes.c_uint64]
    rou = ctypes.c_uint32()
    assert getattr(lib, f"{field}_get_root_of_unity")(ctypes.c_uint64(1 << log_domain), ctypes.byref(rou)) == 0
    dcfg = InitDomainConfig(None, False, None)
    assert getattr(lib, f"{field}_ntt_init_domain")(ctypes.byref(rou), ctypes.byref(dcfg)) == 0
    hashers = [ctypes.c_void_p(getattr(lib, HASHERS[th])(0)), ctypes.c_void_p(getattr(lib, HASHERS[lh])(4 * words)), ctypes.c_void_p(getattr(lib, HASHERS[ch])(2 * OUT[ch]))]
    seed_arr = (ctypes.c_uint32 * words)(*seed)
    lab = [s.encode() for s in labels]
    tc = Transcript(hashers[0], lab[0], len(lab[0]), lab[1], len(lab[1]), lab[2], len(lab[2]), lab[3], len(lab[3]), public, len(public), ctypes.cast(seed_arr, ctypes.c_void_p))
    cfg = FriConfig(None, 2, sd, pow_bits, nq, False, False, None)
    proof = ctypes.c_void_p(getattr(lib, f"{pre}_icicle_initialize_fri_proof")())
    rc = getattr(lib, f"{pre}_fri_merkle_tree_prove")(ctypes.byref(cfg), ctypes.byref(tc), data.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(n), hashers[1], hashers[2],
                                                     ctypes.c_uint64(0), proof)
    assert rc == 0, (name, rc)
    ok = ctypes.c_bool(False)
    assert getattr(lib, f"{pre}_fri_merkle_tree_verify")(ctypes.byref(cfg), ctypes.byref(tc), proof, hashers[1], hashers[2], ctypes.byref(ok)) == 0 and ok.value, name
    nslots, nrounds, fsize, nonce, fptr = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_uint64(), ctypes.c_void_p()
    assert getattr(lib, f"{pre}_fri_proof_get_nof_queries")(proof, ctypes.byref(nslots)) == 0
    assert getattr(lib, f"{pre}_fri_proof_get_nof_rounds")(proof, ctypes.byref(nrounds)) == 0
    assert getattr(lib, f"{pre}_fri_proof_get_final_poly_size")(proof, ctypes.byref(fsize)) == 0
    assert getattr(lib, f"{pre}_fri_proof_get_final_poly")(proof, ctypes.byref(fptr)) == 0
    assert getattr(lib, f"{pre}_fri_proof_get_pow_nonce")(proof, ctypes.byref(nonce)) == 0
    final_poly = np.frombuffer(ctypes.string_at(fptr.value, 4 * words * fsize.value), dtype=np.uint32)
    slots = []
    for q in range(nslots.value):
        arr = (ctypes.c_void_p * nrounds.value)()
        assert getattr(lib, f"{pre}_fri_proof_get_round_proofs_for_query")(proof, ctypes.c_size_t(q), arr) == 0
        row = []
        for r in range(nrounds.value):
            h = ctypes.c_void_p(arr[r])
            leaf, idx = read_bytes(lib.icicle_merkle_proof_get_leaf, h, True)
            row.append({"leaf_idx": idx, "leaf": leaf.hex(), "root": read_bytes(lib.icicle_merkle_proof_get_root, h)[0].hex(),
                        "path": read_bytes(lib.icicle_merkle_proof_get_path, h)[0].hex()})
        slots.append(row)
    assert getattr(lib, f"{pre}_icicle_delete_fri_proof")(proof) == 0
    for h in hashers:
        lib.icicle_hasher_delete(h)
    assert getattr(lib, f"{field}_ntt_release_domain")() == 0
    return {"name": name, "field": field, "extension": ext, "log_n": logn, "nof_queries": nq, "pow_bits": pow_bits, "stopping_degree": sd, "log_domain": log_domain,
            "leaves_hash": lh, "compress_hash": ch, "transcript_hash": th, "labels": labels, "public_state": public.hex(), "seed": [int(v) for v in seed],
            "input": [int(v) for v in data], "final_poly": [int(v) for v in final_poly], "nonce": int(nonce.value), "slots": slots}


def main():
    if not os.path.isdir(REF):
        sys.exit(f"reference tree not found ({REF}): nothing minted")
    cases = []
    with tempfile.TemporaryDirectory() as tmp:
        for field in FIELD_IDS:
            lib = ctypes.CDLL(build(field, tmp))
            for i, case in enumerate(CASES):
                if case[1] == field:
                    cases.append((i, run_case(lib, case, i)))
                    print(case[0], "nonce", cases[-1][1]["nonce"])
            del lib
    doc = {"source": "reference CPU backend through its C ABI (tests/golden/mint_fri_vectors.py)", "cases": [c for _, c in sorted(cases, key=lambda t: t[0])]}
    out = os.path.join(HERE, "fri_vectors.json")
    with open(out, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print(f"{len(cases)} cases, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
