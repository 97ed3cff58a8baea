#!/usr/bin/env python3
"""Mint tests/golden/fri_vectors_wide.json: FRI proofs over Goldilocks (scalar and quadratic extension), stark252 and the scalar
fields of BN254, BLS12-381 and BLS12-377 from the reference's CPU backend, driven through its own C ABI.

The recipe of mint_fri_vectors.py with other field defines: the reference's sources are compiled where they lie, unmodified, into
a temporary directory that is deleted afterwards, one library per field (a curve's scalar field needs the curve's defines next to
the field's; only Goldilocks is built with its extension). Only data is recorded, per case: the input, labels, seed and
configuration, and from the proof every slot's leaf index, leaf, root and path, the final polynomial and the nonce -- elements as
the hex of their bytes. Needs the reference tree ($ICICLE_REFERENCE_DIR, default /root/reference), gcc and a C++17 compiler; the
tests read only the JSON.
"""
import ctypes
import json
import os
import random
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from tests import fri_model_wide as fw  # noqa: E402
import mint_fri_vectors as base  # noqa: E402  (sources, hashers, structs and the proof reader of the 31-bit recipe)

REF = base.REF
# field -> the defines that select it
DEFINES = {
    "goldilocks": ["-DFIELD_ID=1005", "-DFIELD=goldilocks", "-DEXT_FIELD=ON"],
    "stark252": ["-DFIELD_ID=1002", "-DFIELD=stark252"],
    "bn254": ["-DFIELD_ID=1", "-DFIELD=bn254", "-DCURVE_ID=1", "-DCURVE=bn254"],
    "bls12_381": ["-DFIELD_ID=2", "-DFIELD=bls12_381", "-DCURVE_ID=2", "-DCURVE=bls12_381"],
    "bls12_377": ["-DFIELD_ID=3", "-DFIELD=bls12_377", "-DCURVE_ID=3", "-DCURVE=bls12_377"],
}
DEFAULT_LABELS = base.DEFAULT_LABELS

# name, field, extension, log n, queries, pow bits, stopping degree, log of the domain, tree hashers (leaves, compress), transcript hasher, labels,
# public state, seed (coefficients)
CASES = [
    ("gl_keccak", "goldilocks", False, 5, 4, 0, 0, 5, ("keccak256", "keccak256"), "keccak256", DEFAULT_LABELS, b"", [1]),
    ("glx_sha3_pow", "goldilocks", True, 5, 4, 6, 1, 5, ("sha3_256", "sha3_256"), "sha3_256", ["ds", "round", "commit", "nonce"], b"public \x00 state", [7, 0]),
    ("gl_blake2s_pow_bigdomain", "goldilocks", False, 6, 4, 6, 1, 9, ("blake2s", "blake2s"), "blake2s", DEFAULT_LABELS, b"\x01\x02\x03", [0xFFFFFFFF00000000]),
    ("glx_keccak512_trees_bigdomain", "goldilocks", True, 5, 4, 0, 0, 8, ("sha3_512", "keccak512"), "keccak256", DEFAULT_LABELS, b"x", [0, 5]),
    ("stark252_blake3_keccak512_transcript", "stark252", False, 5, 4, 0, 0, 5, ("blake3", "blake3"), "keccak512", DEFAULT_LABELS, b"", [2]),
    ("bn254_keccak_sha3_512_transcript_pow", "bn254", False, 5, 4, 6, 1, 5, ("keccak256", "keccak256"), "sha3_512", DEFAULT_LABELS, b"state", [12345]),
    ("bls12_381_blake2s_bigdomain", "bls12_381", False, 5, 4, 0, 0, 6, ("blake2s", "blake2s"), "blake2s", DEFAULT_LABELS, b"", [3]),
    ("bls12_377_mixed_trees_blake3_transcript_pow", "bls12_377", False, 5, 4, 6, 1, 5, ("keccak256", "sha3_256"), "blake3", ["", "r", "", "n"], b"", [1 << 200]),
]


def build(field, tmp):
    cxx = os.environ.get("ORACLE_CXX", "/opt/rocm/lib/llvm/bin/clang++")
    if not os.path.exists(cxx):
        cxx = "g++"
    objs = []
    for f in ("blake3", "blake3_dispatch", "blake3_portable"):
        objs.append(os.path.join(tmp, f"{f}.o"))
        if not os.path.exists(objs[-1]):
            subprocess.check_call(["gcc", "-O2", "-fPIC", "-c", *base.BLAKE3_FLAGS, os.path.join(REF, "backend/cpu/src/hash", f + ".c"), "-o", objs[-1]])
    so = os.path.join(tmp, f"libref_fri_{field}.so")
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-fPIC", "-shared", "-pthread", "-w", f"-I{REF}/include", f"-I{REF}/backend/cpu/include",
                           f"-I{os.path.join(ROOT, 'oracle', 'shim')}", *DEFINES[field], f"-DICICLE_FFI_PREFIX={field}", "-DNTT=ON", "-DFRI=ON",
                           *[os.path.join(REF, s) for s in base.SOURCES], *objs, "-ldl", "-o", so])
    return so


def run_case(lib, case, index):
    name, field, ext, logn, nq, pow_bits, sd, log_domain, (lh, ch), th, labels, public, seed = case
    F = fw.Field(field, ext)
    n, pre = 1 << logn, fw.prefix(field, ext)
    rng = random.Random(2000 + index)
    elems = [tuple(rng.randrange(F.p) for _ in range(F.coeffs)) for _ in range(n)]
    elems[0], elems[1] = (0,) * F.coeffs, (F.p - 1,) * F.coeffs
    if ext:
        elems[2], elems[3] = (F.p - 1, 0), (0, F.p - 1)
    data = ctypes.create_string_buffer(F.raw(elems), n * F.bytes)
    for f in list(base.HASHERS.values()) + [f"{pre}_icicle_initialize_fri_proof", "icicle_merkle_proof_get_leaf", "icicle_merkle_proof_get_root", "icicle_merkle_proof_get_path"]:
        getattr(lib, f).restype = ctypes.c_void_p
    for f in base.HASHERS.values():
        getattr(lib, f).argtypes = [ctypes.c_uint64]
    rou = (ctypes.c_uint32 * 8)()
    assert getattr(lib, f"{field}_get_root_of_unity")(ctypes.c_uint64(1 << log_domain), rou) == 0
    dcfg = base.InitDomainConfig(None, False, None)
    assert getattr(lib, f"{field}_ntt_init_domain")(rou, ctypes.byref(dcfg)) == 0
    hashers = [ctypes.c_void_p(getattr(lib, base.HASHERS[th])(0)), ctypes.c_void_p(getattr(lib, base.HASHERS[lh])(F.bytes)),
               ctypes.c_void_p(getattr(lib, base.HASHERS[ch])(2 * base.OUT[ch]))]
    seed_raw = F.to_bytes(tuple(seed))
    seed_buf = ctypes.create_string_buffer(seed_raw, len(seed_raw))
    lab = [s.encode() for s in labels]
    tc = base.Transcript(hashers[0], lab[0], len(lab[0]), lab[1], len(lab[1]), lab[2], len(lab[2]), lab[3], len(lab[3]), public, len(public), ctypes.cast(seed_buf, ctypes.c_void_p))
    cfg = base.FriConfig(None, 2, sd, pow_bits, nq, False, False, None)
    proof = ctypes.c_void_p(getattr(lib, f"{pre}_icicle_initialize_fri_proof")())
    rc = getattr(lib, f"{pre}_fri_merkle_tree_prove")(ctypes.byref(cfg), ctypes.byref(tc), ctypes.cast(data, ctypes.c_void_p), ctypes.c_size_t(n), hashers[1], hashers[2],
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
    final_poly = ctypes.string_at(fptr.value, F.bytes * fsize.value)
    slots = []
    for q in range(nslots.value):
        arr = (ctypes.c_void_p * nrounds.value)()
        assert getattr(lib, f"{pre}_fri_proof_get_round_proofs_for_query")(proof, ctypes.c_size_t(q), arr) == 0
        row = []
        for r in range(nrounds.value):
            h = ctypes.c_void_p(arr[r])
            leaf, idx = base.read_bytes(lib.icicle_merkle_proof_get_leaf, h, True)
            row.append({"leaf_idx": idx, "leaf": leaf.hex(), "root": base.read_bytes(lib.icicle_merkle_proof_get_root, h)[0].hex(),
                        "path": base.read_bytes(lib.icicle_merkle_proof_get_path, h)[0].hex()})
        slots.append(row)
    assert getattr(lib, f"{pre}_icicle_delete_fri_proof")(proof) == 0
    for h in hashers:
        lib.icicle_hasher_delete(h)
    assert getattr(lib, f"{field}_ntt_release_domain")() == 0
    return {"name": name, "field": field, "extension": ext, "log_n": logn, "nof_queries": nq, "pow_bits": pow_bits, "stopping_degree": sd, "log_domain": log_domain,
            "leaves_hash": lh, "compress_hash": ch, "transcript_hash": th, "labels": labels, "public_state": public.hex(), "seed": seed_raw.hex(),
            "input": data.raw.hex(), "final_poly": final_poly.hex(), "nonce": int(nonce.value), "slots": slots}


def main():
    if not os.path.isdir(REF):
        sys.exit(f"reference tree not found ({REF}): nothing minted")
    cases = []
    with tempfile.TemporaryDirectory() as tmp:
        for field in DEFINES:
            lib = ctypes.CDLL(build(field, tmp))
            for i, case in enumerate(CASES):
                if case[1] == field:
                    cases.append((i, run_case(lib, case, i)))
                    print(case[0], "nonce", cases[-1][1]["nonce"], flush=True)
            del lib
    doc = {"source": "reference CPU backend through its C ABI (tests/golden/mint_fri_vectors_wide.py)", "cases": [c for _, c in sorted(cases, key=lambda t: t[0])]}
    out = os.path.join(HERE, "fri_vectors_wide.json")
    with open(out, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print(f"{len(cases)} cases, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
