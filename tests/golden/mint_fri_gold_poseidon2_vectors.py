#!/usr/bin/env python3
"""Mint tests/golden/fri_vectors_gold_poseidon2.json: FRI proofs over Goldilocks (scalar and quadratic extension) whose Merkle trees
hash with Poseidon2 over Goldilocks, from the reference's CPU backend, driven through its own C ABI.

The recipe of mint_fri_vectors_wide.py, whose defines, structs and proof reader are imported, with the three Poseidon2 sources added
to the build and the tree hashers made by goldilocks_create_poseidon2_hasher(t, tag, input_size). The transcript hasher stays
Keccak-256. Only data is recorded, per case what the other FRI fixtures record, with the two tree hashers as (t, tag, input_size).
Needs the reference tree ($ICICLE_REFERENCE_DIR, default /root/reference), gcc and a C++17 compiler; the tests read only the JSON.
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
import mint_fri_vectors as base  # noqa: E402
import mint_fri_vectors_wide as wide  # noqa: E402

REF = base.REF
FIELD = "goldilocks"
POSEIDON2_SOURCES = ["src/hash/poseidon2.cpp", "src/hash/poseidon2_c_api.cpp", "backend/cpu/src/hash/cpu_poseidon2.cpp"]
DEFAULT_LABELS = base.DEFAULT_LABELS

# name, extension, log n, queries, pow bits, stopping degree, log of the domain, leaves hasher and compress hasher as (t, tag, input_size),
# labels, public state, seed (coefficients)
CASES = [
    ("gl_t2_t2", False, 5, 4, 0, 0, 5, (2, None, 1), (2, None, 2), DEFAULT_LABELS, b"", [1]),
    ("glx_t3_t2", True, 5, 4, 0, 0, 5, (3, None, 2), (2, None, 0), DEFAULT_LABELS, b"x", [0, 5]),
    ("gl_t8_t3", False, 5, 4, 0, 0, 5, (8, None, 1), (3, None, 2), ["ds", "round", "commit", "nonce"], b"public \x00 state", [0xFFFFFFFF00000000]),
    ("gl_t2_t3_tagged_pow_bigdomain", False, 5, 4, 6, 1, 8, (2, None, 1), (3, 7, 0), DEFAULT_LABELS, b"\x01\x02\x03", [3]),
]


def build(tmp):
    cxx = os.environ.get("ORACLE_CXX", "/opt/rocm/lib/llvm/bin/clang++")
    if not os.path.exists(cxx):
        cxx = "g++"
    objs = []
    for f in ("blake3", "blake3_dispatch", "blake3_portable"):
        objs.append(os.path.join(tmp, f"{f}.o"))
        subprocess.check_call(["gcc", "-O2", "-fPIC", "-c", *base.BLAKE3_FLAGS, os.path.join(REF, "backend/cpu/src/hash", f + ".c"), "-o", objs[-1]])
    so = os.path.join(tmp, "libref_fri_goldilocks_poseidon2.so")
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-fPIC", "-shared", "-pthread", "-w", f"-I{REF}/include", f"-I{REF}/backend/cpu/include",
                           f"-I{os.path.join(ROOT, 'oracle', 'shim')}", *wide.DEFINES[FIELD], f"-DICICLE_FFI_PREFIX={FIELD}", "-DNTT=ON", "-DFRI=ON", "-DPOSEIDON2=ON",
                           *[os.path.join(REF, s) for s in base.SOURCES + POSEIDON2_SOURCES], *objs, "-ldl", "-o", so])
    return so


def poseidon2(lib, spec):
    t, tag, input_size = spec
    tag_buf = (ctypes.c_uint64 * 1)(tag or 0)
    h = ctypes.c_void_p(lib.goldilocks_create_poseidon2_hasher(t, ctypes.cast(tag_buf, ctypes.c_void_p) if tag is not None else None, input_size))
    assert h and lib.icicle_hasher_output_size(h) == 8
    return h


def run_case(lib, case, index):
    name, ext, logn, nq, pow_bits, sd, log_domain, lh, ch, labels, public, seed = case
    F = fw.Field(FIELD, ext)
    n, pre = 1 << logn, fw.prefix(FIELD, ext)
    rng = random.Random(5000 + index)
    elems = [tuple(rng.randrange(F.p) for _ in range(F.coeffs)) for _ in range(n)]
    elems[0], elems[1] = (0,) * F.coeffs, (F.p - 1,) * F.coeffs
    if ext:
        elems[2], elems[3] = (F.p - 1, 0), (0, F.p - 1)
    data = ctypes.create_string_buffer(F.raw(elems), n * F.bytes)
    for f in ["icicle_create_keccak_256", "goldilocks_create_poseidon2_hasher", f"{pre}_icicle_initialize_fri_proof", "icicle_merkle_proof_get_leaf",
              "icicle_merkle_proof_get_root", "icicle_merkle_proof_get_path"]:
        getattr(lib, f).restype = ctypes.c_void_p
    lib.icicle_create_keccak_256.argtypes = [ctypes.c_uint64]
    lib.goldilocks_create_poseidon2_hasher.argtypes = [ctypes.c_uint, ctypes.c_void_p, ctypes.c_uint]
    lib.icicle_hasher_output_size.argtypes = [ctypes.c_void_p]
    lib.icicle_hasher_output_size.restype = ctypes.c_uint64
    rou = (ctypes.c_uint32 * 8)()
    assert lib.goldilocks_get_root_of_unity(ctypes.c_uint64(1 << log_domain), rou) == 0
    dcfg = base.InitDomainConfig(None, False, None)
    assert lib.goldilocks_ntt_init_domain(rou, ctypes.byref(dcfg)) == 0
    hashers = [ctypes.c_void_p(lib.icicle_create_keccak_256(0)), poseidon2(lib, lh), poseidon2(lib, ch)]
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
    assert lib.goldilocks_ntt_release_domain() == 0
    spec = lambda s: {"t": s[0], "tag": s[1], "input_size": s[2]}
    return {"name": name, "field": FIELD, "extension": ext, "log_n": logn, "nof_queries": nq, "pow_bits": pow_bits, "stopping_degree": sd, "log_domain": log_domain,
            "leaves_hash": spec(lh), "compress_hash": spec(ch), "transcript_hash": "keccak256", "labels": labels, "public_state": public.hex(), "seed": seed_raw.hex(),
            "input": data.raw.hex(), "final_poly": final_poly.hex(), "nonce": int(nonce.value), "slots": slots}


def main():
    if not os.path.isdir(REF):
        sys.exit(f"reference tree not found ({REF}): nothing minted")
    with tempfile.TemporaryDirectory() as tmp:
        lib = ctypes.CDLL(build(tmp))
        cases = []
        for i, case in enumerate(CASES):
            cases.append(run_case(lib, case, i))
            print(case[0], "nonce", cases[-1]["nonce"], flush=True)
        del lib
    doc = {"source": "reference CPU backend through its C ABI (tests/golden/mint_fri_gold_poseidon2_vectors.py)", "cases": cases}
    out = os.path.join(HERE, "fri_vectors_gold_poseidon2.json")
    with open(out, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print(f"{len(cases)} cases, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
