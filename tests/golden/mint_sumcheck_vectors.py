#!/usr/bin/env python3
"""Mint tests/golden/sumcheck_vectors.json: sumcheck proofs from the reference's CPU backend, driven through its own C ABI.

The method of mint_fri_vectors.py: the reference's sources are compiled where they lie, unmodified, into a temporary directory that
is deleted afterwards -- the recipe of oracle/build_ref.sh (device + field library against oracle/shim) with -DSUMCHECK=ON and the
program, symbol, hash and sumcheck sources, one library per field. Only data is recorded, per case: the polynomials, labels, seed,
claimed sum and a description of the program (tests/sumcheck_model.py Program), and from the reference the round polynomials and the
challenge vector. With --large: tests/golden/sumcheck_vectors_large.json, the cases of sumcheck_model.LARGE_CASES (2^20 and 2^21
elements), whose inputs come from sumcheck_model.large_inputs and are recorded by seed and sha256 only. User programs are built through the reference's symbol ABI from that description. Needs the reference tree
($ICICLE_REFERENCE_DIR, default /root/reference), gcc and a C++17 compiler; the tests read only the JSON.
"""
import ctypes
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import sumcheck_model as sm  # noqa: E402

REF = os.path.join(os.environ.get("ICICLE_REFERENCE_DIR", "/root/reference"), "icicle")
FIELD_IDS = {"babybear": (1001, ["-DEXT_FIELD=ON"]), "koalabear": (1004, ["-DEXT_FIELD=ON"]), "bn254": (1, []), "bls12_381": (2, [])}
BLAKE3_FLAGS = ["-DBLAKE3_NO_SSE2", "-DBLAKE3_NO_SSE41", "-DBLAKE3_NO_AVX2", "-DBLAKE3_NO_AVX512", "-DBLAKE3_USE_NEON=0"]
SOURCES = [
    "src/device_api.cpp", "src/runtime.cpp", "src/config_extension.cpp", "backend/cpu/src/cpu_device_api.cpp",
    "src/fields/ffi_extern.cpp", "src/program/program_c_api.cpp", "src/symbol/symbol_api.cpp",
    "src/hash/keccak.cpp", "src/hash/blake2s.cpp", "src/hash/blake3.cpp", "src/hash/hash_c_api.cpp",
    "backend/cpu/src/hash/cpu_keccak.cpp", "backend/cpu/src/hash/cpu_blake2s.cpp", "backend/cpu/src/hash/cpu_blake3.cpp",
    "src/sumcheck/sumcheck.cpp", "src/sumcheck/sumcheck_c_api.cpp", "backend/cpu/src/field/cpu_sumcheck.cpp",
]
HASHERS = {"keccak256": "icicle_create_keccak_256", "keccak512": "icicle_create_keccak_512", "sha3_256": "icicle_create_sha3_256",
           "sha3_512": "icicle_create_sha3_512", "blake2s": "icicle_create_blake2s", "blake3": "icicle_create_blake3"}
DEFAULT_LABELS = ["domain_separator_label", "round_poly_label", "round_challenge_label"]
EMPTY_LABELS = ["", "", ""]
LARGE_HASHER, LARGE_SEED, MODEL_CHECKED = "keccak256", 5, "bb_eq_l21"  # --large: transcript of every case of sm.LARGE_CASES

AB, EQ = sm.Program(3, predefined=sm.AB_MINUS_C), sm.Program(4, predefined=sm.EQ_X_AB_MINUS_C)
DEG1 = sm.Program(3, [["in", 0], ["in", 1], ["in", 2], ["add", 0, 1], ["sub", 3, 2]])  # x0 + x1 - x2
# t = x0 + 5 used twice, and a second constant: t t x1 - 7 t
SHARED = sm.Program(2, [["in", 0], ["in", 1], ["const", 5], ["add", 0, 2], ["mul", 3, 3], ["mul", 4, 1], ["const", 7], ["mul", 6, 3], ["sub", 5, 7]])
DEG6 = sm.Program(6, [["in", i] for i in range(6)] + [["mul", 0, 1], ["mul", 6, 2], ["mul", 7, 3], ["mul", 8, 4], ["mul", 9, 5]])

# name, field, program, L, transcript hasher, labels, seed, fill (None: random, with 0 and p - 1 among the values)
CASES = [
    ("bb_ab_l1_keccak256", "babybear", AB, 1, "keccak256", DEFAULT_LABELS, 1, None),
    ("bb_eq_l2_sha3", "babybear", EQ, 2, "sha3_256", DEFAULT_LABELS, 7, None),
    ("bb_eq_l3_blake2s", "babybear", EQ, 3, "blake2s", ["ds", "poly", "challenge"], 12345, None),
    ("bb_ab_l4_empty_labels", "babybear", AB, 4, "keccak256", EMPTY_LABELS, 0, None),
    ("bb_eq_l7_keccak512", "babybear", EQ, 7, "keccak512", DEFAULT_LABELS, 0x77FFFFFF, None),
    ("bb_deg1_l5_blake3", "babybear", DEG1, 5, "blake3", DEFAULT_LABELS, 3, None),
    ("bb_shared_l6_keccak256", "babybear", SHARED, 6, "keccak256", DEFAULT_LABELS, 9, None),
    ("bb_deg6_l4_sha3_512", "babybear", DEG6, 4, "sha3_512", DEFAULT_LABELS, 2, None),
    ("bb_eq_l5_all_p_minus_1", "babybear", EQ, 5, "keccak256", DEFAULT_LABELS, 1, "p-1"),
    ("bb_eq_l5_all_zero", "babybear", EQ, 5, "keccak256", DEFAULT_LABELS, 1, "zero"),
    ("kb_eq_l6_keccak256", "koalabear", EQ, 6, "keccak256", DEFAULT_LABELS, 5, None),
    ("kb_ab_l3_blake3", "koalabear", AB, 3, "blake3", ["", "r", ""], 0, None),
    ("kb_deg6_l3_sha3", "koalabear", DEG6, 3, "sha3_256", DEFAULT_LABELS, 11, None),
    ("bn254_ab_l1_keccak256", "bn254", AB, 1, "keccak256", DEFAULT_LABELS, 1, None),
    ("bn254_eq_l4_keccak512", "bn254", EQ, 4, "keccak512", DEFAULT_LABELS, (1 << 200) + 17, None),
    ("bn254_shared_l3_blake2s", "bn254", SHARED, 3, "blake2s", DEFAULT_LABELS, 4, None),
    ("bn254_deg6_l2_sha3", "bn254", DEG6, 2, "sha3_256", DEFAULT_LABELS, 8, None),
    ("bn254_eq_l3_all_p_minus_1", "bn254", EQ, 3, "keccak256", DEFAULT_LABELS, 1, "p-1"),
    ("bls12_381_eq_l5_sha3", "bls12_381", EQ, 5, "sha3_256", DEFAULT_LABELS, 6, None),
    ("bls12_381_ab_l2_empty_labels", "bls12_381", AB, 2, "keccak256", EMPTY_LABELS, 0, None),
    ("bls12_381_deg1_l3_keccak512", "bls12_381", DEG1, 3, "keccak512", DEFAULT_LABELS, 2, None),
    ("bls12_381_eq_l2_all_zero", "bls12_381", EQ, 2, "blake3", DEFAULT_LABELS, 1, "zero"),
]


class SumcheckConfig(ctypes.Structure):
    _fields_ = [("stream", ctypes.c_void_p), ("use_extension_field", ctypes.c_bool), ("batch", ctypes.c_uint64), ("are_inputs_on_device", ctypes.c_bool),
                ("is_async", ctypes.c_bool), ("ext", ctypes.c_void_p)]


class Transcript(ctypes.Structure):
    _fields_ = [("hasher", ctypes.c_void_p)] + [(f"{n}{s}", t) for n in ("ds", "poly", "challenge") for s, t in (("", ctypes.c_char_p), ("_len", ctypes.c_size_t))] \
        + [("little_endian", ctypes.c_bool), ("seed", ctypes.c_void_p)]


def build(field, tmp):
    cxx = os.environ.get("ORACLE_CXX", "/opt/rocm/lib/llvm/bin/clang++")
    if not os.path.exists(cxx):
        cxx = "g++"
    objs = []
    for f in ("blake3", "blake3_dispatch", "blake3_portable"):
        objs.append(os.path.join(tmp, f"{f}.o"))
        if not os.path.exists(objs[-1]):
            subprocess.check_call(["gcc", "-O2", "-fPIC", "-c", *BLAKE3_FLAGS, os.path.join(REF, "backend/cpu/src/hash", f + ".c"), "-o", objs[-1]])
    so = os.path.join(tmp, f"libref_sumcheck_{field}.so")
    fid, extra = FIELD_IDS[field]
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-fPIC", "-shared", "-pthread", "-w", f"-I{REF}/include", f"-I{REF}/backend/cpu/include",
                           f"-I{os.path.join(ROOT, 'oracle', 'shim')}", f"-DFIELD_ID={fid}", f"-DFIELD={field}", f"-DICICLE_FFI_PREFIX={field}", "-DNTT=ON",
                           "-DSUMCHECK=ON", *extra, *[os.path.join(REF, s) for s in SOURCES], *objs, "-ldl", "-o", so])
    return so


def words_of(field, values):
    w = sm.FIELDS[field][1]
    return np.array([(int(v) >> (32 * i)) & 0xFFFFFFFF for v in values for i in range(w)], dtype=np.uint32)


def ints_of(field, words):
    w = sm.FIELDS[field][1]
    return [sum(int(words[i * w + j]) << (32 * j) for j in range(w)) for i in range(len(words) // w)]


def reference_program(lib, field, program):
    if program.predefined is not None:
        return ctypes.c_void_p(getattr(lib, f"{field}_create_predefined_returning_value_program")(program.predefined))
    handles = []
    for n in program.nodes:
        if n[0] == "in":
            handles.append(ctypes.c_void_p(getattr(lib, f"{field}_create_input_symbol")(n[1])))
        elif n[0] == "const":
            c = words_of(field, [n[1]])
            handles.append(ctypes.c_void_p(getattr(lib, f"{field}_create_scalar_symbol")(c.ctypes.data_as(ctypes.c_void_p))))
        else:
            out = ctypes.c_void_p()
            fn = {"add": "add_symbols", "sub": "sub_symbols", "mul": "multiply_symbols"}[n[0]]
            assert getattr(lib, f"{field}_{fn}")(handles[n[1]], handles[n[2]], ctypes.byref(out)) == 0
            handles.append(out)
    params = (ctypes.c_void_p * (program.nof_inputs + 1))(*[handles[i].value for i in range(program.nof_inputs)], handles[-1].value)
    prog = ctypes.c_void_p()
    assert getattr(lib, f"{field}_generate_returning_value_program")(params, program.nof_inputs + 1, ctypes.byref(prog)) == 0
    return prog


def reference_proof(lib, name, field, program, arrays, n, claimed, hasher, labels, seed):
    """(round polynomials, challenge vector) as ints from the reference's prover, which its own verifier accepts; arrays: flat uint32 words"""
    w = sm.FIELDS[field][1]
    m, L = program.nof_inputs, n.bit_length() - 1
    for f in list(HASHERS.values()) + [f"{field}_{s}" for s in ("sumcheck_create", "sumcheck_get_proof", "sumcheck_proof_get_round_poly_at",
                                                                "create_predefined_returning_value_program", "create_input_symbol", "create_scalar_symbol")]:
        getattr(lib, f).restype = ctypes.c_void_p
    for f in HASHERS.values():
        getattr(lib, f).argtypes = [ctypes.c_uint64]
    th = ctypes.c_void_p(getattr(lib, HASHERS[hasher])(0))
    prog = reference_program(lib, field, program)
    table = (ctypes.c_void_p * m)(*[a.ctypes.data for a in arrays])
    seed_arr, claimed_arr = words_of(field, [seed]), words_of(field, [claimed])
    lab = [s.encode() for s in labels]
    tc = Transcript(th, lab[0], len(lab[0]), lab[1], len(lab[1]), lab[2], len(lab[2]), True, seed_arr.ctypes.data_as(ctypes.c_void_p))
    cfg = SumcheckConfig(None, False, 1, False, False, None)
    sc = ctypes.c_void_p(getattr(lib, f"{field}_sumcheck_create")())
    proof = ctypes.c_void_p(getattr(lib, f"{field}_sumcheck_get_proof")(sc, table, ctypes.c_uint64(n), ctypes.c_uint64(m), claimed_arr.ctypes.data_as(ctypes.c_void_p), prog,
                                                                      ctypes.byref(tc), ctypes.byref(cfg)))
    assert proof.value, name
    ok = ctypes.c_bool(False)
    assert getattr(lib, f"{field}_sumcheck_verify")(sc, proof, claimed_arr.ctypes.data_as(ctypes.c_void_p), ctypes.byref(tc), ctypes.byref(ok)) == 0 and ok.value, name
    size, count = ctypes.c_uint64(), ctypes.c_uint64()
    assert getattr(lib, f"{field}_sumcheck_proof_get_poly_sizes")(proof, ctypes.byref(size), ctypes.byref(count)) == 0
    assert (size.value, count.value) == (program.degree() + 1, L), (name, size.value, count.value)
    rps = []
    for r in range(L):
        ptr = getattr(lib, f"{field}_sumcheck_proof_get_round_poly_at")(proof, ctypes.c_uint64(r))
        rps.append(ints_of(field, np.frombuffer(ctypes.string_at(ptr, 4 * w * size.value), dtype=np.uint32)))
    csize = ctypes.c_size_t()
    assert getattr(lib, f"{field}_sumcheck_get_challenge_size")(sc, ctypes.byref(csize)) == 0 and csize.value == L
    cvec = np.zeros(L * w, dtype=np.uint32)
    assert getattr(lib, f"{field}_sumcheck_get_challenge_vector")(sc, cvec.ctypes.data_as(ctypes.c_void_p), ctypes.byref(csize)) == 0
    assert getattr(lib, f"{field}_sumcheck_proof_delete")(proof) == 0 and getattr(lib, f"{field}_sumcheck_delete")(sc) == 0
    lib.delete_program(prog)
    lib.icicle_hasher_delete(th)
    return rps, ints_of(field, cvec)


def run_case(lib, case, index):
    name, field, program, L, hasher, labels, seed, fill = case
    p, w = sm.FIELDS[field]
    n, m = 1 << L, program.nof_inputs
    rng = np.random.default_rng(2000 + index)
    if fill is None:
        polys = [[int.from_bytes(rng.bytes(40), "little") % p for _ in range(n)] for _ in range(m)]
        polys[0][0], polys[-1][-1] = 0, p - 1
    else:
        polys = [[p - 1 if fill == "p-1" else 0] * n for _ in range(m)]
    claimed = sm.claimed_sum(field, polys, program)
    rps, challenges = reference_proof(lib, name, field, program, [words_of(field, t) for t in polys], n, claimed, hasher, labels, seed)
    hexes = lambda row: [f"{v:x}" for v in row]
    return {"name": name, "field": field, "log_n": L, "transcript_hash": hasher, "labels": labels, "seed": f"{seed:x}", "claimed_sum": f"{claimed:x}",
            "program": program.description(), "degree": program.degree(), "polys": [hexes(t) for t in polys], "round_polys": [hexes(r) for r in rps],
            "challenges": hexes(challenges)}


def run_large_case(lib, case):
    """A case of sm.LARGE_CASES: the inputs come from sm.large_inputs and are recorded by their sha256 only."""
    name, field, program, L, input_seed, _ = case
    p, w = sm.FIELDS[field]
    n = 1 << L
    arrays = sm.large_inputs(field, program.nof_inputs, n, input_seed)
    polys = [sm.ints_of_array(a, w) for a in arrays]
    claimed = sm.claimed_sum(field, polys, program)
    rps, challenges = reference_proof(lib, name, field, program, [np.ascontiguousarray(a).reshape(-1) for a in arrays], n, claimed, LARGE_HASHER, sm.LARGE_LABELS,
                                      LARGE_SEED)
    if name == MODEL_CHECKED:  # the model once at a large size: it and the reference agree, or nothing is written
        t = time.time()
        want = sm.prove(field, polys, claimed, program, LARGE_HASHER, tuple(s.encode() for s in sm.LARGE_LABELS), LARGE_SEED)
        assert want == {"round_polys": rps, "challenges": challenges}, f"{name}: the model and the reference disagree"
        print(f"{name}: the model agrees ({time.time() - t:.1f} s)")
    hexes = lambda row: [f"{v:x}" for v in row]
    return {"name": name, "field": field, "log_n": L, "transcript_hash": LARGE_HASHER, "labels": sm.LARGE_LABELS, "seed": f"{LARGE_SEED:x}", "input_seed": input_seed,
            "input_sha256": sm.sha256_of(arrays), "claimed_sum": f"{claimed:x}", "program": program.description(), "degree": program.degree(),
            "round_polys": [hexes(r) for r in rps], "challenges": hexes(challenges)}


def mint_large():
    cases, start = [], time.time()
    with tempfile.TemporaryDirectory() as tmp:
        for field in FIELD_IDS:
            todo = [c for c in sm.LARGE_CASES if c[1] == field]
            if not todo:
                continue
            lib = ctypes.CDLL(build(field, tmp))
            for case in todo:
                t = time.time()
                cases.append(run_large_case(lib, case))
                print(f"{case[0]} ok ({time.time() - t:.1f} s)")
            del lib
    order = [c[0] for c in sm.LARGE_CASES]
    doc = {"source": "reference CPU backend through its C ABI (tests/golden/mint_sumcheck_vectors.py --large); inputs: tests/sumcheck_model.py large_inputs",
           "cases": sorted(cases, key=lambda c: order.index(c["name"]))}
    out = os.path.join(HERE, "sumcheck_vectors_large.json")
    with open(out, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print(f"{len(cases)} large cases, {os.path.getsize(out)} bytes, {time.time() - start:.1f} s with the builds")


def main():
    if not os.path.isdir(REF):
        sys.exit(f"reference tree not found ({REF}): nothing minted")
    if "--large" in sys.argv[1:]:
        return mint_large()
    cases = []
    with tempfile.TemporaryDirectory() as tmp:
        for field in FIELD_IDS:
            lib = ctypes.CDLL(build(field, tmp))
            for i, case in enumerate(CASES):
                if case[1] == field:
                    cases.append((i, run_case(lib, case, i)))
                    print(case[0], "ok")
            del lib
    doc = {"source": "reference CPU backend through its C ABI (tests/golden/mint_sumcheck_vectors.py)", "cases": [c for _, c in sorted(cases, key=lambda t: t[0])]}
    out = os.path.join(HERE, "sumcheck_vectors.json")
    with open(out, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print(f"{len(cases)} cases, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
