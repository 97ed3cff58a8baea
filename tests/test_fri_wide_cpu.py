"""CPU: FRI over the wide fields without a GPU -- the Python model (tests/fri_model_wide.py) against every fixture of the reference
(tests/golden/fri_vectors_wide.json) byte for byte, and the host-compilable code of the device path (F(digest) of
icicle_amd/csrc/fri_plan.h, the fold arithmetic of icicle_amd/csrc/fri_fold_wide.hpp, through tests/fri_wide_host_harness.cpp built
with g++ plainly and with -fsanitize=address,undefined as a program of its own) against Python integers, and the C ABI's surface of
the six new prefixes."""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest

from tests import blake_model as bm
from tests import fri_model_wide as fw

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INVALID_POINTER, INVALID_ARGUMENT = 3, 11
PREFIXES = ["goldilocks", "goldilocks_extension", "stark252", "bn254", "bls12_381", "bls12_377"]
CASES = fw.load_fixtures()
IDS = [c["name"] for c in CASES]


# ---- the model against the reference's proofs ----------------------------------------------------------------------------------------
def test_fixtures_cover_what_they_should():
    assert {(c["field"], c["extension"]) for c in CASES} == set(fw.KINDS)
    assert {c["leaves_hash"] for c in CASES} | {c["compress_hash"] for c in CASES} == {"keccak256", "keccak512", "sha3_256", "sha3_512", "blake2s", "blake3"}
    assert any(bm.OUT_SIZE[c["transcript_hash"]] == 64 for c in CASES)
    assert {c["pow_bits"] != 0 for c in CASES} == {False, True} and {c["stopping_degree"] for c in CASES} == {0, 1}
    assert any(c["log_domain"] > c["log_n"] for c in CASES)
    assert all(5 <= c["log_n"] <= 6 and c["nof_queries"] in (4, 5) for c in CASES)
    for c in CASES:
        F, elems = fw.case_field(c), fw.case_elements(c)
        assert len(elems) == 1 << c["log_n"] and (0,) * F.coeffs in elems and (F.p - 1,) * F.coeffs in elems
        assert all(v < F.p for e in elems for v in e)
    assert os.path.getsize(fw.FIXTURE) <= 212089  # no larger than tests/golden/fri_vectors.json


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_model_equals_the_reference(case):
    F = fw.case_field(case)
    got = fw.prove(F, fw.case_elements(case), *fw.case_protocol(case))
    want = fw.case_proof(case)
    assert got["final_poly"] == want["final_poly"]
    assert got["nonce"] == want["nonce"]
    assert len(got["slots"]) == len(want["slots"]) == 2 * case["nof_queries"]
    for q, (g, w) in enumerate(zip(got["slots"], want["slots"])):
        assert g == w, f"slot {q}"
    assert fw.verify(F, want, *fw.case_protocol(case))


def flip(b: bytes) -> bytes:
    return bytes([b[0] ^ 1]) + b[1:]


def changed_proofs(case):
    """(what, proof) for one bit flipped in a leaf, a root, the final polynomial and the nonce"""
    F = fw.case_field(case)
    for what in ("leaf", "root", "final_poly", "nonce"):
        pr = fw.case_proof(case)
        if what == "final_poly":
            pr["final_poly"][0] = F.from_bytes(flip(F.to_bytes(pr["final_poly"][0])))
        elif what == "nonce":
            pr["nonce"] ^= 1
        else:
            idx, leaf, root, path = pr["slots"][3][1]
            pr["slots"][3][1] = (idx, flip(leaf), root, path) if what == "leaf" else (idx, leaf, flip(root), path)
        yield what, pr


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_model_verifier_rejects_a_changed_proof(case):
    F = fw.case_field(case)
    for what, pr in changed_proofs(case):
        if what == "nonce" and not case["pow_bits"]:
            continue  # without a proof of work the nonce is not part of the statement
        assert not fw.verify(F, pr, *fw.case_protocol(case)), what


# ---- fri_plan.h and fri_fold_wide.hpp on the host -------------------------------------------------------------------------------------
def build_harness(name, flags):
    exe = os.path.join(HERE, "_build", name)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    src = os.path.join(HERE, "fri_wide_host_harness.cpp")
    deps = [src] + [os.path.join(ROOT, "icicle_amd", "csrc", f) for f in ("fri_plan.h", "fri_fold_wide.hpp", "bigfield.hpp", "goldfield.hpp", "field_consts.h")]
    if not os.path.exists(exe) or max(os.path.getmtime(d) for d in deps) > os.path.getmtime(exe):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-DBIGFIELD_BOUNDS", *flags, src, "-o", exe])
    return exe


def directed(F):
    """scalars of the base field at which the arithmetic changes its path"""
    p = F.p
    return [0, 1, p - 1, (p + 1) // 2, (p - 1) // 2, 2, p - 2]


def fold_cases(F, rng):
    """(lo, hi, tw, alpha): the directed operands crossed where it is cheap, lo == hi, lo == -hi, alpha = 0 and p - 1, and random ones"""
    p, c = F.p, F.coeffs
    d = directed(F)
    rand = lambda: tuple(rng.randrange(p) for _ in range(c))
    elems = [tuple([v] * c) for v in d]
    if c == 2:
        elems += [(v, 0) for v in d[1:4]] + [(0, v) for v in d[1:4]]  # one coefficient zero
    out = []
    for lo in elems:
        for hi in elems:
            out.append((lo, hi, rng.choice(d[1:]), rng.choice(elems)))
    for a in elems + [rand(), rand()]:
        x = rand()
        out.append((x, x, rng.randrange(p), a))                          # lo == hi: the odd part vanishes
        out.append((x, F.sub((0,) * c, x), rng.randrange(p), a))         # lo == -hi: the even part vanishes
        out.append((rand(), rand(), rng.randrange(p), a))
    for tw in d:
        out.append((rand(), rand(), tw, rand()))
    for _ in range(40):
        out.append((rand(), rand(), rng.randrange(p), rand()))
    return out


def harness_script():
    """(commands, expected answers) from Python integers"""
    rng = random.Random(11)
    cmds, want = [], []
    for field, ext in fw.KINDS:
        F = fw.Field(field, ext)
        kind = fw.prefix(field, ext)
        pb = F.p.to_bytes(F.coeff_bytes, "little")
        digests = [bytes(size) for size in (32, 64)] + [b"\xff" * size for size in (32, 64)]
        digests += [pb + bytes(32 - len(pb)), (F.p - 1).to_bytes(32, "little"), (F.p + 1).to_bytes(32, "little"), (2 * F.p).to_bytes(64, "little")]
        digests += [bytes(rng.randrange(256) for _ in range(size)) for size in (32, 64) for _ in range(6)]
        if ext:
            digests += [pb + pb + bytes(16), (F.p - 1).to_bytes(8, "little") + b"\xff" * 24]
        for dg in digests:
            cmds.append(f"digest {kind} {dg.hex()}")
            want.append(F.to_bytes(F.from_digest(dg)).hex())
        for lo, hi, tw, alpha in fold_cases(F, rng):
            cmds.append(f"fold {kind} {F.to_bytes(lo).hex()} {F.to_bytes(hi).hex()} {tw.to_bytes(F.coeff_bytes, 'little').hex()} {F.to_bytes(alpha).hex()}")
            want.append(F.to_bytes(F.fold1(lo, hi, alpha, tw)).hex())
    return cmds, want


@pytest.fixture(scope="module")
def script():
    return harness_script()


def run_harness(exe, cmds):
    r = subprocess.run([exe], input="\n".join(cmds) + "\n", capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    return r.stdout.splitlines()


def test_host_code_matches_python_integers(script):
    cmds, want = script
    got = run_harness(build_harness("fri_wide_host_harness", []), cmds)
    assert len(got) == len(want)
    for c, g, w in zip(cmds, got, want):
        assert g == w, c[:300]


def test_host_code_under_address_and_undefined_behaviour_sanitizers(script):
    """the same program, instrumented: a finding makes it exit non-zero with a report on stderr"""
    cmds, want = script
    exe = build_harness("fri_wide_host_harness_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan"])
    assert run_harness(exe, cmds) == want


# ---- header, library, binding ------------------------------------------------------------------------------------------------------
def test_fri_functions_are_declared_exported_and_bound():
    from icicle_amd import _lib

    text = re.sub(r"\s+", " ", subprocess.check_output(["gcc", "-E", "-P", os.path.join(ROOT, "include", "icicle_hip.h")], text=True))
    nargs = {"icicle_delete_fri_proof": 1, "fri_proof_get_nof_queries": 2, "fri_proof_get_nof_rounds": 2, "fri_proof_get_round_proofs_for_query": 3,
             "fri_proof_get_final_poly_size": 2, "fri_proof_get_final_poly": 2, "fri_proof_get_pow_nonce": 2, "fri_merkle_tree_prove": 8, "fri_merkle_tree_verify": 6,
             "hip_fri_fold": 6}
    assert set(nargs) == set(_lib.FRI_FUNCTIONS) and _lib.FRI_WIDE_PREFIXES == PREFIXES
    assert [_lib.FRI_WIDE_WORDS[p] for p in PREFIXES] == [fw.Field(f, e).words for f, e in fw.KINDS]
    for p in PREFIXES:
        for name, n in nargs.items():
            m = re.search(r"icicle_error_t %s_%s\s*\(([^)]*)\)\s*;" % (p, name), text)
            assert m and len(m.group(1).split(",")) == n, (p, name)
            fn = getattr(_lib.lib, f"{p}_{name}")
            assert f"{p}_{name}" in _lib.API_SYMBOLS and len(fn.argtypes) == n
        for name, n in (("icicle_initialize_fri_proof", 0), ("icicle_create_with_arguments_fri_proof", 6)):
            m = re.search(r"icicle_fri_proof_handle_t %s_%s\s*\(([^)]*)\)\s*;" % (p, name), text)
            assert m and (len(m.group(1).split(",")) == n or (n == 0 and m.group(1).strip() == "void")), (p, name)
            fn = getattr(_lib.lib, f"{p}_{name}")
            assert fn.restype is ctypes.c_void_p and len(fn.argtypes) == n and f"{p}_{name}" in _lib.FRI_HANDLE_SYMBOLS
    for absent in ("bw6_761_fri_merkle_tree_prove", "stark252_extension_fri_merkle_tree_prove", "bn254_extension_hip_fri_fold", "goldilocks_fri_proof_serialize"):
        assert absent not in text and not hasattr(_lib.lib, absent)
    assert not re.search(r"fri_merkle_tree", open(os.path.join(ROOT, "plugin", "hip_c_api.h")).read())  # no plugin registration


# ---- argument errors, with or without a device ---------------------------------------------------------------------------------------
def test_argument_errors_need_no_gpu():
    import icicle_amd
    from icicle_amd import FriConfig, FriProof, FriTranscriptConfig
    from icicle_amd._lib import lib
    from icicle_amd.hash import Hasher

    th = Hasher.keccak256()
    for field, ext in fw.KINDS:
        F, prefix = fw.Field(field, ext), fw.prefix(field, ext)
        leaves, compress = Hasher.blake2s(F.bytes), Hasher.blake2s(64)
        data = np.zeros((32, F.words), dtype=np.uint32)
        proof = FriProof(field, ext)
        assert (proof.nof_queries, proof.nof_rounds, proof.final_poly_size, proof.pow_nonce) == (0, 0, 0, 0)
        ffi, keep = FriTranscriptConfig.new_default_labels(th, 1)._ffi(ext, field)
        prove, verify = getattr(lib, prefix + "_fri_merkle_tree_prove"), getattr(lib, prefix + "_fri_merkle_tree_verify")
        c = FriConfig.default()
        c.nof_queries, c.pow_bits = 4, 0

        def run(with_cfg=True, with_t=True, d=data.ctypes.data, lh=leaves.handle, ch=compress.handle, pr=proof.handle):
            return prove(ctypes.byref(c) if with_cfg else None, ctypes.byref(ffi) if with_t else None, d, 32, lh, ch, 0, pr)

        # no domain is initialised in this process: a well-formed call ends at the domain check, on any machine; pointer errors come first
        assert run() == INVALID_ARGUMENT
        assert run(with_cfg=False) == INVALID_POINTER and run(with_t=False) == INVALID_POINTER and run(d=None) == INVALID_POINTER
        assert run(lh=None) == INVALID_POINTER and run(ch=None) == INVALID_POINTER and run(pr=None) == INVALID_POINTER
        ok = ctypes.c_bool(True)
        assert verify(ctypes.byref(c), ctypes.byref(ffi), proof.handle, leaves.handle, compress.handle, ctypes.byref(ok)) == 0 and ok.value is False
        assert verify(ctypes.byref(c), ctypes.byref(ffi), None, leaves.handle, compress.handle, ctypes.byref(ok)) == INVALID_POINTER
        assert verify(ctypes.byref(c), ctypes.byref(ffi), proof.handle, leaves.handle, compress.handle, None) == INVALID_POINTER
        for bad_leaves in (Hasher.blake2s(F.bytes + 4), Hasher.blake2s(4), Hasher.blake2s(0)):  # a leaf is one element
            assert verify(ctypes.byref(c), ctypes.byref(ffi), proof.handle, bad_leaves.handle, compress.handle, ctypes.byref(ok)) == INVALID_ARGUMENT
        fold = getattr(lib, prefix + "_hip_fri_fold")
        out, alpha = np.zeros_like(data), np.zeros(8, dtype=np.uint32)
        assert fold(data.ctypes.data, 32, alpha.ctypes.data, out.ctypes.data, False, None) == INVALID_ARGUMENT  # no domain
        assert fold(None, 32, alpha.ctypes.data, out.ctypes.data, False, None) == INVALID_POINTER
        with pytest.raises(icicle_amd.IcicleError):
            icicle_amd.fri_merkle_tree_prove(field, c, FriTranscriptConfig.new_default_labels(th, 1), data, leaves, compress, extension=ext)
        del keep
    with pytest.raises(AssertionError):
        FriProof("stark252", True)  # extension=True is valid for goldilocks only among the new fields


def test_a_proof_built_from_arguments_reads_back():
    """create_with_arguments copies the Merkle proofs and the final polynomial at the element size of the field. No GPU."""
    from icicle_amd import FriProof
    from icicle_amd.merkle import MerkleProof

    for case in CASES:
        F, pr = fw.case_field(case), fw.case_proof(case)
        rows = [[MerkleProof.with_data(False, idx, leaf, root, path) for idx, leaf, root, path in row] for row in pr["slots"]]
        fp = np.frombuffer(bytes.fromhex(case["final_poly"]), dtype=np.uint32)
        proof = FriProof.create_with_arguments(case["field"], rows, fp, case["nonce"], extension=case["extension"])
        del rows
        assert proof.nof_queries == 2 * case["nof_queries"] and proof.nof_rounds == len(pr["slots"][0])
        assert proof.final_poly_size == case["stopping_degree"] + 1 and proof.pow_nonce == case["nonce"]
        assert proof.final_poly.shape == (case["stopping_degree"] + 1, F.words) and proof.final_poly.tobytes().hex() == case["final_poly"]
        for q, row in enumerate(proof.slots()):
            for r, mp in enumerate(row):
                assert (mp.leaf_idx, mp.leaf, mp.root, mp.path) == pr["slots"][q][r]
