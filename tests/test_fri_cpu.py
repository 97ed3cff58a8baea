"""CPU: FRI without a GPU -- the Python model (tests/fri_model.py) against every fixture of the reference (tests/golden/
fri_vectors.json) byte for byte, the host-only protocol code (icicle_amd/csrc/fri_plan.h through tests/fri_host_harness.cpp, built
with g++ plainly and with -fsanitize=address,undefined as a program of its own) against the model, and the C ABI's surface: header,
library and binding agree, both structs have the reference's layout as the C compiler lays them out, and every argument error is
returned before the device is touched."""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest

from tests import blake_model as bm
from tests import fri_model as fm

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INVALID_POINTER, INVALID_ARGUMENT = 3, 11
PREFIXES = ["babybear", "babybear_extension", "koalabear", "koalabear_extension"]
CASES = fm.load_fixtures()


# ---- the model against the reference's proofs ----------------------------------------------------------------------------------------
def test_fixtures_cover_what_they_should():
    assert {(c["field"], c["extension"]) for c in CASES} == {(f, e) for f in ("babybear", "koalabear") for e in (False, True)}
    assert {c["pow_bits"] for c in CASES} == {0, 6} and {c["stopping_degree"] for c in CASES} == {0, 1, 3}
    assert any(c["log_domain"] > c["log_n"] for c in CASES) and any(c["public_state"] for c in CASES) and any(not c["public_state"] for c in CASES)
    assert any(c["transcript_hash"] not in (c["leaves_hash"], c["compress_hash"]) and bm.OUT_SIZE[c["transcript_hash"]] == 64 for c in CASES)
    assert {"keccak256", "sha3_256", "blake2s", "blake3"} <= {c["compress_hash"] for c in CASES}
    assert all(5 <= c["log_n"] <= 7 and c["nof_queries"] in (4, 5) for c in CASES)
    assert os.path.getsize(os.path.join(HERE, "golden", "fri_vectors.json")) < 256 * 1024


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_model_equals_the_reference(case):
    got = fm.prove(case["field"], case["extension"], fm.case_elements(case), *fm.case_protocol(case))
    want = fm.case_proof(case)
    assert got["final_poly"] == want["final_poly"]
    assert got["nonce"] == want["nonce"]
    assert len(got["slots"]) == len(want["slots"]) == 2 * case["nof_queries"]
    for q, (g, w) in enumerate(zip(got["slots"], want["slots"])):
        assert g == w, f"slot {q}"
    if case["name"] == "bb_scalar_query_equals_n":
        assert 1 << case["log_n"] in got["queries"]
    assert fm.verify(case["field"], case["extension"], want, *fm.case_protocol(case))


def test_model_verifier_rejects_a_changed_proof():
    case = CASES[1]
    for what in ("final_poly", "leaf", "path", "nonce", "public"):
        pr, proto = fm.case_proof(case), list(fm.case_protocol(case))
        if what == "final_poly":
            pr["final_poly"][0] = tuple(v ^ (i == 0) for i, v in enumerate(pr["final_poly"][0]))
        elif what == "nonce":
            pr["nonce"] += 1
        elif what == "public":
            proto[2] += b"!"
        else:
            idx, leaf, root, path = pr["slots"][3][1]
            flip = lambda b: bytes([b[0] ^ 1]) + b[1:]
            pr["slots"][3][1] = (idx, flip(leaf), root, path) if what == "leaf" else (idx, leaf, root, flip(path))
        assert not fm.verify(case["field"], case["extension"], pr, *proto), what


# ---- fri_plan.h on the host -----------------------------------------------------------------------------------------------------------
def build_harness(name, flags):
    exe = os.path.join(HERE, "_build", name)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    src = os.path.join(HERE, "fri_host_harness.cpp")
    hdr = os.path.join(ROOT, "icicle_amd", "csrc", "fri_plan.h")
    if not os.path.exists(exe) or max(os.path.getmtime(src), os.path.getmtime(hdr)) > os.path.getmtime(exe):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", *flags, src, "-o", exe])
    return exe


def hx(b: bytes) -> str:
    return b.hex() if b else "-"


def harness_script():
    """(commands, expected answers) from the model"""
    rng = random.Random(5)
    cmds, want = [], []

    def add(cmd, answer):
        cmds.append(cmd)
        want.append(answer)

    add("mt_nth 5489 10000", "4123659995")  # the value the C++ standard gives for std::mt19937
    for seed in (0, 1, 5489, 0xFFFFFFFF):
        mt = fm.Mt19937(seed)
        add(f"mt {seed} 1300", " ".join(str(mt.next()) for _ in range(1300)))  # across two twists
    # shapes: every fixture, larger sizes, and every rule
    for n, ff, sd, nq, chunk, out in [(1 << c["log_n"], 2, c["stopping_degree"], c["nof_queries"], 64, 32) for c in CASES] + [
            (1 << 20, 2, 0, 100, 64, 32), (1 << 24, 2, 7, 50, 128, 64), (2, 2, 0, 1, 64, 32), (1 << 31, 2, 0, 1, 64, 32),
            (32, 4, 0, 4, 64, 32), (32, 1, 0, 4, 64, 32), (0, 2, 0, 4, 64, 32), (48, 2, 0, 4, 64, 32), (32, 2, 0, 0, 64, 32), (32, 2, 0, 17, 64, 32), (32, 2, 0, 16, 64, 32),
            (32, 2, 0, 4, 32, 32), (32, 2, 0, 4, 128, 32), (32, 2, 0, 4, 64, 0), (32, 2, 0, 4, 96, 64), (32, 2, 2, 4, 64, 32), (32, 2, 31, 4, 64, 32), (32, 2, 15, 4, 64, 32),
            (1 << 32, 2, 0, 4, 64, 32), (32, 2, 2**64 - 1, 4, 64, 32)]:
        p = fm.plan(n, sd, nq, ff, chunk // out if out and chunk % out == 0 else 0)
        if p is None:
            add(f"plan {n} {ff} {sd} {nq} {chunk} {out}", "1")
        else:
            logn, rounds, fs = p
            shapes = " ".join(f"{n >> r}:{logn - r + 1}" for r in range(rounds))
            add(f"plan {n} {ff} {sd} {nq} {chunk} {out}", f"0 {logn} {rounds} {fs} {sum(n >> r for r in range(rounds + 1))} {shapes}".strip())
    # the sampler: small ranges (where the rejection threshold matters), the fixtures' ranges, the largest range
    for fs, n in [(1, 2), (1, 4), (2, 4), (1, 32), (4, 64), (8, 1 << 20), (1, 1 << 27), (1, 3 * 2**30), (1, 2**32 - 1)]:
        digest = bytes(rng.randrange(256) for _ in range(32))
        q = fm.draw_queries(int.from_bytes(digest[:4], "little"), 40, fs, n)
        assert all(fs <= v <= n for v in q)
        add(f"draw {digest.hex()} 40 {fs} {n}", " ".join(map(str, q)))
    for q, size in [(0, 2), (1, 2), (32, 32), (31, 32), (17, 16), (5, 8)]:
        for sym in (0, 1):
            add(f"leaf {q} {size} {sym}", str((q + sym * size // 2) % size))
    # F(digest)
    for field in ("babybear", "koalabear"):
        for ext in (False, True):
            F = fm.Field(field, ext)
            for size in (32, 64):
                for digest in (bytes(size), b"\xff" * size, bytes(rng.randrange(256) for _ in range(size))):
                    add(f"field {F.p} {F.words} {digest.hex()}", " ".join(map(str, F.from_digest(digest))))
    # transcript bytes: the fixtures' labels, empty ones, and long ones
    label_sets = [(tuple(s.encode() for s in c["labels"]), bytes.fromhex(c["public_state"]), c["log_n"]) for c in CASES]
    label_sets += [((b"", b"", b"", b""), b"", 1), ((bytes(range(256)), b"a" * 100, b"\x00", b"\xff\xfe"), bytes(300), 27)]
    for labels, public, logn in label_sets:
        for elem in (4, 16):
            tr = fm.Transcript("keccak256", labels, public, logn)
            prev, alpha = bytes(rng.randrange(256) for _ in range(elem)), bytes(rng.randrange(256) for _ in range(elem))
            for root_size, nonce in ((32, 0), (64, 2**32 + 5), (32, 2**64 - 1)):
                root = bytes(rng.randrange(256) for _ in range(root_size))
                add(f"transcript {' '.join(hx(s) for s in labels)} {hx(public)} {logn} {hx(prev)} {hx(root)} {hx(alpha)} {nonce}",
                    " ".join(hx(b) for b in (tr.entry0, tr.round_input(prev, root), tr.pow_challenge(alpha), tr.query_input(True, alpha, nonce),
                                             tr.query_input(False, alpha, nonce))))
    return cmds, want


@pytest.fixture(scope="module")
def script():
    return harness_script()


def run_harness(exe, cmds):
    r = subprocess.run([exe], input="\n".join(cmds) + "\n", capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    return r.stdout.splitlines()


def test_host_code_matches_the_model(script):
    cmds, want = script
    got = run_harness(build_harness("fri_host_harness", []), cmds)
    assert len(got) == len(want)
    for c, g, w in zip(cmds, got, want):
        assert g == w, c[:200]


def test_host_code_under_address_and_undefined_behaviour_sanitizers(script):
    """the same program, instrumented: a finding makes it exit non-zero with a report on stderr"""
    cmds, want = script
    exe = build_harness("fri_host_harness_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan"])
    assert run_harness(exe, cmds) == want


# ---- header, library, binding ------------------------------------------------------------------------------------------------------
def test_fri_functions_are_declared_exported_and_bound():
    from icicle_amd import _lib
    import icicle_amd

    text = re.sub(r"\s+", " ", subprocess.check_output(["gcc", "-E", "-P", os.path.join(ROOT, "include", "icicle_hip.h")], text=True))
    nargs = {"icicle_delete_fri_proof": 1, "fri_proof_get_nof_queries": 2, "fri_proof_get_nof_rounds": 2, "fri_proof_get_round_proofs_for_query": 3,
             "fri_proof_get_final_poly_size": 2, "fri_proof_get_final_poly": 2, "fri_proof_get_pow_nonce": 2, "fri_merkle_tree_prove": 8, "fri_merkle_tree_verify": 6,
             "hip_fri_fold": 6}
    assert set(nargs) == set(_lib.FRI_FUNCTIONS) and _lib.FRI_PREFIXES == PREFIXES
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
    # the three serialisation functions stay unbuilt
    assert "fri_proof_serialize" not in text and not hasattr(_lib.lib, "babybear_fri_proof_serialize")
    assert not re.search(r"fri_merkle_tree", open(os.path.join(ROOT, "plugin", "hip_c_api.h")).read())  # no plugin registration
    for name in ("FriConfig", "FriTranscriptConfig", "FriProof", "fri_merkle_tree_prove", "fri_merkle_tree_verify", "fri"):
        assert hasattr(icicle_amd, name), name
    t = icicle_amd.FriTranscriptConfig.new_default_labels(None, 1)
    assert (t.domain_separator_label, t.round_challenge_label, t.commit_phase_label, t.nonce_label, t.public_state) == (
        b"domain_separator_label", b"round_challenge_label", b"commit_phase_label", b"nonce_label", b"")


def test_struct_layouts_as_the_c_compiler_sees_them():
    from icicle_amd import _lib

    C, T = _lib.FriConfig, _lib.FFIFriTranscriptConfig
    assert ctypes.sizeof(C) == 56 and ctypes.sizeof(T) == 96
    d = C.default()
    assert (d.stream, d.folding_factor, d.stopping_degree, d.pow_bits, d.nof_queries, d.are_inputs_on_device, d.is_async, d.ext) == (None, 2, 0, 16, 100, False, False, None)
    cf = ["stream", "folding_factor", "stopping_degree", "pow_bits", "nof_queries", "are_inputs_on_device", "is_async", "ext"]
    tf = ["hasher", "domain_separator_label", "domain_separator_label_len", "round_challenge_label", "round_challenge_label_len", "commit_phase_label",
          "commit_phase_label_len", "nonce_label", "nonce_label_len", "public_state", "public_state_len", "seed_rng"]
    assert [f for f, _ in C._fields_] == cf and [f for f, _ in T._fields_] == tf
    prog = ('#include <stddef.h>\n#include <stdio.h>\n#include "icicle_hip.h"\nint main(void) { printf("%zu %zu", sizeof(icicle_fri_config_t), sizeof(icicle_fri_transcript_config_t));\n'
            + "".join(f'printf(" %zu", offsetof(icicle_fri_config_t, {f}));\n' for f in cf)
            + "".join(f'printf(" %zu", offsetof(icicle_fri_transcript_config_t, {f}));\n' for f in tf) + "return 0; }\n")
    build = os.path.join(HERE, "_build")
    os.makedirs(build, exist_ok=True)
    src, exe = os.path.join(build, "fri_layout.c"), os.path.join(build, "fri_layout")
    with open(src, "w") as f:
        f.write(prog)
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
    got = [int(v) for v in subprocess.check_output([exe], text=True).split()]
    assert got[:2] == [56, 96]
    assert got[2:10] == [getattr(C, f).offset for f in cf] == [0, 8, 16, 24, 32, 40, 41, 48]
    assert got[10:] == [getattr(T, f).offset for f in tf] == [0, 8, 16, 24, 32, 40, 48, 56, 64, 72, 80, 88]


# ---- argument errors, with or without a device ---------------------------------------------------------------------------------------
def test_argument_errors_need_no_gpu():
    import icicle_amd
    from icicle_amd import FriConfig, FriProof, FriTranscriptConfig
    from icicle_amd._lib import lib
    from icicle_amd.hash import Hasher

    th = Hasher.keccak256()
    for prefix in PREFIXES:
        ext = prefix.endswith("_extension")
        field, eb = prefix.split("_")[0], 16 if ext else 4
        leaves, compress = Hasher.blake2s(eb), Hasher.blake2s(64)
        data = np.zeros(32 * eb // 4, dtype=np.uint32)
        proof = FriProof(field, ext)
        assert (proof.nof_queries, proof.nof_rounds, proof.final_poly_size, proof.pow_nonce) == (0, 0, 0, 0)
        ffi, keep = FriTranscriptConfig.new_default_labels(th, 1)._ffi(ext)
        prove, verify = getattr(lib, prefix + "_fri_merkle_tree_prove"), getattr(lib, prefix + "_fri_merkle_tree_verify")

        def cfg(**kw):
            c = FriConfig.default()
            c.nof_queries, c.pow_bits = 4, 0
            for k, v in kw.items():
                setattr(c, k, v)
            return c

        def run(c=None, t=ffi, d=data.ctypes.data, n=32, lh=leaves.handle, ch=compress.handle, pr=proof.handle, with_cfg=True, with_t=True):
            c = c or cfg()
            return prove(ctypes.byref(c) if with_cfg else None, ctypes.byref(t) if with_t else None, d, n, lh, ch, 0, pr)

        # No domain is initialised in this process, so a well-formed call ends at the domain check with INVALID_ARGUMENT, on any machine;
        # the pointer errors below come before it. The argument errors proper cannot be told from that here: they are checked through
        # verify below (no domain needed) and through prove and the fold under a domain in tests/test_gpu_fri.py.
        assert run() == INVALID_ARGUMENT
        assert run(with_cfg=False) == INVALID_POINTER
        assert run(with_t=False) == INVALID_POINTER
        assert run(d=None) == INVALID_POINTER
        assert run(lh=None) == INVALID_POINTER and run(ch=None) == INVALID_POINTER and run(pr=None) == INVALID_POINTER
        for field_name in ("hasher", "seed_rng"):
            t2, keep2 = FriTranscriptConfig.new_default_labels(th, 1)._ffi(ext)
            setattr(t2, field_name, None)
            assert run(t=t2) == INVALID_POINTER, field_name
        # verify: the same pointer rules; an empty proof has no final polynomial -> a wrong proof, not an error
        ok = ctypes.c_bool(True)
        c = cfg()
        assert verify(ctypes.byref(c), ctypes.byref(ffi), proof.handle, leaves.handle, compress.handle, ctypes.byref(ok)) == 0 and ok.value is False
        assert verify(None, ctypes.byref(ffi), proof.handle, leaves.handle, compress.handle, ctypes.byref(ok)) == INVALID_POINTER
        assert verify(ctypes.byref(c), None, proof.handle, leaves.handle, compress.handle, ctypes.byref(ok)) == INVALID_POINTER
        assert verify(ctypes.byref(c), ctypes.byref(ffi), None, leaves.handle, compress.handle, ctypes.byref(ok)) == INVALID_POINTER
        assert verify(ctypes.byref(c), ctypes.byref(ffi), proof.handle, None, compress.handle, ctypes.byref(ok)) == INVALID_POINTER
        assert verify(ctypes.byref(c), ctypes.byref(ffi), proof.handle, leaves.handle, None, ctypes.byref(ok)) == INVALID_POINTER
        assert verify(ctypes.byref(c), ctypes.byref(ffi), proof.handle, leaves.handle, compress.handle, None) == INVALID_POINTER
        # the proof accessors
        n = ctypes.c_size_t()
        for name in ("fri_proof_get_nof_queries", "fri_proof_get_nof_rounds", "fri_proof_get_final_poly_size"):
            fn = getattr(lib, f"{prefix}_{name}")
            assert fn(None, ctypes.byref(n)) == INVALID_POINTER and fn(proof.handle, None) == INVALID_POINTER
        arr = (ctypes.c_void_p * 1)()
        assert getattr(lib, prefix + "_fri_proof_get_round_proofs_for_query")(proof.handle, 0, arr) == INVALID_ARGUMENT
        assert getattr(lib, prefix + "_icicle_delete_fri_proof")(None) == INVALID_POINTER
        # the fold helper
        fold = getattr(lib, prefix + "_hip_fri_fold")
        out, alpha = np.zeros_like(data), np.zeros(4, dtype=np.uint32)
        assert fold(data.ctypes.data, 32, alpha.ctypes.data, out.ctypes.data, False, None) == INVALID_ARGUMENT  # no domain (sizes: test_gpu_fri.py)
        assert fold(None, 32, alpha.ctypes.data, out.ctypes.data, False, None) == INVALID_POINTER
        with pytest.raises(icicle_amd.IcicleError):
            icicle_amd.fri_merkle_tree_prove(field, cfg(), FriTranscriptConfig.new_default_labels(th, 1), data.reshape(-1, 4) if ext else data, leaves, compress,
                                             extension=ext)
        del keep


def rebuilt(case):
    from icicle_amd import FriProof
    from icicle_amd.merkle import MerkleProof

    rows = [[MerkleProof.with_data(False, idx, leaf, root, path) for idx, leaf, root, path in row] for row in fm.case_proof(case)["slots"]]
    return FriProof.create_with_arguments(case["field"], rows, np.array(case["final_poly"], dtype=np.uint32), case["nonce"], extension=case["extension"])


@pytest.mark.parametrize("case", [CASES[0], CASES[1], CASES[2], CASES[3]], ids=[c["name"] for c in CASES[:4]])
def test_verify_tells_every_argument_error_from_an_accepted_call(case):
    """verify checks its arguments before it touches the device and needs no NTT domain, so on a reference proof rebuilt with
    create_with_arguments a well-formed call gets past the checks -- it ends valid on a GPU and in a device error, never INVALID_ARGUMENT,
    without one -- while each bad argument is refused with INVALID_ARGUMENT and a proof that does not fit the configuration is a wrong
    proof (SUCCESS, valid = false), with or without a GPU."""
    from icicle_amd import FriConfig, FriTranscriptConfig, runtime
    from icicle_amd._lib import lib
    from icicle_amd.hash import Hasher

    ext, field = case["extension"], case["field"]
    prefix, eb = f"{field}_extension" if ext else field, 16 if ext else 4
    make = lambda name, chunk=0: getattr(Hasher, name)(chunk)
    out = bm.OUT_SIZE[case["compress_hash"]]
    th, leaves, compress = make(case["transcript_hash"]), make(case["leaves_hash"], eb), make(case["compress_hash"], 2 * out)
    proto = fm.case_protocol(case)
    ffi, keep = FriTranscriptConfig(th, *proto[1], proto[2], list(proto[3]))._ffi(ext)
    proof = rebuilt(case)
    verify = getattr(lib, prefix + "_fri_merkle_tree_verify")

    def run(lh=leaves, ch=compress, **kw):
        c = FriConfig.default()
        c.stopping_degree, c.pow_bits, c.nof_queries = case["stopping_degree"], case["pow_bits"], case["nof_queries"]
        for k, v in kw.items():
            setattr(c, k, v)
        ok = ctypes.c_bool(True)
        return verify(ctypes.byref(c), ctypes.byref(ffi), proof.handle, lh.handle, ch.handle, ctypes.byref(ok)), ok.value

    rc, ok = run()
    if runtime.get_device_count() > 0:
        assert (rc, ok) == (0, True)
    else:
        assert rc not in (0, INVALID_ARGUMENT, INVALID_POINTER) and ok is False  # past every check, stopped by the missing device
    sd = case["stopping_degree"]
    for bad in (dict(folding_factor=4), dict(folding_factor=0), dict(folding_factor=1), dict(nof_queries=0), dict(pow_bits=61), dict(pow_bits=2**40),
                dict(stopping_degree=2), dict(stopping_degree=2**64 - 1)):
        assert run(**bad) == (INVALID_ARGUMENT, False), bad
    # compress arity 1, 4, a chunk that is no multiple of the digest, no chunk; chunk and digest size must not be swapped (64 / 32, not 32 / 64)
    for bad_compress in (make(case["compress_hash"], out), make(case["compress_hash"], 4 * out), make(case["compress_hash"], 2 * out + 1), make(case["compress_hash"], 0),
                         make("keccak512" if out == 32 else "keccak256", 2 * out)):
        assert run(ch=bad_compress) == (INVALID_ARGUMENT, False)
    for bad_leaves in (make(case["leaves_hash"], eb + 4), make(case["leaves_hash"], 20 - eb), make(case["leaves_hash"], 0)):
        assert run(lh=bad_leaves) == (INVALID_ARGUMENT, False)  # a leaf is one element
    # the proof against the configuration: another final size, another number of slots -- a wrong proof, not an error
    n = 1 << case["log_n"]
    for wrong in (dict(stopping_degree=2 * sd + 1), dict(nof_queries=case["nof_queries"] + 1), dict(nof_queries=n // 2 + 1), dict(nof_queries=1)):
        assert run(**wrong) == (0, False), wrong
    del keep


def test_a_proof_built_from_arguments_reads_back():
    """create_with_arguments copies the Merkle proofs; the borrowed handles work with the icicle_merkle_proof_get_* functions. No GPU."""
    from icicle_amd import FriProof
    from icicle_amd.merkle import MerkleProof

    case = CASES[1]
    pr = fm.case_proof(case)
    rows = [[MerkleProof.with_data(False, idx, leaf, root, path) for idx, leaf, root, path in row] for row in pr["slots"]]
    fp = np.array(case["final_poly"], dtype=np.uint32)
    proof = FriProof.create_with_arguments(case["field"], rows, fp, case["nonce"], extension=case["extension"])
    del rows  # the proof holds copies
    assert proof.nof_queries == 2 * case["nof_queries"] and proof.nof_rounds == len(pr["slots"][0])
    assert proof.final_poly_size == case["stopping_degree"] + 1 and proof.pow_nonce == case["nonce"]
    assert proof.final_poly.reshape(-1).tolist() == case["final_poly"]
    for q, row in enumerate(proof.slots()):
        for r, mp in enumerate(row):
            assert (mp.leaf_idx, mp.leaf, mp.root, mp.path) == pr["slots"][q][r] and not mp.pruned
