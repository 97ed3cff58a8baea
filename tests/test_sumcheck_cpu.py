"""CPU: sumcheck without a GPU -- the Python model (tests/sumcheck_model.py) against every fixture of the reference (tests/golden/
sumcheck_vectors.json) byte for byte, the host-only protocol code (icicle_amd/csrc/sumcheck_plan.h and program_plan.h through
tests/sumcheck_host_harness.cpp, built with g++ plainly and with -fsanitize=address,undefined as a program of its own) against the
model, and the C ABI's surface: header, library and binding agree, both structs have the reference's layout as the C compiler lays
them out, and every argument error is returned before the device is touched. The large fixtures (tests/golden/
sumcheck_vectors_large.json): the generator reproduces the recorded inputs, every proof passes the model's verifier, and the claimed
sums of the babybear cases are recomputed in 64-bit arithmetic."""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest

from tests import blake_model as bm
from tests import sumcheck_model as sm

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INVALID_POINTER, INVALID_ARGUMENT = 3, 11
FIELDS = ["babybear", "koalabear", "bn254", "bls12_381"]
CASES = sm.load_fixtures()


def case_args(case):
    """(field, claimed sum, transcript hasher, labels, seed)"""
    return case["field"], int(case["claimed_sum"], 16), case["transcript_hash"], sm.case_labels(case), int(case["seed"], 16)


# ---- the model against the reference's proofs ----------------------------------------------------------------------------------------
def test_fixtures_cover_what_they_should():
    assert {c["field"] for c in CASES} == set(FIELDS)
    for f in FIELDS:
        assert {c["program"].get("predefined") for c in CASES if c["field"] == f} >= {0, 1}, f
    user = [sm.Program.from_description(c["program"]) for c in CASES if "predefined" not in c["program"]]
    assert any(p.degree() == 1 for p in user) and any(p.degree() == 6 and p.nof_inputs == 6 for p in user)
    assert any(sum(n[0] == "const" for n in p.nodes) >= 1 and any(n[0] != "const" and len(n) == 3 and n[1] == n[2] for n in p.nodes) for p in user)  # a node used twice
    assert len({c["name"] for c in CASES if "predefined" not in c["program"]}) >= 3
    assert {c["log_n"] for c in CASES} == set(range(1, 8))
    one_word = lambda c: sm.FIELDS[c["field"]][1] == 1
    assert any(bm.OUT_SIZE[c["transcript_hash"]] == 64 and one_word(c) for c in CASES) and any(bm.OUT_SIZE[c["transcript_hash"]] == 64 and not one_word(c) for c in CASES)
    assert {"blake2s", "blake3"} & {c["transcript_hash"] for c in CASES}
    assert any(c["labels"] == ["", "", ""] for c in CASES)
    values = [(sm.FIELDS[c["field"]][0], {int(v, 16) for t in c["polys"] for v in t}) for c in CASES]
    assert any(v == {p - 1} for p, v in values) and any(v == {0} for p, v in values)
    assert os.path.getsize(os.path.join(HERE, "golden", "sumcheck_vectors.json")) < 256 * 1024


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_model_equals_the_reference(case):
    field, claimed, hasher, labels, seed = case_args(case)
    program = sm.Program.from_description(case["program"])
    assert program.degree() == case["degree"]
    got = sm.prove(field, sm.unhex(case["polys"]), claimed, program, hasher, labels, seed)
    assert got["round_polys"] == sm.unhex(case["round_polys"])
    assert got["challenges"] == [int(v, 16) for v in case["challenges"]] and got["challenges"][0] == 0
    assert sm.verify(field, got["round_polys"], claimed, hasher, labels, seed)


def test_model_verifier_rejects_a_changed_proof():
    for case in (CASES[4], CASES[14]):  # one word with L = 7, eight words with L = 4
        field, claimed, hasher, labels, seed = case_args(case)
        p = sm.FIELDS[field][0]
        good = sm.unhex(case["round_polys"])
        assert sm.verify(field, good, claimed, hasher, labels, seed)
        for r in (0, len(good) // 2, len(good) - 2):
            for k in range(len(good[0])):
                bad = [list(row) for row in good]
                bad[r][k] = (bad[r][k] + 1) % p
                assert not sm.verify(field, bad, claimed, hasher, labels, seed), (r, k)
        assert not sm.verify(field, good, (claimed + 1) % p, hasher, labels, seed)
        for i in range(3):
            changed = tuple(l + b"!" if j == i else l for j, l in enumerate(labels))
            assert not sm.verify(field, good, claimed, hasher, changed, seed), i
        assert not sm.verify(field, good, claimed, hasher, labels, (seed + 1) % p)
        assert not sm.verify(field, [], claimed, hasher, labels, seed)
        assert not sm.verify(field, [row[:1] for row in good], claimed, hasher, labels, seed)


# ---- sumcheck_plan.h and program_plan.h on the host ------------------------------------------------------------------------------------
def build_harness(name, flags):
    exe = os.path.join(HERE, "_build", name)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    src = os.path.join(HERE, "sumcheck_host_harness.cpp")
    deps = [src] + [os.path.join(ROOT, "icicle_amd", "csrc", h) for h in ("sumcheck_plan.h", "program_plan.h", "field_consts.h")]
    if not os.path.exists(exe) or max(os.path.getmtime(d) for d in deps) > os.path.getmtime(exe):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", *flags, src, "-o", exe])
    return exe


def hx(b: bytes) -> str:
    return b.hex() if b else "-"


TAIL20 = [["const", 1], ["const", 2], ["add", 14, 15], ["add", 17, 16], ["add", 18, 15]]  # after the sum of eight inputs (node 14)


def node_spec(field, program):
    return ",".join(f"const:{hx(sm.to_bytes(field, n[1]))}" if n[0] == "const" else ":".join(str(v) for v in n) for n in program.nodes)


def harness_script():
    """(commands, expected answers) from the model"""
    rng = random.Random(11)
    cmds, want = [], []

    def add(cmd, answer):
        cmds.append(cmd)
        want.append(answer)

    el = lambda field, v: hx(sm.to_bytes(field, v))
    for field in FIELDS:
        p, w = sm.FIELDS[field]
        rand = lambda: rng.randrange(p)
        # F(digest): 32 and 64 bytes, all zero, all ones, the modulus itself, random
        for size in (32, 64):
            for digest in (bytes(size), b"\xff" * size, p.to_bytes(size, "little"), (p - 1).to_bytes(size, "little"), bytes(rng.randrange(256) for _ in range(size))):
                add(f"digest {field} {digest.hex()}", el(field, sm.from_digest(field, digest)))
        for a, b in [(0, 0), (1, p - 1), (p - 1, p - 1), (p - 1, 1), (2, (p + 1) // 2)] + [(rand(), rand()) for _ in range(6)]:
            add(f"arith {field} {el(field, a)} {el(field, b)}", " ".join(el(field, v) for v in ((a + b) % p, (a - b) % p, a * b % p, pow(a, p - 2, p))))
        for count in range(2, 8):
            evals, x = [rand() for _ in range(count)], rand()
            add(f"lagrange {field} {el(field, x)} " + " ".join(el(field, v) for v in evals), el(field, sm.lagrange(p, evals, x)))
        evals = [rand() for _ in range(4)]
        add(f"lagrange {field} {el(field, 2)} " + " ".join(el(field, v) for v in evals), el(field, evals[2]))  # at a node
        # transcript bytes: the fixtures' labels, empty and long ones
        label_sets = [sm.case_labels(c) for c in CASES if c["field"] == field] + [(b"", b"", b""), (bytes(range(256)), b"a" * 100, b"\x00\xff")]
        for labels in label_sets:
            rounds, d, claimed, seed, alpha = rng.randrange(1, 21), rng.randrange(1, 7), rand(), rand(), rand()
            tr = sm.Transcript(field, "keccak256", labels, seed, rounds, d, claimed)
            poly = [rand() for _ in range(d + 1)]
            poly_hex = hx(b"".join(sm.to_bytes(field, v) for v in poly))
            for r in (0, 1, rounds - 1):
                add(f"transcript {' '.join(hx(s) for s in labels)} {rounds} {d} {field} {el(field, claimed)} {el(field, seed)} {r} {el(field, alpha)} {poly_hex}",
                    f"{hx(tr.entry0)} {hx(tr.round_input(r, alpha, poly))}")
        # programs: degree, variable count, acceptance, value
        for pid, m in ((0, 3), (1, 4)):
            prog = sm.Program(m, predefined=pid)
            for nof_polys in (m, m - 1, m + 1):
                x = [rand() for _ in range(m)]
                add(f"predefined {field} {pid} {nof_polys} " + " ".join(el(field, v) for v in x),
                    f"{prog.degree()} {m + 1} 0 {int(sm.acceptable(prog, nof_polys))} {el(field, prog.evaluate(p, x))}")
        add(f"predefined {field} 2 3", "refused")
        programs = [sm.Program.from_description(c["program"]) for c in CASES if "predefined" not in c["program"] and c["field"] == field]
        ins = [["in", i] for i in range(8)]
        chain = lambda n, op: [[op, 7 + j if j else 0, j + 1] for j in range(n)]  # ((x0 op x1) op x2) ..
        programs += [
            sm.Program(1, [["in", 0]]),                                    # the return value is an input: one copy
            sm.Program(2, [["in", 0], ["const", 3]]),                      # a constant: degree 0, refused by the prover
            sm.Program(2, ins[:2] + [["mul", 0, 1], ["inv", 2], ["add", 3, 0]]),  # an inverse: degree -1
            sm.Program(8, ins + chain(6, "mul")),                          # degree 7 over 7 of 8 inputs
            sm.Program(8, ins + chain(5, "mul") + [["add", 12, 7]]),       # degree 6 over 8 inputs
            sm.Program(8, ins + chain(7, "add") + TAIL20),                 # 20 variables: 9 parameters, 2 constants, 10 operations, less one
            sm.Program(8, ins + chain(7, "add") + TAIL20 + [["add", 19, 16]]),  # 21 variables
            sm.Program(2, ins[:2] + [["const", 9], ["mul", 0, 0], ["sub", 3, 1]]),  # a constant nothing reaches is not a variable
            sm.Program(3, ins[:3] + [["sub", 0, 1], ["mul", 3, 3], ["mul", 4, 3], ["add", 5, 2]]),
        ]
        for prog in programs:
            m = prog.nof_inputs
            x = [rand() for _ in range(m)]
            n_ops = sum(prog.nodes[j][0] not in ("in", "const") for j in prog._reachable())
            n_ins = n_ops if n_ops else 1  # an input or a constant as the return value is copied into the output slot
            value = el(field, prog.evaluate(p, x)) if prog.degree() >= 0 else "-"
            add(f"program {field} {m} {m} {node_spec(field, prog)} " + " ".join(el(field, v) for v in x),
                f"{prog.degree()} {prog.nof_vars()} {n_ins} {int(sm.acceptable(prog, m))} {value}")
        add(f"program {field} 1 1 in:3", "refused")  # an input index outside the inputs
    return cmds, want


@pytest.fixture(scope="module")
def script():
    return harness_script()


def run_harness(exe, cmds):
    r = subprocess.run([exe], input="\n".join(cmds) + "\n", capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    return r.stdout.splitlines()


def test_the_models_own_rules():
    """the limits the harness answers are compared with: a 20-variable program is accepted, 21 refused, degree 7 refused"""
    ins = [["in", i] for i in range(8)]
    chain = lambda n, op: [[op, 7 + j if j else 0, j + 1] for j in range(n)]
    assert sm.Program(8, ins + chain(6, "mul")).degree() == 7
    p20 = sm.Program(8, ins + chain(7, "add") + TAIL20)
    assert p20.nof_vars() == 20 and sm.acceptable(p20, 8)
    p21 = sm.Program(8, p20.nodes + [["add", 19, 16]])
    assert p21.nof_vars() == 21 and not sm.acceptable(p21, 8)


def test_host_code_matches_the_model(script):
    cmds, want = script
    got = run_harness(build_harness("sumcheck_host_harness", []), cmds)
    assert len(got) == len(want)
    for c, g, w in zip(cmds, got, want):
        assert g == w, c[:300]


def test_host_code_under_address_and_undefined_behaviour_sanitizers(script):
    """the same program, instrumented: a finding makes it exit non-zero with a report on stderr"""
    cmds, want = script
    exe = build_harness("sumcheck_host_harness_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan"])
    assert run_harness(exe, cmds) == want


# ---- header, library, binding ------------------------------------------------------------------------------------------------------
ERROR_FUNCTIONS = {"sumcheck_delete": 1, "hip_sumcheck_prove": 9, "sumcheck_verify": 5, "sumcheck_proof_get_poly_sizes": 3, "sumcheck_proof_delete": 1,
                   "sumcheck_get_challenge_vector": 3, "sumcheck_get_challenge_size": 2, "generate_returning_value_program": 3, "add_symbols": 3, "sub_symbols": 3,
                   "multiply_symbols": 3, "inverse_symbol": 2}
HANDLE_FUNCTIONS = {"sumcheck_create": ("icicle_sumcheck_handle_t", 0), "sumcheck_get_proof": ("icicle_sumcheck_proof_handle_t", 8),
                    "sumcheck_proof_create": ("icicle_sumcheck_proof_handle_t", 3), "sumcheck_proof_get_round_poly_at": (r"uint32_t\s*\*", 2),
                    "create_predefined_returning_value_program": ("icicle_program_handle_t", 1), "create_input_symbol": ("icicle_symbol_handle_t", 1),
                    "create_scalar_symbol": ("icicle_symbol_handle_t", 1), "copy_symbol": ("icicle_symbol_handle_t", 1)}


def test_sumcheck_functions_are_declared_exported_and_bound():
    from icicle_amd import _lib
    import icicle_amd

    text = re.sub(r"\s+", " ", subprocess.check_output(["gcc", "-E", "-P", os.path.join(ROOT, "include", "icicle_hip.h")], text=True))
    assert set(ERROR_FUNCTIONS) == set(_lib.SUMCHECK_FUNCTIONS) and list(_lib.SUMCHECK_FIELDS) == FIELDS
    assert [_lib.SUMCHECK_FIELDS[f] for f in FIELDS] == [sm.FIELDS[f][1] for f in FIELDS]
    for p in FIELDS:
        for name, n in ERROR_FUNCTIONS.items():
            m = re.search(r"icicle_error_t %s_%s\s*\(([^)]*)\)\s*;" % (p, name), text)
            assert m and len(m.group(1).split(",")) == n, (p, name)
            assert f"{p}_{name}" in _lib.API_SYMBOLS and len(getattr(_lib.lib, f"{p}_{name}").argtypes) == n
        for name, (ret, n) in HANDLE_FUNCTIONS.items():
            m = re.search(r"%s %s_%s\s*\(([^)]*)\)\s*;" % (ret, p, name), text)
            assert m and (len(m.group(1).split(",")) == n or (n == 0 and m.group(1).strip() == "void")), (p, name)
            fn = getattr(_lib.lib, f"{p}_{name}")
            assert fn.restype is ctypes.c_void_p and len(fn.argtypes) == n and f"{p}_{name}" in _lib.SUMCHECK_HANDLE_SYMBOLS
    assert re.search(r"icicle_error_t delete_program\s*\(", text) and "delete_program" in _lib.API_SYMBOLS
    # what stays unbuilt: serialisation, printing, the extension_ and rns_ variants, the other fields, the plugin
    for absent in ("sumcheck_proof_serialize", "sumcheck_proof_deserialize", "sumcheck_proof_get_serialized_size", "sumcheck_proof_print",
                   "extension_create_input_symbol", "rns_create_input_symbol", "goldilocks_sumcheck_create", "stark252_sumcheck_create", "bls12_377_sumcheck_create",
                   "grumpkin_sumcheck_create"):
        assert absent not in text and not hasattr(_lib.lib, "babybear_" + absent) and not hasattr(_lib.lib, absent), absent
    assert not re.search(r"sumcheck", open(os.path.join(ROOT, "plugin", "hip_c_api.h")).read())
    for name in ("Symbol", "ReturningValueProgram", "SumcheckConfig", "SumcheckTranscriptConfig", "Sumcheck", "SumcheckProof", "sumcheck"):
        assert hasattr(icicle_amd, name), name


def test_struct_layouts_as_the_c_compiler_sees_them():
    from icicle_amd import _lib

    C, T = _lib.SumcheckConfig, _lib.FFISumcheckTranscriptConfig
    assert ctypes.sizeof(C) == 40 and ctypes.sizeof(T) == 72
    d = C.default()
    assert (d.stream, d.use_extension_field, d.batch, d.are_inputs_on_device, d.is_async, d.ext) == (None, False, 1, False, False, None)
    cf = ["stream", "use_extension_field", "batch", "are_inputs_on_device", "is_async", "ext"]
    tf = ["hasher", "domain_separator_label", "domain_separator_label_len", "round_poly_label", "round_poly_label_len", "round_challenge_label",
          "round_challenge_label_len", "little_endian", "seed_rng"]
    assert [f for f, _ in C._fields_] == cf and [f for f, _ in T._fields_] == tf
    prog = ('#include <stddef.h>\n#include <stdio.h>\n#include "icicle_hip.h"\nint main(void) { printf("%zu %zu", sizeof(icicle_sumcheck_config_t), '
            'sizeof(icicle_sumcheck_transcript_config_t));\n'
            + "".join(f'printf(" %zu", offsetof(icicle_sumcheck_config_t, {f}));\n' for f in cf)
            + "".join(f'printf(" %zu", offsetof(icicle_sumcheck_transcript_config_t, {f}));\n' for f in tf) + "return 0; }\n")
    build = os.path.join(HERE, "_build")
    os.makedirs(build, exist_ok=True)
    src, exe = os.path.join(build, "sumcheck_layout.c"), os.path.join(build, "sumcheck_layout")
    with open(src, "w") as f:
        f.write(prog)
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
    got = [int(v) for v in subprocess.check_output([exe], text=True).split()]
    assert got[:2] == [40, 72]
    assert got[2:8] == [getattr(C, f).offset for f in cf] == [0, 8, 16, 24, 25, 32]
    assert got[8:] == [getattr(T, f).offset for f in tf] == [0, 8, 16, 24, 32, 40, 48, 56, 64]


# ---- argument errors, with or without a device ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", FIELDS)
def test_argument_errors_need_no_gpu(field):
    import icicle_amd
    from icicle_amd import ReturningValueProgram, Sumcheck, SumcheckConfig, SumcheckProof, SumcheckTranscriptConfig, Symbol, runtime
    from icicle_amd._lib import lib
    from icicle_amd.hash import Hasher

    w = sm.FIELDS[field][1]
    th = Hasher.keccak256()
    tcfg = SumcheckTranscriptConfig(th, "ds", "poly", "challenge", 1)
    ffi, keep = tcfg._ffi(field)
    sc, proof = Sumcheck(field), SumcheckProof(field)
    assert proof.sizes() == (0, 0) and sc.challenge_vector().size == 0
    eq = ReturningValueProgram.predefined(field, 1)
    ab = ReturningValueProgram.predefined(field, 0)
    polys = [np.zeros(8 * w, dtype=np.uint32) for _ in range(8)]
    claimed = (ctypes.c_uint32 * w)()
    prove = getattr(lib, field + "_hip_sumcheck_prove")

    def run(n=8, m=4, program=eq, cfg=None, t=ffi, s=sc.handle, table=True, c=claimed, pr=proof.handle, with_cfg=True, with_t=True):
        cfg = cfg or SumcheckConfig.default()
        ptrs = (ctypes.c_void_p * 8)(*[p.ctypes.data for p in polys])
        return prove(s, ptrs if table else None, n, m, c, program.handle if program else None, ctypes.byref(t) if with_t else None,
                     ctypes.byref(cfg) if with_cfg else None, pr)

    # a well-formed call gets past every check: it succeeds on a GPU and ends in a device error, never an argument error, without one
    rc = run()
    if runtime.get_device_count() > 0:
        assert rc == 0
    else:
        assert rc not in (0, INVALID_ARGUMENT, INVALID_POINTER)
    for n in (0, 1, 3, 6, 12, 2**41):
        assert run(n=n) == INVALID_ARGUMENT, n
    assert run(m=3) == INVALID_ARGUMENT and run(m=5) == INVALID_ARGUMENT and run(m=4, program=ab) == INVALID_ARGUMENT and run(m=0) == INVALID_ARGUMENT
    ext = SumcheckConfig.default()
    ext.use_extension_field = True
    assert run(cfg=ext) == INVALID_ARGUMENT
    other = ReturningValueProgram.predefined("bn254" if w == 1 else "babybear", 1)
    assert run(program=other) == INVALID_ARGUMENT  # a program of a field with another element size
    # user programs: nine inputs, degree 0, 7 and -1, 21 variables
    nine = ReturningValueProgram.from_function(field, lambda x: x[0] + x[8], 9)
    assert run(m=9, program=nine) == INVALID_ARGUMENT
    const = ReturningValueProgram.from_function(field, lambda x: 3, 2)
    assert run(m=2, program=const) == INVALID_ARGUMENT
    deg7 = ReturningValueProgram.from_function(field, lambda x: x[0] * x[1] * x[2] * x[3] * x[4] * x[5] * x[6], 7)
    assert run(m=7, program=deg7) == INVALID_ARGUMENT
    inv = ReturningValueProgram.from_function(field, lambda x: (x[0] * x[1]).inverse() + x[0], 2)
    assert run(m=2, program=inv) == INVALID_ARGUMENT

    def sum_with_constants(count):
        def fn(x):
            acc = x[0]
            for j in range(1, 8):
                acc = acc + x[j]
            for c in range(count):
                acc = acc + (c + 1)
            return acc
        return fn

    assert run(m=8, program=ReturningValueProgram.from_function(field, sum_with_constants(4), 8)) == INVALID_ARGUMENT  # 9 + 4 + 11 - 1 = 23 variables
    vars20 = ReturningValueProgram.from_function(field, sum_with_constants(2), 8)  # 9 + 2 + 9 - 1 = 19
    rc = run(m=8, program=vars20)
    assert rc == 0 if runtime.get_device_count() > 0 else rc not in (0, INVALID_ARGUMENT, INVALID_POINTER)
    # NULL pointers
    assert run(s=None) == INVALID_POINTER and run(table=False) == INVALID_POINTER and run(c=None) == INVALID_POINTER and run(program=None) == INVALID_POINTER
    assert run(with_t=False) == INVALID_POINTER and run(with_cfg=False) == INVALID_POINTER and run(pr=None) == INVALID_POINTER
    for name in ("hasher", "seed_rng"):
        t2, keep2 = tcfg._ffi(field)
        setattr(t2, name, None)
        assert run(t=t2) == INVALID_POINTER, name
    null_poly = (ctypes.c_void_p * 8)(*[polys[0].ctypes.data, None, polys[2].ctypes.data, polys[3].ctypes.data] + [None] * 4)
    cfg = SumcheckConfig.default()
    assert prove(sc.handle, null_poly, 8, 4, claimed, eq.handle, ctypes.byref(ffi), ctypes.byref(cfg), proof.handle) == INVALID_POINTER
    # get_proof returns NULL where the _hip_ form returns an error
    ptrs = (ctypes.c_void_p * 8)(*[p.ctypes.data for p in polys])
    assert getattr(lib, field + "_sumcheck_get_proof")(sc.handle, ptrs, 6, 4, claimed, eq.handle, ctypes.byref(ffi), ctypes.byref(cfg)) is None
    # verify: pointer rules; an empty proof and a wrong claimed sum are wrong proofs, not errors, and need no device
    verify = getattr(lib, field + "_sumcheck_verify")
    ok = ctypes.c_bool(True)
    assert verify(sc.handle, proof.handle, claimed, ctypes.byref(ffi), ctypes.byref(ok)) == 0 and ok.value is False
    case = next(c for c in CASES if c["field"] == field and c["log_n"] >= 2)
    rps = np.array([[(int(v, 16) >> (32 * i)) & 0xFFFFFFFF for v in row for i in range(w)] for row in case["round_polys"]], dtype=np.uint32)
    rebuilt = SumcheckProof.create(field, rps)
    assert rebuilt.sizes() == (case["degree"] + 1, case["log_n"]) and np.array_equal(rebuilt.round_polys().reshape(rps.shape), rps)
    ok = ctypes.c_bool(True)
    assert not sc.verify(rebuilt, (int(case["claimed_sum"], 16) + 1) % sm.FIELDS[field][0], tcfg)
    ragged = getattr(lib, field + "_sumcheck_proof_create")
    assert verify(None, rebuilt.handle, claimed, ctypes.byref(ffi), ctypes.byref(ok)) == INVALID_POINTER
    assert verify(sc.handle, None, claimed, ctypes.byref(ffi), ctypes.byref(ok)) == INVALID_POINTER
    assert verify(sc.handle, rebuilt.handle, None, ctypes.byref(ffi), ctypes.byref(ok)) == INVALID_POINTER
    assert verify(sc.handle, rebuilt.handle, claimed, None, ctypes.byref(ok)) == INVALID_POINTER
    assert verify(sc.handle, rebuilt.handle, claimed, ctypes.byref(ffi), None) == INVALID_POINTER
    assert ragged(None, 2, 3) is None
    # the accessors
    n64, n = ctypes.c_uint64(), ctypes.c_size_t()
    assert getattr(lib, field + "_sumcheck_proof_get_poly_sizes")(None, ctypes.byref(n64), ctypes.byref(n64)) == INVALID_ARGUMENT
    assert getattr(lib, field + "_sumcheck_proof_get_poly_sizes")(proof.handle, None, ctypes.byref(n64)) == INVALID_POINTER
    assert getattr(lib, field + "_sumcheck_proof_get_round_poly_at")(proof.handle, 0) is None
    assert getattr(lib, field + "_sumcheck_proof_get_round_poly_at")(rebuilt.handle, case["log_n"]) is None
    assert getattr(lib, field + "_sumcheck_get_challenge_size")(None, ctypes.byref(n)) == INVALID_ARGUMENT
    assert getattr(lib, field + "_sumcheck_get_challenge_size")(sc.handle, None) == INVALID_POINTER
    n.value = 5  # more than the vector holds: nothing is copied, the count comes back
    buf = np.full(5 * w, 7, dtype=np.uint32)
    assert getattr(lib, field + "_sumcheck_get_challenge_vector")(sc.handle, buf.ctypes.data, ctypes.byref(n)) == 0 and n.value == 0 and (buf == 7).all()
    assert getattr(lib, field + "_sumcheck_delete")(None) == INVALID_ARGUMENT and getattr(lib, field + "_sumcheck_proof_delete")(None) == INVALID_ARGUMENT
    assert lib.delete_program(None) == INVALID_POINTER
    # symbols
    a = Symbol.input(field, 0)
    out = ctypes.c_void_p()
    assert getattr(lib, field + "_add_symbols")(a.handle, None, ctypes.byref(out)) == INVALID_ARGUMENT
    assert getattr(lib, field + "_inverse_symbol")(None, ctypes.byref(out)) == INVALID_POINTER
    assert getattr(lib, field + "_create_scalar_symbol")(None) is None
    too_big = (ctypes.c_uint32 * w)(*[0xFFFFFFFF] * w)
    assert getattr(lib, field + "_create_scalar_symbol")(too_big) is None  # not canonical
    prog = ctypes.c_void_p()
    params = (ctypes.c_void_p * 2)(a.handle, None)
    assert getattr(lib, field + "_generate_returning_value_program")(params, 2, ctypes.byref(prog)) == INVALID_ARGUMENT
    with pytest.raises(icicle_amd.IcicleError):
        sc.prove([p[: 6 * w] for p in polys[:4]], 0, eq, tcfg)
    del keep


# ---- the large fixtures (tests/golden/sumcheck_vectors_large.json) and the launch figures ------------------------------------------
LARGE = sm.load_large_fixtures()


@pytest.fixture(scope="module")
def large_inputs():
    """the regenerated inputs of every large case, made once"""
    return {c["name"]: sm.large_inputs(c["field"], sm.Program.from_description(c["program"]).nof_inputs, 1 << c["log_n"], c["input_seed"]) for c in LARGE}


def test_large_fixtures_are_the_listed_cases():
    assert [(c["name"], c["field"], c["log_n"], c["input_seed"]) for c in LARGE] == [(name, field, L, seed) for name, field, _, L, seed, _ in sm.LARGE_CASES]
    for c, (_, _, program, _, _, _) in zip(LARGE, sm.LARGE_CASES):
        assert c["program"] == program.description() and c["degree"] == program.degree() and c["labels"] == sm.LARGE_LABELS
        assert len(c["round_polys"]) == c["log_n"] == len(c["challenges"]) and all(len(r) == c["degree"] + 1 for r in c["round_polys"])
    assert os.path.getsize(os.path.join(HERE, "golden", "sumcheck_vectors_large.json")) < 64 * 1024


@pytest.mark.parametrize("case", LARGE, ids=[c["name"] for c in LARGE])
def test_large_generator_reproduces_the_recorded_inputs(case, large_inputs):
    polys = large_inputs[case["name"]]
    p, w = sm.FIELDS[case["field"]]
    assert sm.sha256_of(polys) == case["input_sha256"]
    assert all(a.dtype == np.uint32 and a.shape == ((1 << case["log_n"],) if w == 1 else (1 << case["log_n"], w)) for a in polys)
    assert sm.ints_of_array(polys[0][:1], w) == [0] and sm.ints_of_array(polys[-1][-1:], w) == [p - 1]
    if w == 1:
        assert all(int(a.max()) < p for a in polys)
    else:
        assert all(int(a[:-1, w - 1].max()) < p >> (32 * (w - 1)) for a in polys)  # canonical; the last row of the last one is p - 1


@pytest.mark.parametrize("case", LARGE, ids=[c["name"] for c in LARGE])
def test_large_proofs_pass_the_models_verifier(case):
    field, claimed, hasher, labels, seed = case_args(case)
    p = sm.FIELDS[field][0]
    rps = sm.unhex(case["round_polys"])
    assert sm.verify(field, rps, claimed, hasher, labels, seed)
    assert not sm.verify(field, rps, (claimed + 1) % p, hasher, labels, seed)
    # the recorded challenges are the transcript's
    tr = sm.Transcript(field, hasher, labels, seed, case["log_n"], case["degree"], claimed)
    alphas = [0]
    for r in range(case["log_n"] - 1):
        alphas.append(tr.alpha(r, alphas[-1], rps[r]))
    assert alphas == [int(v, 16) for v in case["challenges"]]


@pytest.mark.parametrize("case", [c for c in LARGE if c["field"] == "babybear"], ids=[c["name"] for c in LARGE if c["field"] == "babybear"])
def test_large_claimed_sums_recomputed_in_64_bits(case, large_inputs):
    """R_0[0] + R_0[1] and the claimed sum against a sum over the regenerated inputs in uint64 arithmetic (p < 2^31)"""
    p = sm.FIELDS["babybear"][0]
    program = sm.Program.from_description(case["program"])
    total = sm.claimed_sum_u64(p, large_inputs[case["name"]], program)
    r0 = sm.unhex(case["round_polys"])[0]
    assert total == int(case["claimed_sum"], 16) and (r0[0] + r0[1]) % p == total


def test_claimed_sum_in_64_bits_equals_the_model():
    p = sm.FIELDS["babybear"][0]
    for _, _, program, _, seed, _ in sm.LARGE_CASES:
        polys = sm.large_inputs("babybear", program.nof_inputs, 64, seed)
        assert sm.claimed_sum_u64(p, polys, program) == sm.claimed_sum("babybear", [sm.ints_of_array(a, 1) for a in polys], program)


def test_launch_info_is_declared_exported_and_bound():
    from icicle_amd import _lib

    text = re.sub(r"\s+", " ", subprocess.check_output(["gcc", "-E", "-P", os.path.join(ROOT, "include", "icicle_hip.h")], text=True))
    m = re.search(r"icicle_error_t icicle_hip_sumcheck_launch_info\s*\(([^)]*)\)\s*;", text)
    assert m and len(m.group(1).split(",")) == 3
    assert "icicle_hip_sumcheck_launch_info" in _lib.API_SYMBOLS and len(_lib.lib.icicle_hip_sumcheck_launch_info.argtypes) == 3
    figures = {}
    for predefined in (0, 1, 2):
        block, grid = ctypes.c_int(), ctypes.c_int()
        assert _lib.lib.icicle_hip_sumcheck_launch_info(predefined, ctypes.byref(block), ctypes.byref(grid)) == 0
        assert block.value >= 64 and block.value % 64 == 0 and grid.value >= 1
        figures[predefined] = (block.value, grid.value)
    assert figures[1] == figures[2] and figures[0][1] == figures[1][1]  # any non-zero value means predefined; one cap for both
    assert _lib.lib.icicle_hip_sumcheck_launch_info(1, None, ctypes.byref(grid)) == INVALID_POINTER
    assert _lib.lib.icicle_hip_sumcheck_launch_info(1, ctypes.byref(block), None) == INVALID_POINTER
    # the large cases are large enough for these figures: more items than a full grid has lanes in the rounds that are to walk
    for c, (_, _, _, _, _, walking) in zip(LARGE, sm.LARGE_CASES):
        predefined = "predefined" in c["program"]
        block, grid = figures[int(predefined)]
        for r in walking:
            assert sm.round_items(c["field"], predefined, c["log_n"], r) > block * grid, (c["name"], r)
