"""CPU: execute_program without a GPU -- the Python model (tests/execute_program_model.py) against every fixture of the reference
(tests/golden/execute_program_vectors.json), the host-only compiler and lowering (icicle_amd/csrc/program_plan.h in its general
mode and program_lower.h through tests/execute_program_host_harness.cpp, built with g++ plainly and with -fsanitize=address,undefined
as a program of its own) against the model on the fixtures' programs and on seeded random graphs, and the C ABI's surface: header,
library and binding agree, and every argument error is returned before the device is touched."""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest

from tests import execute_program_model as em

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INVALID_POINTER, INVALID_ARGUMENT = 3, 11
FIELDS = ["babybear", "koalabear", "bn254", "bls12_381"]
CASES = em.load_fixtures()


def user_programs(field):
    return {c["name"]: em.VecProgram.from_description(c["program"]) for c in CASES if c["field"] == field and "predefined" not in c["program"]}


# ---- the model against the reference's results -----------------------------------------------------------------------------------------
def test_fixtures_cover_what_the_issue_lists():
    assert {c["field"] for c in CASES} == set(FIELDS)
    assert os.path.getsize(os.path.join(HERE, "golden", "execute_program_vectors.json")) < 256 * 1024
    for f in FIELDS:
        p = em.FIELDS[f][0]
        mine = [c for c in CASES if c["field"] == f]
        assert max(c["size"] * c["batch_size"] for c in mine) <= 67
        for pid in (0, 1):
            assert {c["size"] for c in mine if c["program"].get("predefined") == pid and c["batch_size"] == 1} >= {1, 67}
        assert any(c["batch_size"] == 3 and c["size"] == 5 for c in mine)
        values = {int(v, 16) for c in mine for d in c["data"] for v in d}
        assert {0, 1, p - 1} <= values
        progs = user_programs(f)
        compiled = {n: g.compile() for n, g in progs.items()}
        assert any(len(g.written()) == 2 and len(consts) == 2 for (n, g), (_, consts, _) in zip(progs.items(), compiled.values()))  # two outputs, two constants
        inverse = [c for c in mine if any(n[0] == "inv" for n in c["program"].get("nodes", []))]
        assert inverse and all(0 in [int(v, 16) for v in c["data"][0]] for c in inverse)
        assert any(sum(i[0] == em.COPY for i in ins) >= 2 for ins, _, _ in compiled.values())          # an input as output, one node twice
        assert any(any(i[0] == em.COPY and i[1] >= g.nof_parameters for i in ins) for g, (ins, _, _) in zip(progs.values(), compiled.values()))  # a constant
        assert any(set(g.written()) & {i[1] for i in ins if i[0] != em.COPY} for g, (ins, _, _) in zip(progs.values(), compiled.values()))  # in / out
        long = [g for g in progs.values() if len(g.compile()[0]) >= 40]
        assert long and all(g.nof_vars() > 20 and em.lower(g, 24)[1] <= 4 for g in long)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_model_equals_the_reference(case):
    program = em.VecProgram.from_description(case["program"])
    data = em.unhex(case["data"])
    got = em.execute(case["field"], program, data)
    assert sorted(int(j) for j in case["written"]) == program.written()
    for j in range(program.nof_parameters):
        want = [int(v, 16) for v in case["written"][str(j)]] if str(j) in case["written"] else data[j]
        assert got[j] == want, j


def test_overwrite_case_sees_the_new_value():
    """x0 = x0 + x1; x1 = x0 * 2: the reference doubles the new x0, not the one the call began with"""
    case = next(c for c in CASES if c["name"] == "bb_overwrite_6")
    p = em.FIELDS["babybear"][0]
    x0, x1 = em.unhex(case["data"])
    assert [int(v, 16) for v in case["written"]["1"]] == [2 * (a + b) % p for a, b in zip(x0, x1)]
    assert any(2 * (a + b) % p != 2 * a % p for a, b in zip(x0, x1))


# ---- program_plan.h and program_lower.h on the host ----------------------------------------------------------------------------------
def build_harness(name, flags):
    exe = os.path.join(HERE, "_build", name)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    src = os.path.join(HERE, "execute_program_host_harness.cpp")
    deps = [src] + [os.path.join(ROOT, "icicle_amd", "csrc", h) for h in ("program_lower.h", "sumcheck_plan.h", "program_plan.h", "field_consts.h")]
    if not os.path.exists(exe) or max(os.path.getmtime(d) for d in deps) > os.path.getmtime(exe):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", *flags, src, "-o", exe])
    return exe


def el(field, v):
    return int(v).to_bytes(4 * em.FIELDS[field][1], "little").hex()


def node_spec(field, program):
    return ",".join(f"const:{el(field, n[1])}" if n[0] == "const" else ":".join(str(v) for v in n) for n in program.nodes)


def show_list(code):
    return ",".join(":".join(str(v) for v in i) for i in code) or "-"


def random_program(rng, p):
    """a graph of up to 40 nodes over up to 6 parameters; every parameter is bound to a random node"""
    np_ = rng.randrange(1, 7)
    nodes = [["in", i] for i in range(np_)]
    for _ in range(rng.randrange(0, 35)):
        kind = rng.choice(["add", "sub", "mul", "mul", "inv", "const", "in"])
        if kind == "const":
            nodes.append(["const", rng.choice([0, 1, p - 1, rng.randrange(p)])])
        elif kind == "in":
            nodes.append(["in", rng.randrange(np_)])
        elif kind == "inv":
            nodes.append(["inv", rng.randrange(len(nodes))])
        else:
            nodes.append([kind, rng.randrange(len(nodes)), rng.randrange(len(nodes))])
    params = [rng.choice([i, rng.randrange(len(nodes)), len(nodes) - 1]) for i in range(np_)]
    return em.VecProgram(np_, nodes, params)


def wide_program(k):
    """a_1 = x0 x1, a_j = a_{j-1} x1, x2 = (..(a_k + a_{k-1}) + ..) + a_1: all k products are alive before the first sum"""
    nodes = [["in", 0], ["in", 1], ["in", 2]] + [["mul", 0 if j == 0 else 2 + j, 1] for j in range(k)]
    acc = 2 + k
    for j in range(k - 1, 0, -1):
        nodes.append(["add", acc, 2 + j])
        acc = len(nodes) - 1
    return em.VecProgram(3, nodes, [0, 1, acc])


def expected_answer(field, program, cap, x):
    p, w = em.FIELDS[field]
    ins, consts, inter = program.compile()
    if program.nof_parameters + len(consts) + inter > 255:
        return "refused"
    low = em.lower(program, cap)
    if low is None:
        return "overcap"
    code, peak, use = low
    assert peak <= cap
    after = em.run_lowered(p, code, consts, x, peak)
    assert after == program.evaluate(p, x)  # the lowered list computes what the reference's list computes
    mont = ",".join(el(field, (c % p << em.MONT_BITS[w]) % p) for c in consts) or "-"
    return (f"{program.nof_vars()} {show_list(ins)} {peak} {','.join(str(u) for u in use)} {show_list(code)} {mont} "
            + ",".join(el(field, v) for v in after))


def harness_script():
    rng = random.Random(23)
    cmds, want = [], []
    for field in FIELDS:
        p, w = em.FIELDS[field]
        cap = em.CAPS[w]
        programs = [(g, cap) for g in user_programs(field).values()]
        programs += [(random_program(rng, p), rng.choice([2, 3, 5, 8, cap])) for _ in range(60 if w == 1 else 25)]
        k = next(k for k in range(2, 80) if em.lower(wide_program(k), cap)[1] == cap)  # exactly at the cap, and one value more
        programs += [(wide_program(k), cap), (wide_program(k + 1), cap)]
        many = em.VecProgram(2, [["in", 0], ["in", 1]] + [["const", c + 1] for c in range(cap + 1)]
                             + [["add", 0 if c == 0 else cap + 2 + c, 2 + c] for c in range(cap + 1)], [0, 2 * cap + 3])  # more constants than slots
        programs.append((many, cap))
        for g, c in programs:
            x = [rng.choice([0, 1, p - 1, rng.randrange(p)]) for _ in range(g.nof_parameters)]
            cmds.append(f"lower {field} {c} {g.nof_parameters} {node_spec(field, g)} {','.join(str(j) for j in g.params)} " + " ".join(el(field, v) for v in x))
            want.append(expected_answer(field, g, c, x))
        assert want[-2] == "overcap" and want[-1] == "overcap" and want[-3] not in ("overcap", "refused")
        cmds += [f"predefined {field} 0", f"predefined {field} 1", f"predefined {field} 2", f"lower {field} {cap} 1 in:1 0"]
        want += ["4 1,1,1,2", "5 1,1,1,1,2", "refused", "refused"]  # an input index outside the parameters
    return cmds, want


@pytest.fixture(scope="module")
def script():
    return harness_script()


def run_harness(exe, cmds):
    r = subprocess.run([exe], input="\n".join(cmds) + "\n", capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    return r.stdout.splitlines()


def test_script_has_programs_on_both_sides_of_the_cap(script):
    _, want = script
    assert sum(w == "overcap" for w in want) >= 12 and sum(w not in ("overcap", "refused") and " " in w for w in want) >= 100


def test_host_code_matches_the_model(script):
    cmds, want = script
    got = run_harness(build_harness("execute_program_host_harness", []), cmds)
    assert len(got) == len(want)
    for c, g, w in zip(cmds, got, want):
        assert g == w, c[:300]


def test_host_code_under_address_and_undefined_behaviour_sanitizers(script):
    """the same program, instrumented: a finding makes it exit non-zero with a report on stderr"""
    cmds, want = script
    exe = build_harness("execute_program_host_harness_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan"])
    assert run_harness(exe, cmds) == want


# ---- header, library, binding ------------------------------------------------------------------------------------------------------
def test_functions_are_declared_exported_and_bound():
    from icicle_amd import _lib
    import icicle_amd

    text = re.sub(r"\s+", " ", subprocess.check_output(["gcc", "-E", "-P", os.path.join(ROOT, "include", "icicle_hip.h")], text=True))
    assert _lib.PROGRAM_FUNCTIONS == ["generate_program", "execute_program"]
    for p in FIELDS:
        for name, n in (("generate_program", 3), ("execute_program", 5)):
            m = re.search(r"icicle_error_t %s_%s\s*\(([^)]*)\)\s*;" % (p, name), text)
            assert m and len(m.group(1).split(",")) == n, (p, name)
            assert f"{p}_{name}" in _lib.API_SYMBOLS and len(getattr(_lib.lib, f"{p}_{name}").argtypes) == n
        assert re.search(r"icicle_program_handle_t %s_create_predefined_program\s*\(\s*int pre_def\s*\)\s*;" % p, text)
        fn = getattr(_lib.lib, f"{p}_create_predefined_program")
        assert fn.restype is ctypes.c_void_p and len(fn.argtypes) == 1 and f"{p}_create_predefined_program" in _lib.PROGRAM_HANDLE_SYMBOLS
    # what stays unbuilt: the extension_ and rns_ variants, the fields without the symbol functions, the plugin
    for absent in ("extension_execute_program", "rns_execute_program", "extension_generate_program", "goldilocks_execute_program", "stark252_execute_program",
                   "bls12_377_execute_program", "grumpkin_execute_program"):
        assert absent not in text and not hasattr(_lib.lib, absent) and not hasattr(_lib.lib, "babybear_" + absent), absent
    assert not re.search(r"execute_program", open(os.path.join(ROOT, "plugin", "hip_c_api.h")).read())
    for name in ("Program", "execute_program", "program"):
        assert hasattr(icicle_amd, name), name
    assert icicle_amd.vecops.execute_program is icicle_amd.execute_program


# ---- argument errors, with or without a device ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", FIELDS)
def test_argument_errors_need_no_gpu(field):
    from icicle_amd import Program, ReturningValueProgram, VecOpsConfig, runtime
    from icicle_amd._lib import lib

    w = em.FIELDS[field][1]
    cap = em.CAPS[w]
    run_c = getattr(lib, field + "_execute_program")
    vectors = [np.zeros(4 * w, dtype=np.uint32) for _ in range(6)]

    def run(program, m, size=4, null_at=None, with_cfg=True, table=True):
        cfg = VecOpsConfig.default()
        ptrs = (ctypes.c_void_p * 6)(*[None if j == null_at else v.ctypes.data for j, v in enumerate(vectors)])
        return run_c(ptrs if table else None, m, program.handle if program else None, size, ctypes.byref(cfg) if with_cfg else None)

    eq, ab = Program.predefined(field, 1), Program.predefined(field, 0)
    assert eq.nof_parameters == 5 and ab.nof_parameters == 4
    with pytest.raises(ValueError):
        Program.predefined(field, 2)
    # a well-formed call gets past every check: it succeeds on a GPU and ends in a device error, never an argument error, without one
    rc = run(eq, 5)
    if runtime.get_device_count() > 0:
        assert rc == 0
    else:
        assert rc not in (0, INVALID_ARGUMENT, INVALID_POINTER)
    assert run(eq, 4) == INVALID_ARGUMENT and run(eq, 6) == INVALID_ARGUMENT and run(ab, 5) == INVALID_ARGUMENT and run(ab, 0) == INVALID_ARGUMENT
    assert run(None, 5) == INVALID_POINTER
    for j in range(5):
        assert run(eq, 5, null_at=j) == INVALID_POINTER, j
    assert run(eq, 5, with_cfg=False) == INVALID_POINTER and run(eq, 5, table=False) == INVALID_POINTER
    other = Program.predefined("bn254" if w == 1 else "babybear", 1)
    assert run(other, 5) == INVALID_ARGUMENT  # a program of a field with another element size
    assert run(eq, 5, size=0) == 0 and run(ab, 4, size=0) == 0  # nothing to do, nothing launched
    # a ReturningValueProgram handle is a program as well
    assert run(ReturningValueProgram.predefined(field, 1), 5, size=0) == 0 and run(ReturningValueProgram.predefined(field, 1), 4, size=0) == INVALID_ARGUMENT

    def wide(k):  # tests/test_execute_program_cpu.py wide_program, through the symbols
        def fn(x):
            a = [x[0] * x[1]]
            for _ in range(k - 1):
                a.append(a[-1] * x[1])
            acc = a[-1]
            for t in reversed(a[:-1]):
                acc = acc + t
            x[2] = acc
        return fn

    k = next(k for k in range(2, 80) if em.lower(wide_program(k), cap)[1] == cap)
    at_cap, over_cap = Program.from_function(field, wide(k), 3), Program.from_function(field, wide(k + 1), 3)
    assert run(at_cap, 3, size=0) == 0 and run(over_cap, 3, size=0) == INVALID_ARGUMENT and run(over_cap, 3) == INVALID_ARGUMENT
    # a long program with few values alive is no argument error
    chain = user_programs(field)[[n for n in user_programs(field) if "chain40" in n][0]]
    assert chain.nof_vars() > 24 and em.lower(chain, cap) is not None

    def chain_fn(x):
        acc = x[0]
        for j in range(40):
            acc = acc * x[1] if j % 2 == 0 else acc + x[0]
        x[2] = acc

    assert run(Program.from_function(field, chain_fn, 3), 3, size=0) == 0
    # generate_program's own errors
    gen = getattr(lib, field + "_generate_program")
    out = ctypes.c_void_p()
    assert gen(None, 1, ctypes.byref(out)) == INVALID_POINTER
    one = (ctypes.c_void_p * 1)(None)
    assert gen(one, 1, ctypes.byref(out)) == INVALID_ARGUMENT and gen(one, 0, ctypes.byref(out)) == INVALID_ARGUMENT
    with pytest.raises(Exception):
        Program.from_function(field, lambda x: x.__setitem__(0, x[0].__class__.input(field, 5)), 2)  # an input index outside the parameters
