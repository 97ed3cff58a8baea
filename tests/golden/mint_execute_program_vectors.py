#!/usr/bin/env python3
"""Mint tests/golden/execute_program_vectors.json: execute_program results from the reference's CPU backend, driven through its own
C ABI.

The method of mint_sumcheck_vectors.py: the reference's sources are compiled where they lie, unmodified, into a temporary directory
that is deleted afterwards -- the recipe of oracle/build_ref.sh (device + field library against oracle/shim) cut down to the program,
symbol and vector-operation sources, one library per field. Only data is recorded, per case: a description of the program
(tests/execute_program_model.py VecProgram), the parameters' vectors before the call, and from the reference the vectors of the
parameters it wrote. User programs are built through the reference's symbol ABI from that description. Needs the reference tree
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
sys.path.insert(0, ROOT)
from tests import execute_program_model as em  # noqa: E402

REF = os.path.join(os.environ.get("ICICLE_REFERENCE_DIR", "/root/reference"), "icicle")
FIELD_IDS = {"babybear": (1001, ["-DEXT_FIELD=ON"]), "koalabear": (1004, ["-DEXT_FIELD=ON"]), "bn254": (1, []), "bls12_381": (2, [])}
SOURCES = [
    "src/device_api.cpp", "src/runtime.cpp", "src/config_extension.cpp", "backend/cpu/src/cpu_device_api.cpp",
    "src/fields/ffi_extern.cpp", "src/program/program_c_api.cpp", "src/symbol/symbol_api.cpp",
    "src/vec_ops.cpp", "backend/cpu/src/field/cpu_vec_ops.cpp",
]

V = em.VecProgram
IN = lambda n: [["in", i] for i in range(n)]
AB, EQ = V(4, predefined=em.AB_MINUS_C), V(5, predefined=em.EQ_X_AB_MINUS_C)
# t = x0 + 5 feeds both outputs: x2 = t x1, x3 = 7 t - x1
SHARED = V(4, IN(4) + [["const", 5], ["add", 0, 4], ["mul", 5, 1], ["const", 7], ["mul", 7, 5], ["sub", 8, 1]], [0, 1, 6, 9])
INVERSE = V(3, IN(3) + [["inv", 0], ["mul", 3, 1]], [0, 1, 4])  # x2 = x1 / x0
# x2 = x0 (an input), x3 = x4 = x0 x1 (one node for two parameters): two COPY instructions
COPIES = V(5, IN(5) + [["mul", 0, 1]], [0, 1, 0, 5, 5])
CONST_OUT = V(2, IN(2) + [["const", 9]], [0, 2])  # x1 = 9
IN_OUT = V(2, IN(2) + [["mul", 0, 1], ["add", 2, 0]], [3, 1])  # x0 = x0 x1 + x0
# x0 = x0 + x1; x1 = x0 * 2, in which x0 is the input's node: the reference computes x1 from the new x0
OVERWRITE = V(2, IN(2) + [["add", 0, 1], ["const", 2], ["mul", 0, 3]], [2, 4])
# 40 operations, each consuming the one before: 42 variables in the reference's numbering, three values alive at once
CHAIN = V(3, IN(3) + [[("mul", "add")[k % 2], (0 if k == 0 else 2 + k), 1 - k % 2] for k in range(40)], [0, 1, 42])

# name, field, program, size, batch_size
CASES = []
for _f, _s in (("babybear", "bb"), ("koalabear", "kb"), ("bn254", "bn254"), ("bls12_381", "bls12_381")):
    CASES += [(f"{_s}_ab_1", _f, AB, 1, 1), (f"{_s}_ab_67", _f, AB, 67, 1), (f"{_s}_eq_1", _f, EQ, 1, 1), (f"{_s}_eq_67", _f, EQ, 67, 1),
              (f"{_s}_eq_batch3_size5", _f, EQ, 5, 3), (f"{_s}_shared_9", _f, SHARED, 9, 1), (f"{_s}_inverse_with_zero_7", _f, INVERSE, 7, 1),
              (f"{_s}_copies_5", _f, COPIES, 5, 1), (f"{_s}_const_out_4", _f, CONST_OUT, 4, 1), (f"{_s}_in_out_6", _f, IN_OUT, 6, 1),
              (f"{_s}_overwrite_6", _f, OVERWRITE, 6, 1), (f"{_s}_chain40_5", _f, CHAIN, 5, 1)]


class VecOpsConfig(ctypes.Structure):
    _fields_ = [("stream", ctypes.c_void_p), ("is_a_on_device", ctypes.c_bool), ("is_b_on_device", ctypes.c_bool), ("is_result_on_device", ctypes.c_bool),
                ("is_async", ctypes.c_bool), ("batch_size", ctypes.c_int), ("columns_batch", ctypes.c_bool), ("ext", ctypes.c_void_p)]


def build(field, tmp):
    cxx = os.environ.get("ORACLE_CXX", "/opt/rocm/lib/llvm/bin/clang++")
    if not os.path.exists(cxx):
        cxx = "g++"
    so = os.path.join(tmp, f"libref_program_{field}.so")
    fid, extra = FIELD_IDS[field]
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-fPIC", "-shared", "-pthread", "-w", f"-I{REF}/include", f"-I{REF}/backend/cpu/include",
                           f"-I{os.path.join(ROOT, 'oracle', 'shim')}", f"-DFIELD_ID={fid}", f"-DFIELD={field}", f"-DICICLE_FFI_PREFIX={field}",
                           *extra, *[os.path.join(REF, s) for s in SOURCES], "-ldl", "-o", so])
    return so


def words_of(field, values):
    w = em.FIELDS[field][1]
    return np.array([(int(v) >> (32 * i)) & 0xFFFFFFFF for v in values for i in range(w)], dtype=np.uint32)


def ints_of(field, words):
    w = em.FIELDS[field][1]
    return [sum(int(words[i * w + j]) << (32 * j) for j in range(w)) for i in range(len(words) // w)]


def reference_program(lib, field, program):
    for f in ("create_predefined_program", "create_input_symbol", "create_scalar_symbol"):
        getattr(lib, f"{field}_{f}").restype = ctypes.c_void_p
    if program.predefined is not None:
        return ctypes.c_void_p(getattr(lib, f"{field}_create_predefined_program")(program.predefined))
    handles = []
    for n in program.nodes:
        if n[0] == "in":
            handles.append(ctypes.c_void_p(getattr(lib, f"{field}_create_input_symbol")(n[1])))
        elif n[0] == "const":
            c = words_of(field, [n[1]])
            handles.append(ctypes.c_void_p(getattr(lib, f"{field}_create_scalar_symbol")(c.ctypes.data_as(ctypes.c_void_p))))
        elif n[0] == "inv":
            out = ctypes.c_void_p()
            assert getattr(lib, f"{field}_inverse_symbol")(handles[n[1]], ctypes.byref(out)) == 0
            handles.append(out)
        else:
            out = ctypes.c_void_p()
            fn = {"add": "add_symbols", "sub": "sub_symbols", "mul": "multiply_symbols"}[n[0]]
            assert getattr(lib, f"{field}_{fn}")(handles[n[1]], handles[n[2]], ctypes.byref(out)) == 0
            handles.append(out)
    params = (ctypes.c_void_p * program.nof_parameters)(*[handles[j].value for j in program.params])
    prog = ctypes.c_void_p()
    assert getattr(lib, f"{field}_generate_program")(params, program.nof_parameters, ctypes.byref(prog)) == 0
    return prog


def run_case(lib, case, index):
    name, field, program, size, batch = case
    p, w = em.FIELDS[field]
    n, m = size * batch, program.nof_parameters
    rng = np.random.default_rng(3000 + index)
    data = [[int.from_bytes(rng.bytes(40), "little") % p for _ in range(n)] for _ in range(m)]
    special = [0, 1, p - 1]
    for j in range(m):  # 0, 1 and p - 1 among the values, at different places per parameter
        for k, v in enumerate(special):
            if n > (j + 2 * k) % max(n, 1) and n >= 3:
                data[j][(j + 2 * k) % n] = v
    if n == 1:
        data[0][0], data[-2][0] = p - 1, 1
    if "inverse" in name:
        data[0][2] = 0
    prog = reference_program(lib, field, program)
    arrays = [words_of(field, d) for d in data]
    table = (ctypes.c_void_p * m)(*[a.ctypes.data for a in arrays])
    cfg = VecOpsConfig(None, False, False, False, False, batch, False, None)
    assert getattr(lib, f"{field}_execute_program")(table, ctypes.c_uint64(m), prog, ctypes.c_uint64(size), ctypes.byref(cfg)) == 0, name
    lib.delete_program(prog)
    after = [ints_of(field, a) for a in arrays]
    written = program.written()
    for j in range(m):
        assert j in written or after[j] == data[j], (name, j)
    hexes = lambda row: [f"{v:x}" for v in row]
    return {"name": name, "field": field, "size": size, "batch_size": batch, "program": program.description(), "data": [hexes(d) for d in data],
            "written": {str(j): hexes(after[j]) for j in written}}


def main():
    if not os.path.isdir(REF):
        sys.exit(f"reference tree not found ({REF}): nothing minted")
    cases = []
    with tempfile.TemporaryDirectory() as tmp:
        for field in FIELD_IDS:
            lib = ctypes.CDLL(build(field, tmp))
            for i, case in enumerate(CASES):
                if case[1] == field:
                    cases.append(run_case(lib, case, i))
                    print(case[0], "ok")
            del lib
    doc = {"source": "reference CPU backend through its C ABI (tests/golden/mint_execute_program_vectors.py)", "cases": cases}
    out = os.path.join(HERE, "execute_program_vectors.json")
    with open(out, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print(f"{len(cases)} cases, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
