#!/usr/bin/env python3
"""Mint tests/golden/vecops_ext_vectors.json: the twelve extension-field vector operations over babybear, koalabear and goldilocks from
the reference's CPU backend, driven through its own C ABI (<field>_extension_vector_add ... <field>_extension_bit_reverse,
src/vec_ops.cpp) in oracle/_ref/libicicle_field_<field>.so, which oracle/build_ref.sh builds with -DEXT_FIELD=ON.

Only data is recorded, per case: the function, size, batch_size, columns_batch, and the operands and the result as hex of their bytes.
Every vector starts with a directed prefix (0, 1, -1, x, an element with only its top coefficient set, one whose norm involves a
coefficient of p - 1, and, further in, zeros in the middle) in front of seeded random values. Before anything is written the script
confirms on the reference that the inverse of zero is zero and that a / 0 = 0, and records that per field. The tests read only the
JSON (tests/test_vecops_ext_cpu.py holds tests/vecops_ext_model.py against it, tests/test_gpu_vecops_ext.py the device).
"""
import ctypes
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle.ref import REF_DIR, VecOpsConfig  # noqa: E402
from tests import vecops_ext_model as M  # noqa: E402


def directed(f):
    p, d = M.modulus(f), M.DEGREE[f]
    x = (0, 1) + (0,) * (d - 2)
    top = (0,) * (d - 1) + (5,)
    edge = (p - 1,) * d          # every coefficient p - 1: the norm is built from products of p - 1
    edge2 = (1, p - 1) + (0,) * (d - 2)
    return [M.zero(f), M.one(f), M.sub(f, M.zero(f), M.one(f)), x, top, edge, edge2]


def rand_elems(f, rng, n):
    p, d = M.modulus(f), M.DEGREE[f]
    raw = rng.bytes(16 * n * d)
    return [tuple(int.from_bytes(raw[16 * (i * d + c):16 * (i * d + c + 1)], "little") % p for c in range(d)) for i in range(n)]


def vector(f, rng, n, zeros_in_the_middle=True, nonzero=False):
    v = rand_elems(f, rng, n)
    if nonzero:
        return [e if any(e) else M.one(f) for e in v]
    pre = directed(f)
    v[:min(n, len(pre))] = pre[:min(n, len(pre))]
    if zeros_in_the_middle and n >= 12:
        v[n // 2] = v[n // 2 + 1] = M.zero(f)
    return v


def call(lib, f, op, a, b, size, batch, columns, out_elems):
    cfg = VecOpsConfig(None, False, False, False, False, batch, columns, None)
    out = np.zeros((out_elems, 4), np.uint32)
    fn = getattr(lib, f"{f}_extension_{op}")
    if b is not None:
        fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
        err = fn(a.ctypes.data, b.ctypes.data, size, ctypes.byref(cfg), out.ctypes.data)
    else:
        fn.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
        err = fn(a.ctypes.data, size, ctypes.byref(cfg), out.ctypes.data)
    assert err == 0, (f, op, err)
    return out


def case(lib, f, op, a, b, size, batch=1, columns=False):
    """a, b: lists of elements (b of base-field integers for vector_mixed_mul)"""
    aw = M.to_words(f, a)
    bw = None if b is None else (M.base_to_words(f, b) if op == "vector_mixed_mul" else M.to_words(f, b))
    n_out = batch if op in ("vector_sum", "vector_product") else size * batch
    out = call(lib, f, op, aw, bw, size, batch, columns, n_out)
    return {"field": f, "op": op, "size": size, "batch": batch, "columns": columns, "a": aw.tobytes().hex(),
            "b": None if bw is None else bw.tobytes().hex(), "out": out.tobytes().hex()}


def cases_of(lib, f, rng):
    p = M.modulus(f)
    out = []
    for op in ("vector_add", "vector_sub", "vector_mul", "vector_div"):
        for n in (14, 23):
            a, b = vector(f, rng, n)[::-1], vector(f, rng, n)  # reversed: the directed values meet other partners
            out.append(case(lib, f, op, a, b, n))
        a = vector(f, rng, 9)
        out.append(case(lib, f, op, a, a, 9))  # both operands the same: squares, a / a
    for n in (14, 23):
        base = [int.from_bytes(rng.bytes(16), "little") % p for _ in range(n)]
        base[:3] = [0, 1, p - 1]
        out.append(case(lib, f, "vector_mixed_mul", vector(f, rng, n)[::-1], base, n))
    for n in (5, 14, 29):
        out.append(case(lib, f, "vector_inv", vector(f, rng, n), None, n))
    for size, batch, columns in ((7, 1, False), (8, 3, False), (8, 3, True), (13, 3, True)):
        out.append(case(lib, f, "vector_sum", vector(f, rng, size * batch), None, size, batch, columns))
        out.append(case(lib, f, "vector_product", vector(f, rng, size * batch, nonzero=True), None, size, batch, columns))
    out.append(case(lib, f, "vector_product", vector(f, rng, 14), None, 14))  # with zeros: the product is zero
    for op in ("scalar_add_vec", "scalar_sub_vec", "scalar_mul_vec"):
        for size, batch, columns in ((9, 1, False), (8, 3, False), (8, 3, True)):
            out.append(case(lib, f, op, vector(f, rng, batch, nonzero=True), vector(f, rng, size * batch), size, batch, columns))
    for size, batch, columns in ((8, 1, False), (16, 2, False), (8, 3, True)):
        out.append(case(lib, f, "bit_reverse", vector(f, rng, size * batch), None, size, batch, columns))
    return out


def zero_rule(lib, f):
    """the reference's inverse of zero and its a / 0, asked directly"""
    z, a = M.to_words(f, [M.zero(f)]), M.to_words(f, [(3, 1, 4, 1)[:M.DEGREE[f]]])
    inv0 = call(lib, f, "vector_inv", z, None, 1, 1, False, 1)
    div0 = call(lib, f, "vector_div", a, z, 1, 1, False, 1)
    assert not inv0.any() and not div0.any(), (f, inv0, div0)
    return True


def main():
    so = {f: os.path.join(REF_DIR, f"libicicle_field_{f}.so") for f in M.FIELDS}
    missing = [s for s in so.values() if not os.path.exists(s)]
    if missing:
        sys.exit(f"reference libraries not built ({missing[0]}): nothing minted")
    cases, rules = [], {}
    for k, f in enumerate(M.FIELDS):
        lib = ctypes.CDLL(so[f])
        rules[f] = {"inverse_of_zero_is_zero": zero_rule(lib, f)}
        cases += cases_of(lib, f, np.random.default_rng(9100 + k))
        print(f, "ok")
    doc = {"source": "reference CPU backend through its C ABI (tests/golden/mint_vecops_ext_vectors.py)", "rules": rules, "cases": cases}
    out = os.path.join(HERE, "vecops_ext_vectors.json")
    with open(out, "w") as fh:
        json.dump(doc, fh, separators=(",", ":"))
        fh.write("\n")
    print(f"{len(cases)} cases, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
