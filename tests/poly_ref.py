"""What tests/test_poly_model_cpu.py and tests/test_gpu_poly.py share: the eight fields, conversions between integers and element words,
the directed-prefix random values, and ctypes calls of <field>_slice / _highest_non_zero_idx / _poly_eval /
_poly_division of the reference CPU backend (oracle/_ref/libicicle_field_<F>.so). Test infrastructure only.

An ICICLE_ASSERT of the reference throws through its C interface and ends the process, so the callers keep the reference inside the
cases where it is defined (tests/test_poly_model_cpu.py pins the others in a child process):
  * poly_division asserts when deg(numerator) < deg(denominator) - 1 (its q_size check compares an unsigned size with a negative
    number; a zero numerator is the common case) and when the denominator is a constant and the numerator's constant term is not
    zero (it rescans a remainder of size 0);
  * with row batches it copies numerator_size * batch elements into an r_size-strided buffer and rescans the remainder of entry idx at
    r_out + idx * deg_r: defined for batch_size == 1, and for columns_batch with r_size == numerator_size;
  * it leaves q_out above the quotient's degree untouched: the outputs are zero-filled here."""
import ctypes
import functools
import os

import numpy as np

from oracle import pyref

FIELDS = {"babybear": 1, "koalabear": 1, "goldilocks": 2, "bn254": 8, "bls12_381": 8, "bls12_377": 8, "stark252": 8, "grumpkin": 8}  # words
ALL = list(FIELDS)
PER_TYPE = ["babybear", "goldilocks", "bn254", "bls12_377"]  # one field per element type, and bls12_377 for its p ending in ...00000001


def modulus(f):
    """a curve name stands for its scalar field"""
    return pyref.CURVES[f].r if f in pyref.CURVES else pyref.NTT_FIELDS[f].p


def words(vals, w):
    if len(vals) == 0:
        return np.zeros((0, w), np.uint32)
    return np.frombuffer(b"".join(int(v).to_bytes(4 * w, "little") for v in vals), np.uint32).reshape(-1, w).copy()


def ints(arr, w):
    return [int.from_bytes(r.tobytes(), "little") for r in np.ascontiguousarray(arr).reshape(-1, w)]


def rand_vals(rng, n, p, nonzero=False):
    """n uniform values below p behind the directed prefix 0, 1, 2, p-1, (p+1)/2 (without it if nonzero)"""
    raw = rng.bytes(40 * n)
    vals = [int.from_bytes(raw[40 * i:40 * i + 40], "little") % p for i in range(n)]
    if nonzero:
        return [v or 1 for v in vals]
    pre = [0, 1, 2, p - 1, (p + 1) // 2]
    vals[:min(n, len(pre))] = pre[:min(n, len(pre))]
    return vals


def ref_available(f):
    from oracle.ref import REF_DIR

    return os.path.exists(os.path.join(REF_DIR, f"libicicle_field_{f}.so"))


@functools.lru_cache(maxsize=None)
def _ref_lib(f):
    from oracle.ref import REF_DIR

    return ctypes.CDLL(os.path.join(REF_DIR, f"libicicle_field_{f}.so"))


def _cfg(batch, columns):
    from oracle.ref import VecOpsConfig

    return VecOpsConfig(None, False, False, False, False, batch, columns, None)


def ref_slice(f, a, offset, stride, size_in, size_out, batch=1, columns=False):
    w = FIELDS[f]
    a = np.ascontiguousarray(a)
    assert size_out > 0 and offset + (size_out - 1) * stride < size_in and a.size == size_in * batch * w, "the reference would assert"
    out = np.zeros((size_out * batch, w), np.uint32)
    fn = getattr(_ref_lib(f), f"{f}_slice")
    fn.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
    cfg = _cfg(batch, columns)
    assert fn(a.ctypes.data, offset, stride, size_in, size_out, ctypes.byref(cfg), out.ctypes.data) == 0
    return out


def ref_hnz(f, a, size, batch=1, columns=False):
    a = np.ascontiguousarray(a)
    assert size > 0 and a.size == size * batch * FIELDS[f], "the reference would assert"
    out = np.full(batch, -2, np.int64)
    fn = getattr(_ref_lib(f), f"{f}_highest_non_zero_idx")
    fn.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
    cfg = _cfg(batch, columns)
    assert fn(a.ctypes.data, size, ctypes.byref(cfg), out.ctypes.data) == 0
    return out


def ref_eval(f, coeffs, coeffs_size, domain, batch=1, columns=False):
    w = FIELDS[f]
    coeffs, domain = np.ascontiguousarray(coeffs), np.ascontiguousarray(domain)
    m = domain.size // w
    assert coeffs_size > 0 and m > 0 and coeffs.size == coeffs_size * batch * w, "the reference would assert"
    out = np.zeros((m * batch, w), np.uint32)
    fn = getattr(_ref_lib(f), f"{f}_poly_eval")
    fn.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
    cfg = _cfg(batch, columns)
    assert fn(coeffs.ctypes.data, coeffs_size, domain.ctypes.data, m, ctypes.byref(cfg), out.ctypes.data) == 0
    return out


def ref_division_defined(num_vals, den_vals):
    """may the reference be called on this single entry? (the module docstring's first rule)"""
    from tests.poly_model import degree

    dn, db = degree(num_vals), degree(den_vals)
    return db >= 0 and dn >= db - 1 and not (db == 0 and num_vals[0] != 0)


def ref_division(f, num, num_size, den, den_size, q_size, r_size, batch=1, columns=False, guard=True):
    """zero-filled outputs. guard: refuse, in Python, a call the reference would end the process on (off only where a child process pins that)"""
    assert batch == 1 or (columns and r_size == num_size), "the reference is not defined for this batch"
    w = FIELDS[f]
    num, den = np.ascontiguousarray(num), np.ascontiguousarray(den)
    assert num.size == num_size * batch * w and den.size == den_size * batch * w
    for k in range(batch if guard else 0):  # every entry inside the reference's domain of definition, and room for its results
        nk, dk = ints(num.reshape(-1, w)[k::batch][:num_size], w), ints(den.reshape(-1, w)[k::batch][:den_size], w)
        from tests.poly_model import degree

        assert ref_division_defined(nk, dk), "the reference would assert"
        assert r_size >= degree(nk) + 1 and q_size >= degree(nk) - degree(dk) + 1, "the reference would assert"
    q, r = np.zeros((q_size * batch, w), np.uint32), np.zeros((r_size * batch, w), np.uint32)
    fn = getattr(_ref_lib(f), f"{f}_poly_division")
    fn.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64]
    cfg = _cfg(batch, columns)
    assert fn(num.ctypes.data, num_size, den.ctypes.data, den_size, ctypes.byref(cfg), q.ctypes.data, q_size, r.ctypes.data, r_size) == 0
    return q, r
