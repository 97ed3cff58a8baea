"""Operand tuples and integer expectations for the element-wise arithmetic tests, shared by the host leg (tests/test_host_math.py,
libhost_math.so with the bound tracker) and the device leg (tests/test_gpu_device_math.py, the two builds of
tests/device_math_harness.hip). A backend is anything with canon / raw / small / ec methods that runs the case bodies of
tests/math_cases.hpp on arrays; every expected value here is computed with Python integers (oracle/pyref.py for Fq2 and the curves).

Which tuples an op sees:
  * two-operand ops: ALL directed pairs (directed_operands.directed_pairs) and the seeded random pairs;
  * four-operand ops: the same (a, b), with (c, d) a seeded permutation of the same pair list;
  * one-operand ops (sqr, neg, inv, dbl, conversions, is_zero, the aliased products): every distinct directed value and the first
    operands of the random pairs -- a pair adds nothing to an op that reads one operand.
Fq2 has its own directed element list (canon_operands): every directed base-field value in one component against the named values in
the other, both ways round; all pairs of base-field values are the base field's own test.
Raw mode: the representatives a0 + j*p of directed_operands.raw_seeds; one-operand ops see every j in 0..K-1, products and sums
see j in {0, 1, K-1} of a subset of the seeds, for every admissible combination of stated bounds.
EC tier: sequences of affine points, one per thread (ec_plan). Quad tier (device only): the four-lane operations, one sequence per DPP quad
(quad_plan), every lane's words, every position in the wave, the one-lane twins, raw operands up to the headers' stated bounds."""
import ctypes
import functools
import os
import random
import signal
import subprocess
import sys
import tempfile

import numpy as np

from oracle import pyref
from tests import directed_operands as D

RB = D.RB
# field id -> (name, modulus, 29-bit limbs, 32-bit words); ids as in math_cases.hpp with_field
BIG = {0: ("bn254_fq", pyref.BN254.q, 9, 8), 1: ("bn254_fr", pyref.BN254.r, 9, 8), 2: ("bls12_381_fq", pyref.BLS12_381.q, 14, 12),
       3: ("bls12_381_fr", pyref.BLS12_381.r, 9, 8), 4: ("bls12_377_fq", pyref.BLS12_377.q, 14, 12), 5: ("bls12_377_fr", pyref.BLS12_377.r, 9, 8),
       6: ("stark252_fr", pyref.STARK252.p, 9, 8)}
GOLD = 7
FQ2 = {8: 0, 9: 2, 10: 4}  # Fq2 id -> base field id
FIELD_NAME = {**{k: v[0] for k, v in BIG.items()}, 7: "goldilocks", 8: "bn254_fq2", 9: "bls12_381_fq2", 10: "bls12_377_fq2"}
SMALL = {0: pyref.BABYBEAR, 1: pyref.KOALABEAR}
TAG_ASM, TAG_NOASM = 0x41534D31, 0x4E4F4153

_u32p = ctypes.POINTER(ctypes.c_uint32)
_i32p = ctypes.POINTER(ctypes.c_int)


def _p(a, t=_u32p):
    return a.ctypes.data_as(t)


class Backend:
    """host: libhost_math.so (host_* entry points, no tag); device: a libdevice_math_*.so (dm_* entry points, tag checked on every call)"""

    def __init__(self, lib, device, tag=None, name="host"):
        self.lib, self.device, self.tag, self.name = lib, device, tag, name
        self.tags_seen = 0
        if device:
            lib.dm_variant_tag.restype = ctypes.c_uint32
            assert lib.dm_variant_tag() == tag, (name, hex(lib.dm_variant_tag()))

    def _call(self, fn, *args):
        if not self.device:
            rc = getattr(self.lib, "host_" + fn)(*args)
            assert rc == 0, (self.name, fn, rc)
            return
        tag = np.zeros(1, dtype=np.uint32)
        rc = getattr(self.lib, "dm_" + fn)(*args, _p(tag))
        assert rc == 0, (self.name, fn, "HIP error / bad op", rc)
        assert int(tag[0]) == self.tag, f"{self.name}: kernel wrote variant tag {int(tag[0]):#x}, expected {self.tag:#x}"
        self.tags_seen += 1

    def canon(self, field, op, a, b, c, d):
        out = np.zeros_like(a)
        self._call("field_canon", field, op, a.shape[0], _p(a), _p(b), _p(c), _p(d), _p(out))
        return out

    def raw(self, field, op, K, kb, a, b, c, d):
        out = np.zeros_like(a)
        kba = np.array(kb, dtype=np.int32)
        self._call("field_raw", field, op, K, _p(kba, _i32p), a.shape[0], _p(a), _p(b), _p(c), _p(d), _p(out))
        return out

    def small(self, field, op, a, b):
        out = np.zeros_like(a)
        self._call("small_batch" if not self.device else "small", field, op, a.shape[0], _p(a), _p(b), _p(out))
        return out

    def ec(self, curve, op, pts, offs, aux, out_words):
        out = np.zeros((len(offs) - 1, out_words), dtype=np.uint32)
        self._call("ec_batch" if not self.device else "ec", curve, op, len(offs) - 1, _p(pts), _p(offs, _i32p), _p(aux), _p(out))
        return out

    def ec_quad(self, curve, op, pts, offs, aux, out_words):
        """device only: one sequence per DPP quad; out[s, role] = the words lane `role` of the quad stored"""
        out = np.zeros((len(offs) - 1, 4, out_words), dtype=np.uint32)
        self._call("ec_quad", curve, op, len(offs) - 1, _p(pts), _p(offs, _i32p), _p(aux), _p(out))
        return out

    def refuses(self, fn, curve, op, npts=1):
        """the entry point answers -1 (nothing launched) for a (curve, op) pair it does not have; one well-formed sequence of npts points"""
        z, o = np.zeros(1024, dtype=np.uint32), np.array([0, npts], dtype=np.int32)
        args = (curve, op, 1, _p(z), _p(o, _i32p), _p(z), _p(np.zeros(1024, dtype=np.uint32)))
        if not self.device:
            return getattr(self.lib, "host_" + fn)(*args) == -1
        return getattr(self.lib, "dm_" + fn)(*args, _p(np.zeros(1, dtype=np.uint32))) == -1


def words(vals, W):
    return np.frombuffer(b"".join(v.to_bytes(4 * W, "little") for v in vals), dtype=np.uint32).reshape(len(vals), W).copy()


def limb_rows(vals, NL):
    """values below 2^(29*NL) -> rows of NL normalised 29-bit limbs (vectorised: the words of each value, re-cut at 29 bits)"""
    W = (RB * NL + 31) // 32 + 1
    w = words(vals, W).astype(np.uint64)
    out = np.empty((len(vals), NL), dtype=np.uint32)
    for i in range(NL):
        word, sh = (RB * i) // 32, (RB * i) % 32
        out[:, i] = (((w[:, word] | (w[:, word + 1] << np.uint64(32))) >> np.uint64(sh)) & np.uint64((1 << RB) - 1)).astype(np.uint32)
    return out


def row_ints(arr, bits):
    """rows of little-endian `bits`-bit digits -> Python integers"""
    cols = [[int(x) for x in arr[:, i]] for i in range(arr.shape[1])]
    return [sum(c[r] << (bits * i) for i, c in enumerate(cols)) for r in range(arr.shape[0])]


# ---- algebras: how one element is encoded and computed with integers ---------------------------------------------------------
class Fp:
    def __init__(self, p, W, mont_bits):
        self.p, self.W, self.ew = p, W, W
        self.R = pow(2, mont_bits, p)      # the device's Montgomery radix (1 for goldilocks: elements are canonical)
        self.R32 = pow(2, 32 * W, p)       # the reference's Montgomery radix

    def elems(self, pairs):
        return [a for a, _ in pairs], [b for _, b in pairs]

    def enc(self, vals):
        return words(vals, self.W)

    add = lambda s, a, b: (a + b) % s.p
    sub = lambda s, a, b: (a - b) % s.p
    mul = lambda s, a, b: a * b % s.p
    scal = lambda s, a, k: a * k % s.p
    inv = lambda s, a: pow(a, -1, s.p) if a else 0
    iszero = lambda s, a: a == 0


class Fp2:
    def __init__(self, base: Fp):
        self.b, self.p, self.W, self.ew = base, base.p, 2 * base.W, base.W
        self.R, self.R32 = base.R, base.R32

    def enc(self, vals):
        return words([v for e in vals for v in e], self.ew).reshape(len(vals), self.W)

    add = lambda s, a, b: pyref.f2_add(s.p, a, b)
    sub = lambda s, a, b: pyref.f2_sub(s.p, a, b)
    mul = lambda s, a, b: pyref.f2_mul(s.p, a, b)
    scal = lambda s, a, k: (a[0] * k % s.p, a[1] * k % s.p)
    inv = lambda s, a: pyref.f2_inv(s.p, a) if a != (0, 0) else (0, 0)
    iszero = lambda s, a: a == (0, 0)


def algebra(fid):
    if fid in BIG:
        _, p, NL, NL32 = BIG[fid]
        return Fp(p, NL32, RB * NL)
    if fid == GOLD:
        return Fp(D.GOLD_P, 2, 0)
    _, p, NL, NL32 = BIG[FQ2[fid]]
    return Fp2(Fp(p, NL32, RB * NL))


@functools.lru_cache(maxsize=None)
def canon_operands(fid):
    """(directed count, pair tuples (x, y, z, w), single tuples): elements as the algebra's values"""
    rnd = random.Random(1000 + fid)
    if fid in BIG:
        _, p, NL, NL32 = BIG[fid]
        dp, rp = D.directed_pairs(p, NL, NL32, fid)
        singles = D.directed_values(p, NL, NL32) + [a for a, _ in rp]
    elif fid == GOLD:
        dp, rp = D.gold_pairs()
        singles = D.gold_values() + [a for a, _ in rp]
    else:  # Fq2: an element is a base-field pair. Directed elements: every directed value of the base field in one component against each of
        # the named values (0, 1, 2, 3, p-1, p-2, p-3, (p+-1)/2, R, R^2, -R, R^-1, plain and in the Montgomery domain) in the other, both
        # ways round -- so each component meets every limb pattern, and the products' cross terms (two base-field mul_add, which see ALL
        # base pairs in the base field's own test) meet the values that make them vanish or wrap. y is a seeded permutation of the same
        # list; then x against itself, -x and its conjugate.
        _, p, NL, NL32 = BIG[FQ2[fid]]
        V = D.directed_values(p, NL, NL32)
        Rinv = pow(1 << (RB * NL), -1, p)
        named = list(dict.fromkeys(V[:13] + [v * Rinv % p for v in V[:13]]))
        E = [(u, k) for u in V for k in named] + [(k, u) for u in V for k in named]
        perm = rnd.sample(range(len(E)), len(E))
        dp = [(E[i], E[perm[i]]) for i in range(len(E))]
        for x in D.relation_pairs(V, p):
            dp += [(x, x), (x, ((-x[0]) % p, (-x[1]) % p)), (x, (x[0], (-x[1]) % p))]
        br = D.random_pairs(p, 2 * D.RANDOM_PAIRS, fid)
        rp = [(br[2 * i], br[2 * i + 1]) for i in range(D.RANDOM_PAIRS)]
        singles = E[::7] + [(v, 0) for v in V] + [(0, v) for v in V] + [x for x, _ in rp[:500]]
    pairs = dp + rp
    perm = rnd.sample(range(len(pairs)), len(pairs))
    quads = [(pairs[i][0], pairs[i][1], pairs[perm[i]][0], pairs[perm[i]][1]) for i in range(len(pairs))]
    return len(dp), quads, [(s, s, s, s) for s in singles]


# op -> (name, arity, expected(A, x, y, z, w)); arity 1 runs on the singles, 2 and 4 on all pairs. flag ops give 0 / 1.
def _ops(A):
    R, R32, p = A.R, A.R32, A.p
    R32i = pow(R32, -1, p)
    return {
        0: ("mul", 2, lambda x, y, z, w: A.mul(x, y)),
        1: ("sqr", 1, lambda x, y, z, w: A.mul(x, x)),
        2: ("add", 2, lambda x, y, z, w: A.add(x, y)),
        3: ("sub<2>", 2, lambda x, y, z, w: A.sub(x, y)),
        4: ("neg<2>", 1, lambda x, y, z, w: A.sub(A.sub(x, x), x)),
        5: ("lazy 2(x+y)(x-4y)", 2, lambda x, y, z, w: A.mul(A.scal(A.add(x, y), 2), A.sub(x, A.scal(y, 4)))),
        6: ("from_refmont", 1, lambda x, y, z, w: A.scal(x, R32i)),
        7: ("to_refmont", 1, lambda x, y, z, w: A.scal(x, R32)),
        8: ("is_zero(x-y)", 2, lambda x, y, z, w: x == y),
        9: ("inv", 1, lambda x, y, z, w: A.inv(x)),
        10: ("mul_add", 4, lambda x, y, z, w: A.add(A.mul(x, y), A.mul(z, w))),
        11: ("mul_inplace", 2, lambda x, y, z, w: A.mul(x, y)),
        12: ("mul_inplace(a,a)", 1, lambda x, y, z, w: A.mul(x, x)),
        13: ("mul_add_inplace_c", 4, lambda x, y, z, w: A.add(A.mul(x, y), A.mul(z, w))),
        14: ("mul_add_inplace_c(c,c,b,d)", 4, lambda x, y, z, w: A.add(A.mul(z, y), A.mul(z, w))),
        15: ("dbl", 1, lambda x, y, z, w: A.add(x, x)),
        16: ("select(true)", 2, lambda x, y, z, w: x),
        17: ("select(false)", 2, lambda x, y, z, w: y),
        18: ("eq", 2, lambda x, y, z, w: x == y),
        19: ("is_zero", 1, lambda x, y, z, w: A.iszero(x)),
        20: ("mul_add_inplace_c(c,a,c,c)", 4, lambda x, y, z, w: A.add(A.mul(x, z), A.mul(z, z))),
        21: ("mul_inplace(a,R^2)", 1, lambda x, y, z, w: A.scal(x, R)),
    }


FLAG_OPS = (8, 18, 19)
GOLD_MISSING = (10, 11, 12, 13, 14, 20, 21)  # goldilocks' FieldOps has no mul_add and no in-place products
HOST_SKIPS_INV_ABOVE = 400  # the host build (-O1, tracker on) inverts only this many elements per field; the device all of them


def _hex(e):
    return "(" + ", ".join(hex(v) for v in e) + ")" if isinstance(e, tuple) else hex(e)


_EXPECTED = {}
_SAME_AS = {11: 0, 13: 10, 18: 8, 12: 1}  # mul_inplace = mul, mul_add_inplace_c = mul_add, eq = is_zero(x - y), mul_inplace(a, a) = sqr


def check_canon(be: Backend, fid, ops=None):
    """every op of the field on every tuple, exact; returns the number of (op, tuple) comparisons"""
    A = algebra(fid)
    ndir, quads, singles = canon_operands(fid)
    table = _ops(A)
    compared = 0
    for arity_set, tuples in (((2, 4), quads), ((1,), singles)):
        cols = [A.enc([t[i] for t in tuples]) for i in range(4)]
        for op, (name, arity, fn) in table.items():
            if arity not in arity_set or (ops is not None and op not in ops) or (fid == GOLD and op in GOLD_MISSING):
                continue
            sel = slice(None)
            if op == 9 and not be.device:
                sel = slice(0, HOST_SKIPS_INV_ABOVE)
            tl = tuples[sel]
            got = be.canon(fid, op, *[np.ascontiguousarray(c[sel]) for c in cols])
            key = (fid, _SAME_AS.get(op, op), len(tl))  # (ops with the same definition share one expectation)
            if key not in _EXPECTED and op in (16, 17):  # select: the operand itself
                _EXPECTED[key] = np.ascontiguousarray(cols[op - 16][sel])
            if key not in _EXPECTED:  # (the second build of the device harness meets the same expectations: computed once per field)
                if any(k[0] != fid for k in _EXPECTED):
                    _EXPECTED.clear()
                exp_vals = [fn(*t) for t in tl]
                if op in FLAG_OPS:
                    exp = np.zeros_like(got)
                    exp[:, 0] = np.array(exp_vals, dtype=np.uint32)
                else:
                    exp = A.enc(exp_vals)
                _EXPECTED[key] = exp
            exp = _EXPECTED[key]
            if not np.array_equal(got, exp):
                bad = np.nonzero((got != exp).any(axis=1))[0]
                lines = [f"  x={_hex(tl[i][0])} y={_hex(tl[i][1])} z={_hex(tl[i][2])} w={_hex(tl[i][3])}\n    got {[hex(int(v)) for v in got[i]]}\n    exp {[hex(int(v)) for v in exp[i]]}"
                         for i in bad[:4]]
                raise AssertionError(f"{FIELD_NAME[fid]} op {op} ({name}) variant {be.name}: {len(bad)} of {len(tl)} tuples differ from the integers; first:\n" + "\n".join(lines))
            compared += len(tl)
    return compared


def check_gold_noncanonical(be: Backend):
    """goldilocks' unpack brings a word pair in [p, 2^64) below p ("v >= P"): only a non-canonical input reaches that branch"""
    p = D.GOLD_P
    vals = D.gold_values()
    tuples = [(nc, v) for nc in D.GOLD_NONCANONICAL for v in vals] + [(v, nc) for nc in D.GOLD_NONCANONICAL for v in vals]
    a, b = words([t[0] for t in tuples], 2), words([t[1] for t in tuples], 2)
    for op, name, fn in ((0, "mul", lambda x, y: x * y % p), (2, "add", lambda x, y: (x + y) % p), (3, "sub", lambda x, y: (x - y) % p),
                         (16, "select", lambda x, y: x % p), (18, "eq", lambda x, y: int((x - y) % p == 0))):
        got = be.canon(GOLD, op, a, b, a, b)
        exp = words([fn(x, y) for x, y in tuples], 2)
        bad = np.nonzero((got != exp).any(axis=1))[0]
        assert not len(bad), f"goldilocks {name} on non-canonical words, variant {be.name}: first {[(hex(tuples[i][0]), hex(tuples[i][1])) for i in bad[:4]]}"
    return 5 * len(tuples)


# ---- raw mode ---------------------------------------------------------------------------------------------------------------
def _edge_js(K):
    return sorted({0, 1, K - 1} & set(range(K)))


@functools.lru_cache(maxsize=None)
def raw_plan(fid):
    """list of (op, K, kb, a, b, c, d) with a..d lists of integer VALUES (raw representatives, value < kb[i] * p)"""
    _, p, NL, NL32 = BIG[fid]
    mb = D.max_bound(p, NL)
    Ks = [k for k in D.LAZY_K if k <= mb]
    seeds = D.raw_seeds(p, NL, NL32)
    sub = seeds[:8] + seeds[-4:]
    rnd = random.Random(77 + fid)
    edge = {K: [a0 + j * p for a0 in sub for j in _edge_js(K)] for K in Ks}
    full = {K: [v for a0 in seeds for v in D.lazy_values(a0, K, p, NL)] for K in Ks}
    plan = []

    def cross(la, lb):
        return [a for a in la for _ in lb], [b for _ in la for b in lb]

    for Ka in Ks:
        for Kb in Ks:
            a, b = cross(edge[Ka], edge[Kb])
            plan.append((0, 0, (Ka, Kb, 1, 1), a, b, a, b))
            perm = rnd.sample(range(len(a)), len(a))
            plan.append((2, 0, (Ka, Kb, Kb, Ka), a, b, [b[i] for i in perm], [a[i] for i in perm]))  # mul_add(a, b, c, d): c < Kb p, d < Ka p
            if Ka + Kb <= mb:
                plan.append((3, 0, (Ka, Kb, 1, 1), a, b, a, b))
            if Ka <= 32 and Kb <= 32:
                plan.append((9, 0, (Ka, Kb, 1, 1), a, b, a, b))
        plan.append((1, 0, (Ka, 1, 1, 1), full[Ka], full[Ka], full[Ka], full[Ka]))
        if Ka <= 32:
            plan.append((5, 0, (Ka, 1, 1, 1), full[Ka], full[Ka], full[Ka], full[Ka]))
            plan.append((8, 0, (Ka, 1, 1, 1), full[Ka], full[Ka], full[Ka], full[Ka]))
        if Ka <= 16:
            plan.append((6, 0, (Ka, 1, 1, 1), full[Ka], full[Ka], full[Ka], full[Ka]))
    for K in (2, 4, 8, 16):
        for Kb in [k for k in Ks if k <= K]:
            for Ka in [k for k in Ks if k + K <= mb]:
                a, b = cross(edge[Ka], edge[Kb])
                plan.append((4, K, (Ka, Kb, 1, 1), a, b, a, b))
    for K in (1, 2, 4, 8, 16):  # cond_sub<K> on everything below 2K p: exactly K p (a0 = 0, j = K) and its neighbours are in
        v = full[min(2 * K, mb)]
        plan.append((7, K, (min(2 * K, mb), 1, 1, 1), v, v, v, v))
    z = [j * p for j in range(4)] + [j * p + d for j in range(4) for d in (1, p - 1)] + full[4]
    plan.append((10, 0, (4, 1, 1, 1), z, z, z, z))
    canon = D.directed_values(p, NL, NL32)
    plan.append((11, 0, (1, 1, 1, 1), canon, canon, canon, canon))
    plan.append((12, 0, (1, 1, 1, 1), canon, canon, canon, canon))
    return plan


RAW_NAMES = {0: "mul", 1: "sqr", 2: "mul_add", 3: "add", 4: "sub<K>", 5: "reduce", 6: "below4", 7: "cond_sub<K>", 8: "is_zero", 9: "eq", 10: "maybe_zero_mulout",
             11: "pack", 12: "unpack"}


_RAW_CACHE = {}  # (fid, plan index) -> [operand arrays, output bytes that passed the checks]


def check_raw(be: Backend, fid):
    """the written contract of every op on raw lazy representatives; returns (tuples checked, {plan index: output bytes})"""
    _, p, NL, NL32 = BIG[fid]
    rop = 1 << (RB * NL - p.bit_length())  # the tracker's r_over_p()
    Rinv = pow(1 << (RB * NL), -1, p)
    outs, checked = {}, 0
    zero_mulouts = []
    if any(k[0] != fid for k in _RAW_CACHE):
        _RAW_CACHE.clear()
    for idx, (op, K, kb, a, b, c, d) in enumerate(raw_plan(fid)):
        if (fid, idx) not in _RAW_CACHE:
            if op == 12:  # words in
                arrs = [np.concatenate([words(a, NL32), np.zeros((len(a), NL - NL32), dtype=np.uint32)], axis=1)] * 4
            else:
                la, lb = limb_rows(a, NL), limb_rows(b, NL)
                arrs = [la, lb, limb_rows(c, NL) if c is not a else la, limb_rows(d, NL) if d is not b else lb]
            _RAW_CACHE[(fid, idx)] = [[np.ascontiguousarray(x) for x in arrs], None]
        arrs, verified = _RAW_CACHE[(fid, idx)]
        got = be.raw(fid, op, K, kb, *arrs)
        outs[idx] = got.tobytes()
        if verified is not None and verified == outs[idx]:  # bit-identical to an output that already passed every check below
            checked += len(a)
            continue
        ctx = (FIELD_NAME[fid], RAW_NAMES[op], "K", K, "bounds", kb, be.name)

        def fail(i, why):
            raise AssertionError(f"{ctx}: {why}\n  a={hex(a[i])}\n  b={hex(b[i])}\n  c={hex(c[i])}\n  d={hex(d[i])}\n  out limbs {[hex(int(v)) for v in got[i]]}")

        if op in (8, 9, 10):
            flags = [int(v) for v in got[:, 0]]
            assert not got[:, 1:].any(), ctx
            for i, f in enumerate(flags):
                if op == 8 and f != (a[i] % p == 0): fail(i, "is_zero wrong")
                if op == 9 and f != ((a[i] - b[i]) % p == 0): fail(i, "eq wrong")
                if op == 10 and a[i] % p == 0 and a[i] < 4 * p and not f: fail(i, "maybe_zero_mulout false on a zero-class value below 4p")
        elif op == 11:
            vals = row_ints(got[:, :NL32], 32)
            assert not got[:, NL32:].any(), ctx
            for i, v in enumerate(vals):
                if v != a[i]: fail(i, "pack: words differ from the value")
        else:
            if (got[:, : NL - 1] >> RB).any():
                fail(int(np.nonzero((got[:, : NL - 1] >> RB).any(axis=1))[0][0]), "a low limb is not below 2^29")
            vals = row_ints(got, RB)
            ka, kb_, kc, kd = kb
            for i, v in enumerate(vals):
                if op == 0: cls, bound = a[i] * b[i] * Rinv, ka * kb_ / rop + 1
                elif op == 1: cls, bound = a[i] * a[i] * Rinv, ka * ka / rop + 1
                elif op == 2: cls, bound = (a[i] * b[i] + c[i] * d[i]) * Rinv, (ka * kb_ + kc * kd) / rop + 1
                elif op == 3:
                    if v != a[i] + b[i]: fail(i, "add: not the exact sum")
                    continue
                elif op == 4:
                    if v != a[i] - b[i] + K * p: fail(i, "sub<K>: not a - b + K p")
                    continue
                elif op == 5:
                    if v != a[i] % p: fail(i, "reduce: not value mod p")
                    continue
                elif op == 6: cls, bound = a[i], 4
                elif op == 7:
                    if v != (a[i] - K * p if a[i] >= K * p else a[i]): fail(i, "cond_sub<K>: wrong decision or difference")
                    continue
                elif op == 12:
                    if v != a[i]: fail(i, "unpack: limbs differ from the value")
                    continue
                if (v - cls) % p: fail(i, "result not congruent to the exact value mod p")
                if not v < bound * p: fail(i, f"result not below the stated bound {bound} p")
                if op == 0 and cls % p == 0 and bound <= 4: zero_mulouts.append(v)
        _RAW_CACHE[(fid, idx)][1] = outs[idx]
        checked += len(a)
    zero_mulouts = _RAW_CACHE.setdefault((fid, "zero-class products"), zero_mulouts)  # (a build whose outputs were bit-identical skipped the loop above)
    if zero_mulouts:  # maybe_zero_mulout on the products the device itself made of zero-class operands
        z = zero_mulouts[:20000]
        la = limb_rows(z, NL)
        got = be.raw(fid, 10, 0, (4, 1, 1, 1), la, la, la, la)
        assert got[:, 0].all(), (FIELD_NAME[fid], "maybe_zero_mulout false on a zero-class mul output", be.name)
        checked += len(z)
    return checked, outs


# ---- 31-bit fields ------------------------------------------------------------------------------------------------------------
def check_small(be: Backend, fi):
    f = SMALL[fi]
    p = f.p
    dp, rp = D.small_pairs(p, fi)
    pairs = dp + rp
    a = np.array([x for x, _ in pairs], dtype=np.uint32)
    b = np.array([y for _, y in pairs], dtype=np.uint32)
    n = 0
    for op, name, fn in ((0, "mul", lambda x, y: x * y % p), (1, "add", lambda x, y: (x + y) % p), (2, "sub", lambda x, y: (x - y) % p),
                         (3, "pow", lambda x, y: pow(x, y, p)), (4, "inv", lambda x, y: pow(x, p - 2, p)), (5, "neg", lambda x, y: (-x) % p)):
        got = be.small(fi, op, a, b)
        exp = np.array([fn(x, y) for x, y in pairs], dtype=np.uint32)
        if not np.array_equal(got, exp):
            bad = np.nonzero(got != exp)[0]
            raise AssertionError(f"{f.name} {name} variant {be.name}: {len(bad)} differ; first " + ", ".join(f"({pairs[i][0]:#x}, {pairs[i][1]:#x}) got {int(got[i]):#x} exp {int(exp[i]):#x}" for i in bad[:4]))
        n += len(pairs)
    return n


# ---- EC tier: the sequences of test_host_math.py's test_ec_ops / test_g2_ec_ops, one per thread ----------------------------------
G1 = {0: pyref.BN254, 1: pyref.BLS12_381, 4: pyref.BLS12_377, 5: pyref.GRUMPKIN}
G2 = {2: pyref.BN254_G2, 3: pyref.BLS12_381_G2, 6: pyref.BLS12_377_G2}


SIGNED_ADD = (0, 5)   # EC::SIGNED_MADD: G1 over a 9-limb field (bn254, grumpkin) -- ec_case op 7
SMALL_B3 = (0, 1, 4)  # has_small_b3: bn254, bls12_381, bls12_377 G1 -- ec_case op 8, the quad tier's dbl_quad


class _Group:
    """a curve id's integer group law (oracle/pyref.py) and what the encodings need"""

    def __init__(self, ci):
        self.ci, self.g2 = ci, ci in G2
        self.c = G2[ci] if self.g2 else G1[ci]
        self.INF = pyref.INF2 if self.g2 else pyref.INF
        fns = (pyref.g2_add, pyref.g2_neg, pyref.g2_mul) if self.g2 else (pyref.ec_add, pyref.ec_neg, pyref.ec_mul)
        self.add, self.neg, self.mul = (functools.partial(f, self.c) for f in fns)
        self.order = self.c.base.r if self.g2 else self.c.r
        self.q = self.c.base.q if self.g2 else self.c.q
        self.n32 = self.c.base.limbs_q if self.g2 else self.c.limbs_q
        self.comp = 2 if self.g2 else 1
        self.zero = (0, 0) if self.g2 else 0

    def sum(self, pts, ng):
        acc = self.INF
        for p_, n_ in zip(pts, ng):
            acc = self.add(acc, self.neg(p_) if n_ else p_)
        return acc

    def affine(self, v):
        """3 * comp coordinate integers (X, Y, Z as the harnesses store them) -> (affine point, X, Y, Z)"""
        if self.g2:
            X, Y, Z = (v[0], v[1]), (v[2], v[3]), (v[4], v[5])
            return pyref.g2_proj_to_affine(self.c, X, Y, Z), X, Y, Z
        X, Y, Z = v
        return pyref.proj_to_affine(self.c, X, Y, Z), X, Y, Z


@functools.lru_cache(maxsize=None)
def group(ci):
    return _Group(ci)


@functools.lru_cache(maxsize=None)
def ec_base(ci):
    """the base points of ec_plan (its seed's first draw is their offset)"""
    G = group(ci)
    k0 = random.Random((142 if G.g2 else 42) + ci).randrange(G.order)
    return pyref.g2_gen_points(G.c, 20, k0=k0) if G.g2 else pyref.gen_points(G.c, 30, k0=k0)


@functools.lru_cache(maxsize=None)
def ec_plan(ci):
    """{op: list of (points, aux words, expected affine point)}"""
    g2 = ci in G2
    c = G2[ci] if g2 else G1[ci]
    INF = pyref.INF2 if g2 else pyref.INF
    add, neg, mul = (pyref.g2_add, pyref.g2_neg, pyref.g2_mul) if g2 else (pyref.ec_add, pyref.ec_neg, pyref.ec_mul)
    rnd = random.Random((142 if g2 else 42) + ci)
    order = c.base.r if g2 else c.r
    rnd.randrange(order)  # (the offset of the base points)
    base = ec_base(ci)
    seqs = []
    for trial in range(16 if g2 else 24):
        k = rnd.randrange(1, 14 if g2 else 16)
        pts = [rnd.choice(base) for _ in range(k)]
        ng = [rnd.randrange(2) for _ in range(k)]
        if trial % 3 == 0:  # doubling right at the start of a bucket
            pts[0:0] = [pts[0]] * 2
            ng[0:0] = [ng[0]] * 2
        if trial % 4 == 0:  # cancellation at the end
            pts.append(pts[-1])
            ng.append(1 - ng[-1])
        if trial % 5 == 0:
            pts.insert(1, INF)
            ng.insert(1, 0)
        if trial == 7:
            pts, ng = [base[0], base[0]], [0, 1]
        if trial == 8:
            pts, ng = [base[0], base[0], base[1]], [0, 1, 0]
        if trial == 9:
            pts, ng = [base[0]] * 9, [0] * 9
        exp = INF
        for p_, n_ in zip(pts, ng):
            exp = add(c, exp, neg(c, p_) if n_ else p_)
        seqs.append((pts, ng, exp))
    plan = {0: seqs, 1: seqs}
    plan[2] = [([base[3]], [k], mul(c, k, base[3])) for k in [0, 1, 2, 3, 5, 255, 256, 32767, 32768, 65535, 1 << 20]] + [([INF], [5], INF)]
    plan[4] = [([base[2]], [k], mul(c, 1 << k, base[2])) for k in [0, 1, 5, 16]]
    plan[5] = [([base[2]], [k], mul(c, 1 << k, base[2])) for k in [0, 1, 2, 7, 64, 300]] + [([INF], [9], INF)]
    plan[6] = [([b], [k], mul(c, 1 << k, b)) for k in [0, 1, 2, 3, 17, 84, 300] for b in (base[2], base[5])] + [([INF], [9], INF)]
    if ci in SIGNED_ADD:
        # op 7, one lane of k_reduce_wave on the signed layer: tri = add_signed(tri, line); line = add_signed(line, b_i) from two identities,
        # output signed_to_unsigned(add_signed(tri, line)) = sum (m - i) b_i over the buckets b_0 .. b_{m-1}
        P, Q, T = base[0], base[1], base[6]
        buckets = [(pts, ng) for pts, ng, _ in seqs]
        buckets += [([INF], [0]), ([INF] * 7, [0] * 7)]                                              # all-identity
        buckets += [([P] + [INF] * 6, [0] * 7), ([INF] * 3 + [P] + [INF] * 3, [0] * 7), ([INF] * 6 + [P], [0] * 7)]  # one bucket, first / middle / last
        buckets += [([P, P], [0, 0]), ([INF, Q, Q, INF, T, T, T], [0] * 7), ([Q, Q, P, P], [1, 1, 0, 0])]   # equal neighbouring buckets
        buckets += [([P, P], [0, 1]), ([Q, P, P, T], [0, 1, 0, 0]), ([P, P, Q, Q, INF, T, T], [0, 1, 1, 0, 0, 0, 1])]  # b, -b pairs
        plan[7] = []
        for pts, ng in buckets:
            tri, line = INF, INF
            for p_, n_ in zip(pts, ng):
                tri = add(c, tri, line)
                line = add(c, line, neg(c, p_) if n_ else p_)
            plan[7].append((pts, ng, add(c, tri, line)))
    if ci in SMALL_B3:  # op 8: op 5's cases through EcDblSmallB::dbl, the one-lane twin of dbl_quad
        plan[8] = plan[5]
    return plan


IDENTITY_FORM_OPS = (0, 1, 2, 5, 7, 8)  # complete formulas (and from_jac): the identity comes out as (0 : y != 0 : 0)


def encode_cases(G, cases):
    """(point words, offsets, aux words) of a case list as dm_ec / dm_ec_quad / host_ec_batch take them"""
    flat, offs, aux = [], [0], []
    for pts, ax, _ in cases:
        for (x, y) in pts:
            flat += list(x) + list(y) if G.g2 else [x, y]
        aux += list(ax) if len(ax) == len(pts) else list(ax) + [0] * (len(pts) - len(ax))
        offs.append(offs[-1] + len(pts))
    return words(flat, G.n32).reshape(-1), np.array(offs, dtype=np.int32), np.array(aux, dtype=np.uint32)


def run_ec(be: Backend, ci, op, cases):
    """one-lane tier: the canonical projective words of every case, one row each"""
    G = group(ci)
    return be.ec(ci, op, *encode_cases(G, cases), 3 * G.comp * G.n32)


def verify_points(G, rows, cases, ctx, identity_form=True):
    """rows of canonical projective words against the cases' expected affine points"""
    vals = row_ints(np.ascontiguousarray(rows).reshape(-1, G.n32), 32)
    k = 3 * G.comp
    for s, (pts, ax, exp) in enumerate(cases):
        v = vals[s * k:(s + 1) * k]
        assert all(t < G.q for t in v), (ctx, s, "a coordinate is not below q")
        got, X, Y, Z = G.affine(v)
        assert got == exp, f"{ctx} sequence {s}: aux {list(ax)}, points {[_hexpt(p_) for p_ in pts]}: got {_hexpt(got)} expected {_hexpt(exp)}"
        if exp == G.INF and identity_form:
            assert Z == G.zero and Y != G.zero, (ctx, s, "identity must be (0 : y != 0 : 0)")
    return len(cases)


def check_ec(be: Backend, ci):
    G = group(ci)
    n = 0
    for op, cases in ec_plan(ci).items():
        out = run_ec(be, ci, op, cases)
        n += verify_points(G, out, cases, f"{G.c.name} {'G2' if G.g2 else 'G1'} ec op {op} variant {be.name}", identity_form=op in IDENTITY_FORM_OPS)
    return n


def ec_unsupported(ci):
    """(op) pairs of the one-lane tier that must answer -1 for this curve"""
    return [op for op, ok in ((7, ci in SIGNED_ADD), (8, ci in SMALL_B3)) if not ok]


def _hexpt(pt):
    return "(" + ", ".join(_hex(v) for v in pt) + ")"


# ---- quad tier (device only): the four-lane EC operations, one sequence per DPP quad (device_math_harness.hip k_ec_quad) ------------
# Q0 complete sum with EcQuadAdd::add | Q1 the same with EC::add_quad | Q2 2^k P by dbl_quad | Q3 to_jac, k x dbl_jac_quad, from_jac |
# Q4 the Horner walk of k_final_horner, acc = 2^w acc + S down the sequence (aux = width << 1 | negate). Each function only for the
# curves the product instantiates it for; every other (curve, op) pair answers -1.
Q_ADD, Q_ADDQ, Q_DBL, Q_JAC, Q_HORNER = 0, 1, 2, 3, 4
Q_RAW = 0x100  # Q0 (two points per sequence) and Q2 (one point, one doubling): operands as raw Montgomery limb rows (X, Y, Z)
QUAD_CURVES = {Q_ADD: (0, 1, 4, 5, 2), Q_ADDQ: (5, 2, 3, 6), Q_DBL: SMALL_B3, Q_JAC: (5, 2, 3, 6), Q_HORNER: (0, 1, 2, 3, 4, 5, 6)}
QUAD_NAME = {Q_ADD: "EcQuadAdd::add", Q_ADDQ: "EC::add_quad", Q_DBL: "EcDblSmallB::dbl_quad", Q_JAC: "EC::dbl_jac_quad", Q_HORNER: "Horner walk"}
QUAD_TWIN = {Q_ADD: (1, "EC::add"), Q_ADDQ: (1, "EC::add"), Q_DBL: (8, "EcDblSmallB::dbl"), Q_JAC: (5, "EC::dbl_jac")}  # ec_case op of the one-lane twin
HORNER_CANCEL = -2  # index of the cancelling Horner case in quad_plan(ci)[Q_HORNER]


@functools.lru_cache(maxsize=None)
def quad_plan(ci):
    """{op: list of (points, aux words, expected affine point)} for the ops this curve has"""
    G = group(ci)
    base, INF = ec_base(ci), G.INF
    P, Q = base[0], base[1]
    plan = {}
    sums = list(ec_plan(ci)[1])
    for pts, ng in (([INF], [0]), ([INF, INF], [0, 0]), ([P, INF], [0, 0]), ([P] * 4, [0] * 4),  # [P] * 4: the sum meets the operand again after a doubling
                    ([P, Q, Q, P, Q, P], [0, 0, 1, 1, 0, 0])):                                        # the running sum returns to O in the middle and goes on
        sums.append((pts, ng, G.sum(pts, ng)))
    for op in (Q_ADD, Q_ADDQ):
        if ci in QUAD_CURVES[op]:
            plan[op] = sums
    for op in (Q_DBL, Q_JAC):
        if ci in QUAD_CURVES[op]:
            plan[op] = ec_plan(ci)[5]  # k in 0, 1, 2, 7, 64, 300 on a point with a non-trivial Z, and P = O

    def horner(pts, aux):
        acc = G.neg(pts[0]) if aux[0] & 1 else pts[0]
        for p_, a in zip(pts[1:], aux[1:]):
            acc = G.add(G.mul(1 << (a >> 1), acc), G.neg(p_) if a & 1 else p_)
        return acc

    H = []

    def case(pts, widths, ng=None):
        aux = [(w << 1) | n for w, n in zip(widths, ng or [0] * len(pts))]
        H.append((pts, aux, horner(pts, aux)))

    rnd = random.Random(4242 + ci)
    for t in range(11):
        n = rnd.randrange(3, 9)
        pts = [rnd.choice(base) for _ in range(n)]
        ws = [0] + [rnd.randrange(1, 23) for _ in range(n - 1)]
        if t == 0:
            ws[1], ws[-1] = 1, 22
        if t % 2 == 0:
            pts[rnd.randrange(1, n)] = INF
        case(pts, ws, [rnd.randrange(2) for _ in range(n)])
    case([INF] * 5, [0, 3, 22, 1, 8])           # every window sum the identity
    case([P, INF, INF, INF], [0, 22, 13, 1])    # only the top window
    case([INF, INF, INF, P], [0, 5, 1, 22])     # only window 0
    w1, w3 = 5, 22                                # S_i = -2^{w_i} acc: the addition after a doubling chain cancels, in the middle and at the end
    case([P, G.neg(G.mul(1 << w1, P)), Q, G.neg(G.mul(1 << w3, Q))], [0, w1, 7, w3])
    case([P, G.mul(1 << 4, P), Q], [0, 4, 9])   # S_i = +2^{w_i} acc: the addition is a doubling
    plan[Q_HORNER] = H
    return plan


def run_quad(be: Backend, ci, op, cases):
    G = group(ci)
    return be.ec_quad(ci, op, *encode_cases(G, cases), 3 * G.comp * G.n32)


def lanes_agree(out, ctx):
    """the four lanes of every quad stored identical words (lanes 1..3 feed the next operation of every real chain)"""
    for role in (1, 2, 3):
        bad = np.nonzero((out[:, role, :] != out[:, 0, :]).any(axis=1))[0]
        assert not len(bad), (ctx, f"lane {role} of the quad differs from lane 0 in sequences {bad[:8].tolist()}")
    return np.ascontiguousarray(out[:, 0, :])


_QUAD_VERIFIED = {}  # (ci, op) -> lane-0 bytes that passed the integer checks (a second build that returns the same bytes is not checked twice)


def check_ec_quad(be: Backend, ci):
    """every quad op of the curve on its directed sequences; returns ({op: comparisons}, {op: output bytes}, {op: twin claim held})"""
    G = group(ci)
    res, outs, twin_ok = {}, {}, {}
    for op in range(5):
        ctx = f"{G.c.name} {'G2' if G.g2 else 'G1'} quad op {op} ({QUAD_NAME[op]}) variant {be.name}"
        if ci not in QUAD_CURVES[op]:
            assert be.refuses("ec_quad", ci, op), (ctx, "the product does not instantiate this pair: the harness must answer -1")
            continue
        cases = quad_plan(ci)[op]
        rows = lanes_agree(run_quad(be, ci, op, cases), ctx)
        outs[op] = rows.tobytes()
        if _QUAD_VERIFIED.get((ci, op)) != outs[op]:
            verify_points(G, rows, cases, ctx)
            _QUAD_VERIFIED[(ci, op)] = outs[op]
        if op in QUAD_TWIN:  # the comment of each function claims "the same values" as its one-lane form
            top, tname = QUAD_TWIN[op]
            twin = run_ec(be, ci, top, cases)
            bad = np.nonzero((twin != rows).any(axis=1))[0]
            twin_ok[op] = not len(bad)
            assert not len(bad), (ctx, f"projective words differ from the one-lane twin {tname} in sequences {bad[:8].tolist()} (affine values agree: a projective scale)")
        res[op] = len(cases)
    for op, npts in ((Q_ADD | Q_RAW, 2), (Q_DBL | Q_RAW, 1), (Q_ADDQ | Q_RAW, 2), (Q_JAC | Q_RAW, 1), (Q_HORNER | Q_RAW, 2), (5, 1)):
        if (op & 0xFF) not in (Q_ADD, Q_DBL) or not op & Q_RAW or ci not in QUAD_CURVES[op & 0xFF]:
            assert be.refuses("ec_quad", ci, op, npts), (G.c.name, hex(op), "must answer -1")
    return res, outs, twin_ok


def check_ec_quad_placement(be: Backend, ci):
    """one complete-sum sequence and one Horner sequence in each of the 16 quad positions of a wave, the other 15 quads running different
    sequences of different lengths; once more in a launch whose sequence count is no multiple of 16. A sequence must give the same
    words wherever it runs (quads 3 and 4 sit on either side of the 16-lane DPP row boundary); the integers are consulted once per sequence.
    Returns {op: (sequence, placement) comparisons}"""
    G = group(ci)
    res = {}
    for op, ti in ((Q_ADD if ci in QUAD_CURVES[Q_ADD] else Q_ADDQ, 0), (Q_HORNER, HORNER_CANCEL)):
        ctx = f"{G.c.name} {'G2' if G.g2 else 'G1'} quad op {op} ({QUAD_NAME[op]}) placement, variant {be.name}"
        cases = quad_plan(ci)[op]
        target = cases[ti]  # sums: doubling at the start, inserted identity, cancellation at the end; Horner: the cancelling walk
        fillers = [c for c in cases if c is not target][:15]
        assert len(fillers) == 15 and len({len(c[0]) for c in fillers}) >= 4
        full = []
        for pos in range(16):
            full += fillers[:pos] + [target] + fillers[pos:]
        ragged = full + fillers[:2] + [target] + fillers[2:4]
        assert len(full) == 256 and len(ragged) % 16 == 5
        words_of = {}
        n = 0
        for layout in (full, ragged):
            rows = lanes_agree(run_quad(be, ci, op, layout), ctx)
            if not words_of:  # the first block holds every sequence once: position 0 for the target
                verify_points(G, rows[:16], layout[:16], ctx)
                words_of = {id(c): rows[i].tobytes() for i, c in enumerate(layout[:16])}
            for i, c in enumerate(layout):
                assert rows[i].tobytes() == words_of[id(c)], (ctx, f"sequence at index {i} (quad {i % 16} of its wave, launch of {len(layout)}) differs from the same sequence in another position")
            n += len(layout)
        res[op] = n
    return res


# raw operands at the documented bounds: ec_dbl_quad.hpp states X, Y, Z <= 8 p for the doubling, the additions are laid out for <= 4 p
CURVE_FIELD = {0: 0, 1: 2, 4: 4, 5: 1, 2: 0, 3: 2, 6: 4}  # curve id -> id of the field its coordinates (G2: their components) live in
RAW_STATED = {Q_ADD: 4, Q_DBL: 8}
HOST_RAW_FN = {Q_ADD: 0, Q_DBL: 2}  # host_ec_raw: 0 = E::add, 2 = EcDblSmallB::dbl (what host op 7 runs under the tracker)


@functools.lru_cache(maxsize=None)
def raw_quad_cases(ci, op, K):
    """(limb rows (points, 3 * comp * NL), offsets, cases): projective points with a non-trivial Z whose coordinates are the Montgomery
    representatives a0 + j p, j from _edge_js(K): 0, 1 and the largest inside the stated bound K p"""
    G = group(ci)
    _, p, NL, _ = BIG[CURVE_FIELD[ci]]
    assert p == G.q
    R = 1 << (RB * NL)
    A = Fp2(Fp(p, 1, 0)) if G.g2 else Fp(p, 1, 0)
    base = ec_base(ci)
    P, Q2, T = base[0], base[1], base[3]
    rnd = random.Random(8800 + 16 * ci + op)
    js = _edge_js(K)

    def elem():
        return tuple(rnd.randrange(1, p) for _ in range(2)) if G.g2 else rnd.randrange(1, p)

    def proj(pt):
        if pt == G.INF:
            return [G.zero, elem(), G.zero]
        lam = elem()
        return [A.mul(pt[0], lam), A.mul(pt[1], lam), lam]

    def reps(coords, jl):  # one j per coordinate (both components of an Fq2 coordinate take it)
        out = []
        for e, j in zip(coords, jl):
            out += [(v * R) % p + j * p for v in (e if G.g2 else (e,))]
        return out

    vals, offs, cases = [], [0], []

    def emit(points, jls, exp):
        for pt, jl in zip(points, jls):
            vals.extend(reps(proj(pt), jl))
        offs.append(offs[-1] + len(points))
        cases.append((points, [j for jl in jls for j in jl], exp))

    if op == Q_ADD:
        for a, b in ((P, Q2), (P, P), (P, G.neg(P)), (P, G.INF), (G.INF, P), (G.INF, G.INF)):
            exp = G.add(a, b)
            for ja in js:
                for jb in js:
                    emit([a, b], [[ja] * 3, [jb] * 3], exp)
            for _ in range(3):
                emit([a, b], [[rnd.choice(js) for _ in range(3)] for _ in range(2)], exp)
    else:
        for a in (P, T, G.INF):
            exp = G.add(a, a)
            for j in js:
                emit([a], [[j] * 3], exp)
            for _ in range(4):
                emit([a], [[rnd.choice(js) for _ in range(3)]], exp)
    assert all(v < K * p and v < R for v in vals)
    limbs = limb_rows(vals, NL).reshape(offs[-1], 3 * G.comp * NL)
    return np.ascontiguousarray(limbs), np.array(offs, dtype=np.int32), cases


HERE = os.path.dirname(os.path.abspath(__file__))
HOST_SO = os.path.join(HERE, "_build", "libhost_math.so")
HOST_SRC = os.path.join(HERE, "host_math_harness.cpp")
HOST_DEPS = [HOST_SRC, os.path.join(HERE, "math_cases.hpp")] + [os.path.join(HERE, "..", "icicle_amd", "csrc", f) for f in
                                                                ("bigfield.hpp", "fq2.hpp", "ec.hpp", "smallfield.hpp", "goldfield.hpp", "field_consts.h", "glv.hpp", "ec_dbl_quad.hpp")]


def host_lib():
    """tests/_build/libhost_math.so, the host build of the arithmetic headers with the bound tracker on; rebuilt when stale"""
    os.makedirs(os.path.dirname(HOST_SO), exist_ok=True)
    if not os.path.exists(HOST_SO) or any(os.path.getmtime(d) > os.path.getmtime(HOST_SO) for d in HOST_DEPS):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-DBIGFIELD_BOUNDS", "-fPIC", "-shared", HOST_SRC, "-o", HOST_SO + ".tmp"])
        os.replace(HOST_SO + ".tmp", HOST_SO)
    return HOST_SO


def _host_raw_child(ci, op, K, outpath):
    """(child process) the one-lane twin of a quad function on the raw operands of raw_quad_cases, bound tracker on: the tracker aborts
    the process when a stated bound K is outside a precondition"""
    G = group(ci)
    lib = ctypes.CDLL(HOST_SO)
    limbs, offs, cases = raw_quad_cases(ci, op, K)
    out = np.zeros((len(cases), 3 * G.comp * G.n32), dtype=np.uint32)
    rc = lib.host_ec_raw(ci, HOST_RAW_FN[op], K, len(cases), _p(limbs), _p(out))
    np.save(outpath, out)
    return rc


@functools.lru_cache(maxsize=None)
def host_raw_twin(ci, op, K):
    """(canonical projective words of the one-lane twin under the tracker, None) or (None, the tracker's message) when it aborted"""
    host_lib()
    root = os.path.dirname(HERE)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "out.npy")
        code = f"import sys; sys.path.insert(0, {root!r}); from tests import math_expect as X; sys.exit(X._host_raw_child({ci}, {op}, {K}, {path!r}))"
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=root, timeout=300)
        if r.returncode == 0:
            return np.load(path), None
    assert r.returncode == -signal.SIGABRT and "bigfield bound violation" in r.stderr, (ci, op, K, r.returncode, r.stderr[-2000:])
    return None, r.stderr.strip().splitlines()[0]


@functools.lru_cache(maxsize=None)
def accepted_raw_bound(ci, op):
    """(largest K <= the header's stated bound that the tracker accepts for the one-lane twin, its output rows, the refusals on the way)"""
    K, refused = RAW_STATED[op], []
    while K >= 1:
        rows, msg = host_raw_twin(ci, op, K)
        if rows is not None:
            return K, rows, tuple(refused)
        refused.append((K, msg))
        K //= 2
    raise AssertionError((ci, op, "the tracker accepts no bound", refused))


def check_host_raw(ci):
    """CPU leg: the tracker's accepted range against the header's, and the one-lane twin against the integers. {op: (accepted K, stated K, cases)}"""
    G = group(ci)
    res = {}
    for op in (Q_ADD, Q_DBL):
        if ci not in QUAD_CURVES[op]:
            continue
        K, rows, refused = accepted_raw_bound(ci, op)
        _, _, cases = raw_quad_cases(ci, op, K)
        verify_points(G, rows, cases, f"{G.c.name} {'G2' if G.g2 else 'G1'} host twin of {QUAD_NAME[op]} on raw operands below {K} p")
        res[op] = (K, RAW_STATED[op], len(cases), refused)
    return res


def check_ec_quad_raw(be: Backend, ci):
    """the quad addition and doubling on raw representatives up to the bound the tracker accepted for the one-lane twin (an operand
    outside it never reaches the device). Returns ({op: (accepted K, stated K, cases)}, {op: output bytes})"""
    G = group(ci)
    res, outs = {}, {}
    for op in (Q_ADD, Q_DBL):
        if ci not in QUAD_CURVES[op]:
            continue
        K, host_rows, _ = accepted_raw_bound(ci, op)
        limbs, offs, cases = raw_quad_cases(ci, op, K)
        ctx = f"{G.c.name} {'G2' if G.g2 else 'G1'} {QUAD_NAME[op]} on raw operands below {K} p, variant {be.name}"
        out = be.ec_quad(ci, op | Q_RAW, limbs.reshape(-1), offs, np.zeros(offs[-1], dtype=np.uint32), 3 * G.comp * G.n32)
        rows = lanes_agree(out, ctx)
        outs[op] = rows.tobytes()
        verify_points(G, rows, cases, ctx)
        bad = np.nonzero((rows != host_rows).any(axis=1))[0]
        assert not len(bad), (ctx, f"projective words differ from the one-lane twin on the host in cases {bad[:8].tolist()}")
        res[op] = (K, RAW_STATED[op], len(cases))
    return res, outs
