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
see j in {0, 1, K-1} of a subset of the seeds, for every admissible combination of stated bounds."""
import ctypes
import functools
import random

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


@functools.lru_cache(maxsize=None)
def ec_plan(ci):
    """{op: list of (points, aux words, expected affine point)}"""
    g2 = ci in G2
    c = G2[ci] if g2 else G1[ci]
    INF = pyref.INF2 if g2 else pyref.INF
    add, neg, mul = (pyref.g2_add, pyref.g2_neg, pyref.g2_mul) if g2 else (pyref.ec_add, pyref.ec_neg, pyref.ec_mul)
    rnd = random.Random((142 if g2 else 42) + ci)
    order = c.base.r if g2 else c.r
    base = (pyref.g2_gen_points(c, 20, k0=rnd.randrange(order)) if g2 else pyref.gen_points(c, 30, k0=rnd.randrange(order)))
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
    return plan


def check_ec(be: Backend, ci):
    g2 = ci in G2
    c = G2[ci] if g2 else G1[ci]
    q = c.base.q if g2 else c.q
    n32 = c.base.limbs_q if g2 else c.limbs_q
    comp = 2 if g2 else 1
    INF = pyref.INF2 if g2 else pyref.INF
    n = 0
    for op, cases in ec_plan(ci).items():
        flat, offs, aux = [], [0], []
        for pts, ax, _ in cases:
            for (x, y) in pts:
                flat += list(x) + list(y) if g2 else [x, y]
            aux += ax if len(ax) == len(pts) else ax + [0] * (len(pts) - len(ax))
            offs.append(offs[-1] + len(pts))
        out = be.ec(ci, op, words(flat, n32).reshape(-1), np.array(offs, dtype=np.int32), np.array(aux, dtype=np.uint32), 3 * comp * n32)
        vals = row_ints(out.reshape(-1, n32), 32)
        for s, (pts, ax, exp) in enumerate(cases):
            v = vals[s * 3 * comp:(s + 1) * 3 * comp]
            assert all(t < q for t in v), (c.name, op, s, be.name)
            if g2:
                X, Y, Z = (v[0], v[1]), (v[2], v[3]), (v[4], v[5])
                got = pyref.g2_proj_to_affine(c, X, Y, Z)
                zero = (0, 0)
            else:
                X, Y, Z = v
                got = pyref.proj_to_affine(c, X, Y, Z)
                zero = 0
            assert got == exp, f"{c.name} {'G2' if g2 else 'G1'} ec op {op} sequence {s} variant {be.name}: aux {ax}, points {[_hexpt(p_) for p_ in pts]}: got {_hexpt(got)} expected {_hexpt(exp)}"
            if exp == INF and op in (0, 1, 2, 5):
                assert Z == zero and Y != zero, (c.name, op, s, "identity must be (0 : y != 0 : 0)", be.name)
            n += 1
    return n


def _hexpt(pt):
    return "(" + ", ".join(_hex(v) for v in pt) + ")"
