"""CPU: the signed layer of bigfield.hpp (limb-wise add / sub / neg / 2a + b / conditional negate, the signed carry pass, the
Montgomery products of signed operands) and the mixed addition of ec.hpp that runs on it, against Python integers.

tests/signed_limbs_harness.cpp is a stand-alone program built with the bound tracker on (-DBIGFIELD_BOUNDS), and once more with
-fsanitize=address,undefined; both builds answer the same requests. Directed limbs first, then madd() chains of a few thousand
additions per curve against oracle/pyref, where the tracker re-imposes the accumulator's stated invariant at the top of every
addition -- a chain that runs through proves the invariant a fixed point --, and one negative test: an operand one past the limb
bound madd() states must abort a child process."""
import os
import random
import subprocess

import pytest

from oracle import pyref

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "signed_limbs_harness.cpp")
BUILD = os.path.join(HERE, "_build")
CSRC = os.path.join(HERE, "..", "icicle_amd", "csrc")
N, RB = 9, 29
M = (1 << RB) - 1
R = 1 << (RB * N)
FIELDS = {0: pyref.BN254.q, 1: pyref.BN254.r}
CURVES = {0: pyref.BN254, 1: pyref.GRUMPKIN}


def _build(name, extra):
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, name)
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("bigfield.hpp", "fq2.hpp", "ec.hpp", "field_consts.h", "mont_asm.hpp")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-DBIGFIELD_BOUNDS"] + extra + [SRC, "-o", exe])
    return exe


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request):
    if request.param == "plain":
        return _build("signed_limbs_harness", [])
    return _build("signed_limbs_harness_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan"])


def _run(exe, text, check=True):
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600)
    if check:
        assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    return r


def val(l):
    return sum(int(v) << (RB * i) for i, v in enumerate(l))


def norm_limbs(v):
    """v >= 0 below 2^(29 * 9 + 2): limbs 0..7 in [0, 2^29), the rest in the top limb"""
    return [(v >> (RB * i)) & M for i in range(N - 1)] + [v >> (RB * (N - 1))]


def directed(p):
    """limb vectors inside what every product takes (|limb| <= 2^29 - 1, 27 products of 2^58 per column)"""
    rnd = random.Random(p & 0xFFFF)
    d = [[0] * N, [1] * N, [M] * N, [-M] * N,
         [M if i % 2 == 0 else -M for i in range(N)], [-M if i % 2 == 0 else M for i in range(N)], [M if i % 2 else 0 for i in range(N)],
         norm_limbs(p - 1), norm_limbs(p), norm_limbs(2 * p), norm_limbs(1), norm_limbs(p >> 1),
         [0] * (N - 1) + [-1], [rnd.randrange(M + 1) for _ in range(N - 1)] + [-5], [rnd.randrange(-M, M + 1) for _ in range(N - 1)] + [-(1 << 24)],
         [-M] * (N - 1) + [-(1 << 25)], [rnd.randrange(-M, M + 1) for _ in range(N)], [rnd.randrange(M + 1) for _ in range(N - 1)] + [rnd.randrange(1 << 22)]]
    assert all(len(v) == N for v in d)
    return d


def wide():
    """for the limb-wise operations and the carry pass: limbs up to 2^30 - 1 in magnitude (a sum still fits an int32), and the
    widest operand the mixed addition normalises: R^2 - (2Q + PPP), limbs in (-3 * 2^29, 2^29)"""
    W = (1 << 30) - 1
    return [[W] * N, [-W] * N, [W if i % 2 else -W for i in range(N)], [-3 * (M + 1) + 1] * (N - 1) + [-77], [M] * (N - 1) + [1 << 26],
            [-3 * M if i % 3 else M for i in range(N - 1)] + [5], [1 << RB] * N, [-(1 << RB)] * N, [-1] * N]


def mont(p, *pairs):
    """(sum of a b + m p) / R with the one m in [0, R) that makes the division exact"""
    s = sum(a * b for a, b in pairs)
    m = (-s * pow(p, -1, R)) % R
    assert (s + m * p) % R == 0
    return (s + m * p) // R


def line(f, op, flag, *ops):
    ops = list(ops) + [[0] * N] * (4 - len(ops))
    return f"F {f} {op} {flag} " + " ".join(str(v) for o in ops for v in o)


@pytest.mark.parametrize("f", [0, 1])
def test_directed_limbs(exe, f):
    p = FIELDS[f]
    D = directed(p)
    L = D + wide()
    req, exp = [], []  # exp: ("limbs", [..]) exact limbs, or ("value", v) normalised limbs of that value

    def ask(op, flag, ops, kind, e):
        req.append(line(f, op, flag, *ops))
        exp.append((op, ops, kind, e))

    for a in L:
        ask("neg", 0, [a], "limbs", [-x for x in a])
        ask("cneg", 0, [a], "limbs", list(a))
        ask("cneg", 1, [a], "limbs", [-x for x in a])
        ask("norm", 0, [a], "value", val(a))
        for b in L:  # (a result limb outside int32 is what the tracker refuses: those pairs are not asked)
            for op, e in (("add", [x + y for x, y in zip(a, b)]), ("sub", [x - y for x, y in zip(a, b)])):
                if all(abs(v) < (1 << 31) for v in e) and max(abs(min(a[:-1])) + abs(min(b[:-1])), max(a[:-1]) + max(b[:-1]), abs(min(a[:-1])) + max(b[:-1]), max(a[:-1]) + abs(min(b[:-1]))) < (1 << 31):
                    ask(op, 0, [a, b], "limbs", e)
    for a in D:
        for b in D:
            ask("add2", 0, [a, b], "limbs", [2 * x + y for x, y in zip(a, b)])
            ask("mul", 0, [a, b], "value", mont(p, (val(a), val(b))))
            ask("mul_inplace", 0, [a, b], "value", mont(p, (val(a), val(b))))
        ask("sqr", 0, [a], "value", mont(p, (val(a), val(a))))
        for K in (1, 2, 8):
            if -K * p <= val(a) <= (60 - K) * p:  # (the result is an element of the unsigned operations: below 64 p)
                ask(f"tou{K}", 0, [a], "unsigned", val(a) + K * p)
    for i in range(len(D)):  # a b + c d: every operand through every position, the all-extreme tuples among them
        for s in (1, 3, 4, 7):
            a, b, c, d = D[i], D[(i * s + 1) % len(D)], D[(i + s) % len(D)], D[(i * s + 5) % len(D)]
            e = mont(p, (val(a), val(b)), (val(c), val(d)))
            ask("mul_add", 0, [a, b, c, d], "value", e)
            ask("mul_add_inplace_c", 0, [a, b, c, d], "value", e)
    for a, b, c, d in ([[-M] * N] * 4, [[M] * N, [-M] * N, [M] * N, [-M] * N], [[M] * N] * 4):
        ask("mul_add", 0, [a, b, c, d], "value", mont(p, (val(a), val(b)), (val(c), val(d))))
    out = _run(exe, "\n".join(req) + "\n").stdout.split("\n")
    assert len(out) >= len(req)
    for ln, (op, ops, kind, e) in zip(out, exp):
        t = ln.split()
        assert t[0] == "R" and len(t) == N + 1, ln
        got = [int(v) for v in t[1:]]
        if kind == "limbs":
            assert got == e, (op, ops, got)
        else:
            assert val(got) == e, (op, ops, got)
            assert all(0 <= v <= M for v in got[:N - 1]), (op, ops, got)
            assert -(1 << 31) <= got[N - 1] < (1 << 31)
            if kind == "unsigned":
                assert got[N - 1] >= 0
    print(f"field {f}: {len(req)} signed operations against Python integers")


def _sqrt_mod(a, q):
    """Tonelli-Shanks; None if a is no square"""
    a %= q
    if a == 0:
        return 0
    if pow(a, (q - 1) // 2, q) != 1:
        return None
    if q % 4 == 3:
        return pow(a, (q + 1) // 4, q)
    s, t = 0, q - 1
    while t % 2 == 0:
        s, t = s + 1, t // 2
    z = 2
    while pow(z, (q - 1) // 2, q) != q - 1:
        z += 1
    m, c, u, r = s, pow(z, t, q), pow(a, t, q), pow(a, (t + 1) // 2, q)
    while u != 1:
        i, w = 0, u
        while w != 1:
            w, i = w * w % q, i + 1
        b = pow(c, 1 << (m - i - 1), q)
        m, c, u, r = i, b * b % q, u * b * b % q, r * b % q
    return r


def _point_with_x_limb0(c, l0):
    """a curve point whose x has the given lowest 29-bit limb (both groups have cofactor 1: every curve point is a group element)"""
    x = l0 + (12345 << RB)
    while True:
        y = _sqrt_mod(x * x * x + c.b, c.q)
        if y:
            assert pyref.on_curve(c, (x, y))
            return (x, y)
        x += 1 << RB


def _chain(c, n, seed):
    """points, negate flags, modes and the expected sum: random picks from a pool (with the filter's four lowest-limb constants among
    the x coordinates), every other step negated, and every 37 steps one of: the accumulator's own value (doubling in mid-chain),
    its negative (cancel) followed by the same point twice (first-point path, then doubling), a point and at once its negative"""
    rnd = random.Random(seed)
    p0 = c.q & M
    pool = pyref.gen_points(c, 48, k0=rnd.randrange(c.r)) + [_point_with_x_limb0(c, l0) for l0 in (0, p0, (2 * p0) & M, (3 * p0) & M)]
    for pt, l0 in zip(pool[-4:], (0, p0, (2 * p0) & M, (3 * p0) & M)):
        assert pt[0] & M == l0
    steps, acc = [], pyref.INF

    def push(pt, neg, mode):
        nonlocal acc
        steps.append((pt, neg, mode))
        acc = pyref.ec_add(c, acc, pyref.ec_neg(c, pt) if neg else pt)

    push(pool[0], 0, 0)  # a point, its negative (cancel), then the same point twice (refill, doubling)
    push(pool[0], 1, 0)
    assert acc == pyref.INF
    push(pool[1], 0, 1)
    push(pool[1], 0, 0)
    i = 0
    while len(steps) < n:
        i += 1
        neg, mode = len(steps) & 1, (len(steps) >> 1) & 1
        if i % 37 == 0 and acc != pyref.INF:
            ev = (i // 37) % 3
            if ev == 0:  # acc + acc
                push(pyref.ec_neg(c, acc) if neg else acc, neg, mode)
            elif ev == 1:  # acc - acc, then P, P
                push(acc if neg else pyref.ec_neg(c, acc), neg, mode)
                assert acc == pyref.INF
                pt = rnd.choice(pool)
                push(pt, 0, mode)
                push(pyref.ec_neg(c, pt), 1, 1 - mode)
            else:  # ... + P - P
                pt = rnd.choice(pool)
                push(pt, neg, mode)
                push(pt, 1 - neg, mode)
            continue
        if i % 101 == 0:
            push(pyref.INF, 0, 0)  # (0, 0): skipped
            continue
        push(rnd.choice(pool), neg, mode)
    return steps, acc


def _chain_text(ci, steps):
    rows = [f"C {ci} {len(steps)}"]
    for (x, y), neg, mode in steps:
        rows.append(" ".join(str((v >> (32 * k)) & 0xFFFFFFFF) for v in (x, y) for k in range(8)) + f" {neg} {mode}")
    return "\n".join(rows) + "\n"


def _chain_result(c, r):
    t = r.stdout.split()
    assert t[0] == "P" and len(t) == 25, r.stdout[:200]
    w = [int(v) for v in t[1:]]
    X, Y, Z = (sum(v << (32 * k) for k, v in enumerate(w[8 * j:8 * j + 8])) for j in range(3))
    assert X < c.q and Y < c.q and Z < c.q
    return pyref.proj_to_affine(c, X, Y, Z), (X, Y, Z)


@pytest.mark.parametrize("ci", [0, 1])
def test_madd_chains(exe, ci):
    c = CURVES[ci]
    steps, exp = _chain(c, 3000, 900 + ci)
    got, _ = _chain_result(c, _run(exe, _chain_text(ci, steps)))
    assert got == exp and exp != pyref.INF
    # a chain that ends on a cancellation: the identity as (0 : y != 0 : 0)
    steps, acc = _chain(c, 120, 950 + ci)
    steps.append((acc, 1, 0))
    got, raw = _chain_result(c, _run(exe, _chain_text(ci, steps)))
    assert got == pyref.INF and raw[2] == 0 and raw[1] != 0
    # one point, and one point twice
    pt = pyref.gen_points(c, 1, k0=31)[0]
    assert _chain_result(c, _run(exe, _chain_text(ci, [(pt, 1, 0)])))[0] == pyref.ec_neg(c, pt)
    assert _chain_result(c, _run(exe, _chain_text(ci, [(pt, 1, 0), (pt, 1, 1)])))[0] == pyref.ec_add(c, pyref.ec_neg(c, pt), pyref.ec_neg(c, pt))


def test_operand_outside_the_limb_bound_trips_the_tracker():
    """madd() states limbs in (-2^29, 2^29) for its operand: 2^29 - 1 passes, 2^29 aborts the child with the tracker's message"""
    exe = _build("signed_limbs_harness", [])
    ok = _run(exe, "T 0\n")
    assert ok.stdout.strip() == "T ok"
    bad = _run(exe, "T 1\n", check=False)
    assert bad.returncode != 0 and "T ok" not in bad.stdout
    assert "bigfield bound violation" in bad.stderr and "operand limb outside" in bad.stderr, bad.stderr[-2000:]
