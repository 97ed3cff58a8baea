"""CPU: ec.hpp's add_signed -- the complete projective addition (Renes-Costello-Batina Algorithm 7, a = 0) on the signed layer of
bigfield.hpp that k_reduce_wave and k_reduce_window use for bn254 and grumpkin -- and bigfield.hpp's smul_small under it, against
oracle/pyref in affine form and against Python integers.

tests/signed_add_harness.cpp is a stand-alone program built with the bound tracker on (-DBIGFIELD_BOUNDS), and once more with
-fsanitize=address,undefined; both builds answer the same requests. add_signed asserts its operand contract (normalised, value in
[-1.5, 4] p) and re-imposes it on the tracker at the top of every addition, asserts every column of its products below 2^63 and its
result inside the loop value's range at the end: a chain that runs through proves the range a fixed point. One negative test: an
operand one past the limb bound must abort a child process."""
import os
import random
import subprocess

import pytest

from oracle import pyref

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "signed_add_harness.cpp")
BUILD = os.path.join(HERE, "_build")
CSRC = os.path.join(HERE, "..", "icicle_amd", "csrc")
N, RB = 9, 29
M = (1 << RB) - 1
R = 1 << (RB * N)
FIELDS = {0: pyref.BN254.q, 1: pyref.GRUMPKIN.q}
CURVES = {0: pyref.BN254, 1: pyref.GRUMPKIN}
IDENT = "identity"


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
        return _build("signed_add_harness", [])
    return _build("signed_add_harness_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan"])


def _run(exe, text, check=True):
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600)
    if check:
        assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    return r


def val(l):
    return sum(int(v) << (RB * i) for i, v in enumerate(l))


def norm_limbs(v):
    """any integer of the element's range: limbs 0..7 in [0, 2^29), the (signed) rest in the top limb"""
    return [(v >> (RB * i)) & M for i in range(N - 1)] + [v >> (RB * (N - 1))]


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


def proj(c, pt, z=1, reps=(0, 0, 0)):
    """27 limbs of the affine point (or IDENT / pyref.INF) as (x z : y z : z) in Montgomery form, coordinate j as its residue + reps[j] p"""
    q = c.q
    if pt == IDENT or pt == pyref.INF:
        X, Y, Z = 0, z % q, 0
    else:
        X, Y, Z = pt[0] * z % q, pt[1] * z % q, z % q
    out = []
    for v, k in zip((X, Y, Z), reps):
        out += norm_limbs(v * R % q + k * q)
    return out


def proj_with_coordinate(c, pt, j, mont_value):
    """the point with the Montgomery form of coordinate j (0: X, 1: Y) equal to mont_value exactly: the scaling z is solved for"""
    q = c.q
    z = mont_value * pow(R, -1, q) % q * pow(pt[j], -1, q) % q
    limbs = proj(c, pt, z)
    assert val(limbs[9 * j:9 * j + 9]) == mont_value % q
    limbs[9 * j:9 * j + 9] = norm_limbs(mont_value)
    return limbs


def _points_out(c, words):
    pts = []
    for o in range(0, len(words), 24):
        X, Y, Z = (sum(v << (32 * k) for k, v in enumerate(words[o + 8 * j:o + 8 * j + 8])) for j in range(3))
        assert X < c.q and Y < c.q and Z < c.q
        if Z == 0:
            assert X == 0 and Y != 0  # the identity is (0 : y != 0 : 0), as the complete formulas leave it
        pts.append(pyref.proj_to_affine(c, X, Y, Z))
    return pts


def _affine(pt):
    return pyref.INF if pt == IDENT else pt


@pytest.mark.parametrize("f", [0, 1])
def test_small_constant_step(exe, f):
    """smul_small<K>: K a, normalised, on directed limbs -- any int32 limb goes in, K times a limb need not fit an int32"""
    p = FIELDS[f]
    rnd = random.Random(77 + f)
    I = (1 << 31) - 1
    D = [[0] * N, [1] * N, [M] * N, [-M] * N, [M + 1] * (N - 1) + [3], [(1 << 30) - 1] * (N - 1) + [1 << 20], [-(1 << 30)] * (N - 1) + [-(1 << 20)],
         [I] * (N - 1) + [1 << 24], [-I] * (N - 1) + [-(1 << 24)], [I if i % 2 else -I for i in range(N - 1)] + [0],
         norm_limbs(p - 1), norm_limbs(4 * p - 1), norm_limbs(-p), norm_limbs(-3 * p // 2), [0] * (N - 1) + [-1],
         [rnd.randrange(-M, M + 1) for _ in range(N - 1)] + [-(1 << 22)], [rnd.randrange(M + 1) for _ in range(N - 1)] + [rnd.randrange(1 << 22)]]
    req = [(K, a) for K in (3, 9, 12, -9, 64, -64) for a in D if abs(K * a[N - 1]) + abs(K) * 8 < (1 << 31)]
    out = _run(exe, "".join(f"S {f} {K} " + " ".join(map(str, a)) + "\n" for K, a in req)).stdout.split("\n")
    assert len(out) >= len(req)
    for ln, (K, a) in zip(out, req):
        t = ln.split()
        assert t[0] == "R" and len(t) == N + 1, ln
        got = [int(v) for v in t[1:]]
        assert val(got) == K * val(a), (K, a, got)
        assert all(0 <= v <= M for v in got[:N - 1]) and -(1 << 31) <= got[N - 1] < (1 << 31), (K, a, got)
    print(f"field {f}: {len(req)} small-constant steps against Python integers")


@pytest.mark.parametrize("ci", [0, 1])
def test_directed_additions(exe, ci):
    c = CURVES[ci]
    q = c.q
    rnd = random.Random(310 + ci)
    P, Q, S = pyref.gen_points(c, 3, k0=rnd.randrange(c.r))
    cases = []  # (limbs of p, limbs of q, expected affine)

    def case(a, b, la=None, lb=None):
        cases.append((la or proj(c, a, rnd.randrange(1, q)), lb or proj(c, b, rnd.randrange(1, q)), pyref.ec_add(c, _affine(a), _affine(b))))

    negP = pyref.ec_neg(c, P)
    for a, b in ((P, Q), (P, P), (P, negP), (P, IDENT), (IDENT, P), (IDENT, IDENT), (Q, S), (negP, negP)):
        case(a, b)
        case(a, b, proj(c, a, 1), proj(c, b, 1))
    # a point (0, y) if the curve has one, with itself, its negative, the identity and another point
    y0 = _sqrt_mod(c.b, q)
    if y0:
        Z0 = (0, y0)
        assert pyref.on_curve(c, Z0)
        for a, b in ((Z0, Z0), (Z0, pyref.ec_neg(c, Z0)), (Z0, IDENT), (IDENT, Z0), (Z0, P), (Q, Z0)):
            case(a, b)
    # every representative the contract allows: a loop value lies in (-1.5, 1.75) p -- residue - p, residue, and + p where that stays
    # inside --, what lies in memory is unsigned below 4 p: residue + 0 .. 3 p; both operands may be of either kind
    for reps_a in ((-1, -1, -1), (0, -1, 0), (-1, 0, 0), (0, 0, -1)):
        for reps_b in ((3, 3, 3), (0, 3, 1), (2, 0, 3), (-1, -1, -1), (1, 2, 3)):
            for a, b in ((P, Q), (P, P), (P, negP), (IDENT, Q), (P, IDENT), (IDENT, IDENT)):
                za, zb = rnd.randrange(1, q), rnd.randrange(1, q)
                case(a, b, proj(c, a, za, reps_a), proj(c, b, zb, reps_b))
                case(b, a, proj(c, b, zb, reps_b), proj(c, a, za, reps_a))
    # extreme limbs: one coordinate all ones (2^29 - 1 in limbs 0..7) or all zeros below the top, at the largest top limb below 4 p
    # (memory) and at a negative top limb (loop value)
    top4 = (4 * q - 1) >> (RB * (N - 1))
    for j in (0, 1):
        for mv in (val([M] * (N - 1) + [top4 - 1]), val([0] * (N - 1) + [top4 - 1]), val([M] * (N - 1) + [0]), val([1] + [0] * (N - 1))):
            case(P, Q, None, proj_with_coordinate(c, Q, j, mv))
            case(Q, Q, proj_with_coordinate(c, Q, j, mv), proj_with_coordinate(c, Q, 1 - j, mv))
        for mv in (val([M] * (N - 1) + [-1]), val([0] * (N - 1) + [-(q >> (RB * (N - 1)))]), -q - q // 3):
            case(P, Q, proj_with_coordinate(c, P, j, mv), None)
            case(P, P, proj_with_coordinate(c, P, j, mv), proj_with_coordinate(c, P, j, mv))
    out = _run(exe, "".join(f"A {ci} " + " ".join(map(str, la + lb)) + "\n" for la, lb, _ in cases)).stdout.split("\n")
    assert len(out) >= len(cases)
    for ln, (la, lb, e) in zip(out, cases):
        t = ln.split()
        assert t[0] == "P" and len(t) == 25, ln
        assert _points_out(c, [int(v) for v in t[1:]])[0] == e, (la, lb)
    print(f"curve {ci}: {len(cases)} directed additions against pyref")


def _buckets(c, n, seed):
    """the buckets of a chunk as k_reduce_wave meets them, last row first: random points with identities, runs of one point (after
    the first of a run tri == line: an addition that is a doubling) and cancelling pairs among them, at the representatives memory
    holds (unsigned, residue + 0 .. 3 p per coordinate), and the expected (tri, line)"""
    rnd = random.Random(seed)
    pool = pyref.gen_points(c, 40, k0=rnd.randrange(c.r))
    seq = [pool[0], IDENT, IDENT, pool[1], pyref.ec_neg(c, pool[1])]  # line back at pool[0] ...
    while len(seq) < n:
        ev = rnd.randrange(12)
        if ev == 0:
            seq.append(IDENT)
        elif ev == 1:
            pt = rnd.choice(pool)
            seq += [pt, pyref.ec_neg(c, pt)]
        elif ev == 2:
            seq += [rnd.choice(pool)] * 3
        elif ev == 3:
            seq.append("-line")  # the bucket that empties the column sum
        elif ev == 4:
            seq.append("line")  # the column sum itself: line doubles
        else:
            seq.append(rnd.choice(pool))
    tri = line = pyref.INF
    rows = []
    for b in seq:
        if b == "-line":
            b = pyref.ec_neg(c, line) if line != pyref.INF else IDENT
        elif b == "line":
            b = line if line != pyref.INF else IDENT
        tri = pyref.ec_add(c, tri, line)
        line = pyref.ec_add(c, line, _affine(b))
        rows.append(proj(c, b, rnd.randrange(1, c.q), tuple(rnd.randrange(4) for _ in range(3))))
    return rows, tri, line


@pytest.mark.parametrize("ci", [0, 1])
def test_reduction_loop_chains(exe, ci):
    """tri += line; line += bucket, a few thousand steps: the invariant is asserted and re-imposed at the top of every addition"""
    c = CURVES[ci]
    for n, seed in ((3000, 500 + ci), (2, 510 + ci), (65, 520 + ci)):
        rows, tri, line = _buckets(c, n, seed)
        r = _run(exe, f"L {ci} {len(rows)}\n" + "".join(" ".join(map(str, row)) + "\n" for row in rows))
        t = r.stdout.split()
        assert t[0] == "P" and len(t) == 49, r.stdout[:200]
        got = _points_out(c, [int(v) for v in t[1:]])
        assert got == [tri, line], (n, seed)
        if n == 3000:
            assert tri != pyref.INF
    # all buckets empty: the identity throughout; one point in every bucket: tri == line at the second step
    pt = pyref.gen_points(c, 1, k0=9)[0]
    for b, n in ((IDENT, 40), (pt, 40)):
        rows = [proj(c, b, 5 + i, (i % 4, (i + 1) % 4, (i + 2) % 4)) for i in range(n)]
        t = _run(exe, f"L {ci} {n}\n" + "".join(" ".join(map(str, row)) + "\n" for row in rows)).stdout.split()
        e = _affine(b)
        assert _points_out(c, [int(v) for v in t[1:]]) == [pyref.ec_mul(c, n * (n - 1) // 2, e) if e != pyref.INF else e, pyref.ec_mul(c, n, e) if e != pyref.INF else e]


def test_operand_outside_the_limb_bound_trips_the_tracker():
    """add_signed states normalised operands (limbs 0..7 in [0, 2^29)): 2^29 - 1 passes, 2^29 aborts the child with the tracker's message"""
    exe = _build("signed_add_harness", [])
    ok = _run(exe, "T 0\n")
    assert ok.stdout.strip() == "T ok"
    bad = _run(exe, "T 1\n", check=False)
    assert bad.returncode != 0 and "T ok" not in bad.stdout
    assert "bigfield bound violation" in bad.stderr and "operand must be normalised" in bad.stderr, bad.stderr[-2000:]
