"""Poseidon2 over BabyBear and KoalaBear in Python integers: the parameter derivation, the hash and a Merkle tree over it.

Written from the specification, independently of icicle_amd/csrc/poseidon2_params.h and poseidon2.hpp, and with other means where
there is a choice, so that the two do not share a shortcut:
  * both linear layers are dense matrix-vector products here (the device code uses the addition chain of M4 and sum + diagonal);
  * the characteristic polynomial is computed from the Hessenberg form (the C++ uses the Krylov sequence of a vector);
  * polynomials are multiplied as packed integers (Kronecker substitution).

The derivation (Poseidon, USENIX Security 2021 / eprint 2019/458; Poseidon2, eprint 2023/323; binomial bound eprint 2023/537):
  alpha         smallest a >= 3 with gcd(a, p - 1) = 1
  R_F, R_P      the cheapest pair (t R_F + R_P, ties to the smaller R_F) that meets the statistical, interpolation, Groebner and
                binomial bounds at M = 128, plus the margin R_F += 2, R_P = ceil(1.075 R_P)
  constants     Grain LFSR, R_F t + R_P values in round order: t per full round, one per partial round
  M_E           circ(2, 1), circ(2, 1, 1), M4, or blocks of M4 with 2 M4 on the diagonal
  M_I           all ones off the diagonal; diagonal (2, 3), (2, 2, 3), or drawn from the same Grain stream until the characteristic
                polynomial of M_I^i is irreducible for i = 1 .. 2t
Hash semantics: the reference's CPU backend (backend/cpu/src/hash/cpu_poseidon2.cpp), restated at hash().
"""
import functools
from math import ceil, comb, floor, gcd, log, log2

FIELDS = {"babybear": 0x78000001, "koalabear": 0x7F000001}
WIDTHS = (2, 3, 4, 8, 12, 16, 20, 24)
SECURITY = 128


# ---- round numbers ---------------------------------------------------------------------------------------------------------------
def alpha_of(p):
    a = 3
    while gcd(a, p - 1) != 1:
        a += 1
    return a


def ceil_log(base, x):
    """smallest k with base^k >= x"""
    k, v = 0, 1
    while v < x:
        v, k = v * base, k + 1
    return k


def rounds_suffice(p, t, alpha, r_f, r_p):
    """True when r_f full and r_p partial rounds (before the margin) withstand the attacks at SECURITY bits."""
    n, lg, m = p.bit_length(), log2(p), SECURITY
    log_a_2 = log(2) / log(alpha)
    # statistical attacks: 6 full rounds while the S-box's differential probability over t + 1 words stays below 2^-M, else 10 (the
    # parameter script takes (alpha - 1) / 2 for the constant of the paper's eq. 2, and the published instances follow the script)
    full = [6 if m <= floor(lg - (alpha - 1) / 2.0) * (t + 1) else 10]
    # interpolation attack
    full.append(1 + ceil(log_a_2 * min(m, n)) + ceil_log(alpha, t) - r_p)
    # Groebner basis attacks, three ways of writing the system down
    full.append(ceil(log_a_2 * min(m, lg) - r_p))
    full.append(ceil(t - 1 + log_a_2 * min(m / (t + 1), lg / 2) - r_p))
    full.append(ceil((t - 2 + m / (2 * log2(alpha)) - r_p) / (t - 1)))
    if r_f < max(full):
        return False
    # eprint 2023/537: the attack that skips rounds costs binom(v + d, v)^2 with v the variables and d the degree left; r_f is even,
    # so every argument is an integer
    r = t // 3
    under = r * (r_f // 2) + r_p + alpha
    over = (r_f - 1) * t + r_p + r + under
    return comb(over, under) ** 2 > 1 << (m - 1)  # ceil(2 log2 binom) >= M


@functools.lru_cache(maxsize=None)
def round_numbers(p, t):
    alpha, best = alpha_of(p), None
    for r_p in range(1, 500):
        for r_f in range(4, 100, 2):
            if rounds_suffice(p, t, alpha, r_f, r_p):
                cand = (t * (r_f + 2) + ceil(1.075 * r_p), r_f + 2, ceil(1.075 * r_p))
                if best is None or cand[:2] < best[:2]:
                    best = cand
                break  # a larger r_f with this r_p only costs more
    return alpha, best[1], best[2]


# ---- Grain ---------------------------------------------------------------------------------------------------------------------------
class Grain:
    """The 80-bit LFSR of the Poseidon papers, self-shrinking output."""

    def __init__(self, n, t, r_f, r_p):
        seed = f"{1:02b}{0:04b}{n:012b}{t:012b}{r_f:010b}{r_p:010b}" + "1" * 30
        assert len(seed) == 80
        self.s = [int(c) for c in seed]
        for _ in range(160):
            self.step()

    def step(self):
        s = self.s
        b = s[62] ^ s[51] ^ s[38] ^ s[23] ^ s[13] ^ s[0]
        s.pop(0)
        s.append(b)
        return b

    def bit(self):
        while not self.step():  # a pair (0, x) is dropped, a pair (1, x) gives x
            self.step()
        return self.step()

    def bits(self, n):
        v = 0
        for _ in range(n):
            v = v << 1 | self.bit()
        return v


# ---- polynomials over F_p, coefficients low first, multiplied as packed integers ---------------------------------------------------------
SLOT = 80  # a coefficient of a product of two polynomials of degree < 32 is below 32 * 2^62


def pack(a):
    v = 0
    for c in reversed(a):
        v = v << SLOT | c
    return v


def unpack(v, n, p):
    mask = (1 << SLOT) - 1
    return [(v >> (SLOT * i) & mask) % p for i in range(n)]


class ModPoly:
    """arithmetic modulo a monic f of degree t"""

    def __init__(self, f, p):
        self.f, self.p, self.t = f, p, len(f) - 1
        # x^(t + k) mod f for k < t - 1, packed
        self.high = []
        cur = [(-c) % p for c in f[:-1]]  # x^t
        for _ in range(self.t - 1):
            self.high.append(pack(cur))
            top = cur[-1]
            cur = [(-top * f[0]) % p] + [(cur[i - 1] - top * f[i]) % p for i in range(1, self.t)]

    def mul(self, a, b):
        t, p = self.t, self.p
        c = unpack(pack(a) * pack(b), 2 * t - 1, p)
        v = pack(c[:t])
        for k in range(t - 1):
            if c[t + k]:
                v += c[t + k] * self.high[k]
        return unpack(v, t, p)

    def pow(self, a, e):
        r = None
        for bit in bin(e)[2:]:
            if r is not None:
                r = self.mul(r, r)
            if bit == "1":
                r = a if r is None else self.mul(r, a)
        return r


def poly_trim(a):
    while a and a[-1] == 0:
        a = a[:-1]
    return a


def poly_rem(a, b, p):
    a, inv = list(a), pow(b[-1], -1, p)
    while len(a) >= len(b):
        q = a[-1] * inv % p
        if q:
            off = len(a) - len(b)
            for i, c in enumerate(b):
                a[off + i] = (a[off + i] - q * c) % p
        a.pop()
    return poly_trim(a)


def poly_gcd_is_one(a, b, p):
    a, b = poly_trim(list(a)), poly_trim(list(b))
    while b:
        a, b = b, poly_rem(a, b, p)
    return len(a) == 1


def is_irreducible(f, p):
    """Rabin: monic f of degree t is irreducible iff x^(p^t) = x mod f and gcd(x^(p^(t/q)) - x, f) = 1 for every prime q | t"""
    t = len(f) - 1
    if t == 1:
        return True
    ring = ModPoly(f, p)
    x = [0, 1] + [0] * (t - 2)
    wanted = {t // q for q in range(2, t + 1) if t % q == 0 and all(q % r for r in range(2, q))}
    cur = x
    for k in range(1, t + 1):
        cur = ring.pow(cur, p)  # x^(p^k)
        if k in wanted:
            diff = [(c - d) % p for c, d in zip(cur, x)]
            if not poly_trim(diff) or not poly_gcd_is_one(f, diff, p):
                return False
    return cur == x


def charpoly(m, p):
    """det(x - m), coefficients low first: reduce to upper Hessenberg form by similarity, then the recurrence on leading minors"""
    n = len(m)
    h = [row[:] for row in m]
    for k in range(1, n - 1):
        piv = next((i for i in range(k, n) if h[i][k - 1]), None)
        if piv is None:
            continue
        if piv != k:
            h[k], h[piv] = h[piv], h[k]
            for row in h:
                row[k], row[piv] = row[piv], row[k]
        inv = pow(h[k][k - 1], -1, p)
        for i in range(k + 1, n):
            if h[i][k - 1]:
                c = h[i][k - 1] * inv % p
                h[i] = [(a - c * b) % p for a, b in zip(h[i], h[k])]  # row_i -= c row_k
                for row in h:
                    row[k] = (row[k] + c * row[i]) % p  # col_k += c col_i
    # p_k = (x - h[k-1][k-1]) p_(k-1) - sum_j h[j][k-1] (prod of the subdiagonal between) p_j
    polys = [[1]]
    for k in range(1, n + 1):
        prev = polys[k - 1]
        cur = [0] + prev
        for i, c in enumerate(prev):
            cur[i] = (cur[i] - h[k - 1][k - 1] * c) % p
        sub = 1
        for j in range(k - 2, -1, -1):
            sub = sub * h[j + 1][j] % p
            c = h[j][k - 1] * sub % p
            if c:
                for i, v in enumerate(polys[j]):
                    cur[i] = (cur[i] - c * v) % p
        polys.append(cur)
    return polys[n]


def mat_mul(a, b, p):
    cols = list(zip(*b))
    return [[sum(x * y for x, y in zip(row, col)) % p for col in cols] for row in a]


# ---- parameters ----------------------------------------------------------------------------------------------------------------------
M4 = [[5, 7, 1, 3], [4, 6, 1, 1], [1, 3, 5, 7], [1, 1, 4, 6]]


def external_matrix(t):
    if t == 2:
        return [[2, 1], [1, 2]]
    if t == 3:
        return [[2, 1, 1], [1, 2, 1], [1, 1, 2]]
    if t == 4:
        return [row[:] for row in M4]
    return [[M4[i % 4][j % 4] * (2 if i // 4 == j // 4 else 1) for j in range(t)] for i in range(t)]


def internal_matrix(diag):
    t = len(diag)
    return [[diag[i] if i == j else 1 for j in range(t)] for i in range(t)]


def diagonal_is_good(diag, p):
    t = len(diag)
    m = internal_matrix(diag)
    cur = m
    for i in range(1, 2 * t + 1):
        if not is_irreducible(charpoly(cur, p), p):
            return False
        if i < 2 * t:
            cur = mat_mul(m, cur, p)
    return True


class Params:
    def __init__(self, field, t):
        assert t in WIDTHS
        self.field, self.t, self.p = field, t, FIELDS[field]
        p, n = self.p, self.p.bit_length()
        self.alpha, self.r_f, self.r_p = round_numbers(p, t)
        g = Grain(n, t, self.r_f, self.r_p)
        self.rc = []
        while len(self.rc) < self.r_f * t + self.r_p:
            v = g.bits(n)
            if v < p:
                self.rc.append(v)
        if t == 2:
            self.diag = [2, 3]
        elif t == 3:
            self.diag = [2, 2, 3]
        else:
            while True:
                self.diag = [g.bits(n) % p for _ in range(t)]
                if diagonal_is_good(self.diag, p):
                    break
        self.m_e, self.m_i = external_matrix(t), internal_matrix(self.diag)


@functools.lru_cache(maxsize=None)
def params(field, t):
    return Params(field, t)


# ---- the permutation and the hash --------------------------------------------------------------------------------------------------------
def mat_vec(m, v, p):
    return [sum(a * b for a, b in zip(row, v)) % p for row in m]


def permute(P, state):
    """one external layer, R_F / 2 full rounds, R_P partial rounds, R_F / 2 full rounds"""
    p, t, a = P.p, P.t, P.alpha
    s = mat_vec(P.m_e, state, p)
    at, half = 0, P.r_f // 2
    for r in range(P.r_f + P.r_p):
        if r < half or r >= half + P.r_p:
            s = mat_vec(P.m_e, [pow(x + c, a, p) for x, c in zip(s, P.rc[at:at + t])], p)
            at += t
        else:
            s[0] = pow(s[0] + P.rc[at], a, p)
            s = mat_vec(P.m_i, s, p)
            at += 1
    assert at == len(P.rc)
    return s


def hash_one(field, t, msg, tag=None):
    """One digest (an element) of msg, a list of elements. len(msg) == t (t - 1 with a tag, which then is state[0]): one permutation.
    Any other length is a sponge: the state starts at zero, state[0] is the tag or else the first element, the rest is added into
    state[1 .. t-1], t - 1 elements per permutation; an incomplete last block -- and only that -- is padded with 1, 0, 0, ..; a message
    shorter than t is one permutation. The digest is state[1]."""
    P = params(field, t)
    p = P.p
    msg = list(msg)
    if len(msg) == (t - 1 if tag is not None else t):
        return permute(P, ([tag] if tag is not None else []) + msg)[1]
    state = [0] * t
    if tag is not None:
        state[0] = tag
    else:
        state[0], msg = msg[0], msg[1:]
    blocks = 1 if len(msg) + 1 < t + (tag is not None) else -(-len(msg) // (t - 1))
    # (len(msg) is n - [no tag] here: n < t means one permutation)
    for b in range(blocks):
        chunk = msg[b * (t - 1):(b + 1) * (t - 1)]
        if len(chunk) < t - 1:
            chunk = chunk + [1] + [0] * (t - 2 - len(chunk))
        for i, v in enumerate(chunk):
            state[1 + i] = (state[1 + i] + v) % p
        state = permute(P, state)
    return state[1]


def hash_batch(field, t, elements, size, tag=None):
    """back-to-back messages of `size` elements -> list of digests"""
    assert len(elements) % size == 0
    return [hash_one(field, t, elements[i:i + size], tag) for i in range(0, len(elements), size)]


def merkle_layers(field, leaves, layer_specs):
    """leaves: list of elements; layer_specs: [(t, input elements, tag)] from the leaf layer up -> the list of digest layers"""
    layers, cur = [], list(leaves)
    for t, size, tag in layer_specs:
        cur = hash_batch(field, t, cur, size, tag)
        layers.append(cur)
    return layers
