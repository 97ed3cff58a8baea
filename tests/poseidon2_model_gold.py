"""Poseidon2 over Goldilocks, p = 2^64 - 2^32 + 1, in Python integers: the parameter derivation, the hash and a Merkle tree over it.

The derivation is that of tests/poseidon2_model.py, whose parts that depend on p only through its bit length, log2 p and alpha
(alpha_of, round_numbers, Grain) or not at all (charpoly, mat_mul, the matrices, permute) are imported. What is its own here is
the polynomial arithmetic of the irreducibility test: that model packs coefficients into slots of 80 bits, and a coefficient of a
product of two polynomials of degree < 32 over this field reaches 32 * 2^128, so the slot here is 144 bits. Written independently of
icicle_amd/csrc/poseidon2_gold_params.h and poseidon2_gold.hpp, with other means where there is a choice: both linear layers are
dense matrix-vector products, the characteristic polynomial comes from the Hessenberg form (the C++ takes the Krylov sequence of
a vector), polynomials are multiplied as packed integers and x^(p^k) is found by repeated exponentiation (the C++ applies the
matrix of the Frobenius map).

Elements travel as 8 little-endian bytes. tests/golden/poseidon2_vectors_gold.json holds digests of the reference, which prove
this model and the library.
"""
import functools

from tests import poseidon2_model as m31

P = (1 << 64) - (1 << 32) + 1
WIDTHS = (2, 3, 4, 8, 12, 16, 20, 24)
ES = 8  # bytes of an element
# alpha and (R_F, R_P) per width as the reference's table states them
EXPECTED_ALPHA = 7
EXPECTED_ROUNDS = {2: (8, 27), 3: (8, 23), 4: (8, 21), 8: (8, 22), 12: (8, 22), 16: (8, 22), 20: (8, 22), 24: (8, 22)}

# ---- polynomials over F_p, coefficients low first, multiplied as packed integers ---------------------------------------------------------
SLOT = 144  # a coefficient of a product of two polynomials of degree < 32 is below 32 * 2^128, and the reduction adds 31 more such


def pack(a):
    v = 0
    for c in reversed(a):
        v = v << SLOT | c
    return v


def unpack(v, n):
    mask = (1 << SLOT) - 1
    return [(v >> (SLOT * i) & mask) % P for i in range(n)]


class ModPoly:
    """arithmetic modulo a monic f of degree t"""

    def __init__(self, f):
        self.f, self.t = f, len(f) - 1
        self.high = []  # x^(t + k) mod f for k < t - 1, packed
        cur = [(-c) % P for c in f[:-1]]
        for _ in range(self.t - 1):
            self.high.append(pack(cur))
            top = cur[-1]
            cur = [(-top * f[0]) % P] + [(cur[i - 1] - top * f[i]) % P for i in range(1, self.t)]

    def mul(self, a, b):
        t = self.t
        c = unpack(pack(a) * pack(b), 2 * t - 1)
        v = pack(c[:t])
        for k in range(t - 1):
            if c[t + k]:
                v += c[t + k] * self.high[k]
        return unpack(v, t)

    def pow(self, a, e):
        r = None
        for bit in bin(e)[2:]:
            if r is not None:
                r = self.mul(r, r)
            if bit == "1":
                r = a if r is None else self.mul(r, a)
        return r


def is_irreducible(f):
    """Rabin: monic f of degree t is irreducible iff x^(p^t) = x mod f and gcd(x^(p^(t/q)) - x, f) = 1 for every prime q | t"""
    t = len(f) - 1
    ring = ModPoly(f)
    x = [0, 1] + [0] * (t - 2)
    wanted = {t // q for q in range(2, t + 1) if t % q == 0 and all(q % r for r in range(2, q))}
    cur = x
    for k in range(1, t + 1):
        cur = ring.pow(cur, P)  # x^(p^k)
        if k in wanted:
            diff = [(c - d) % P for c, d in zip(cur, x)]
            if not m31.poly_trim(diff) or not m31.poly_gcd_is_one(f, diff, P):
                return False
    return cur == x


def diagonal_is_good(diag):
    t = len(diag)
    m = m31.internal_matrix(diag)
    cur = m
    for i in range(1, 2 * t + 1):
        if not is_irreducible(m31.charpoly(cur, P)):
            return False
        if i < 2 * t:
            cur = m31.mat_mul(m, cur, P)
    return True


class Params:
    """the attributes m31.permute reads: p, t, alpha, r_f, r_p, rc, m_e, m_i; `draws` counts the diagonals tried"""

    def __init__(self, t):
        assert t in WIDTHS
        self.t, self.p = t, P
        n = P.bit_length()
        self.alpha, self.r_f, self.r_p = m31.round_numbers(P, t)
        g = m31.Grain(n, t, self.r_f, self.r_p)
        self.rc = []
        while len(self.rc) < self.r_f * t + self.r_p:
            v = g.bits(n)
            if v < P:
                self.rc.append(v)
        self.draws = 0
        if t == 2:
            self.diag = [2, 3]
        elif t == 3:
            self.diag = [2, 2, 3]
        else:
            while True:
                self.diag = [g.bits(n) % P for _ in range(t)]
                self.draws += 1
                if diagonal_is_good(self.diag):
                    break
        self.m_e, self.m_i = m31.external_matrix(t), m31.internal_matrix(self.diag)


@functools.lru_cache(maxsize=None)
def params(t):
    return Params(t)


# ---- the hash -----------------------------------------------------------------------------------------------------------------------
def hash_one(t, msg, tag=None):
    """One digest (an element) of msg, a list of elements; the semantics tests/poseidon2_model.py states at its hash_one. An element
    in [p, 2^64) counts as its residue."""
    Q = params(t)
    msg = [v % P for v in msg]
    if len(msg) == (t - 1 if tag is not None else t):
        return m31.permute(Q, ([tag] if tag is not None else []) + msg)[1]
    state = [0] * t
    if tag is not None:
        state[0] = tag
    else:
        state[0], msg = msg[0], msg[1:]
    blocks = 1 if len(msg) + 1 < t + (tag is not None) else -(-len(msg) // (t - 1))
    for b in range(blocks):
        chunk = msg[b * (t - 1):(b + 1) * (t - 1)]
        if len(chunk) < t - 1:
            chunk = chunk + [1] + [0] * (t - 2 - len(chunk))
        for i, v in enumerate(chunk):
            state[1 + i] = (state[1 + i] + v) % P
        state = m31.permute(Q, state)
    return state[1]


def hash_batch(t, elements, size, tag=None):
    """back-to-back messages of `size` elements -> list of digests"""
    assert len(elements) % size == 0
    return [hash_one(t, elements[i:i + size], tag) for i in range(0, len(elements), size)]


def merkle_layers(leaves, layer_specs):
    """leaves: list of elements (already padded); layer_specs: [(t, input elements, tag)] from the leaf layer up -> the digest layers"""
    layers, cur = [], list(leaves)
    for t, size, tag in layer_specs:
        cur = hash_batch(t, cur, size, tag)
        layers.append(cur)
    return layers


def to_bytes(values):
    return b"".join(int(v).to_bytes(ES, "little") for v in values)


def from_bytes(raw):
    raw = bytes(raw)
    assert len(raw) % ES == 0
    return [int.from_bytes(raw[i:i + ES], "little") for i in range(0, len(raw), ES)]
