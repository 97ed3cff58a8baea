"""Poseidon2 over the 256-bit scalar fields (BN254, BLS12-381, BLS12-377, Grumpkin, stark252) in Python integers: the parameter
derivation, the hash and a Merkle tree over it.

The derivation is that of tests/poseidon2_model.py, whose parts that depend on p only through its bit length, log2 p and alpha
(alpha_of, round_numbers, Grain) or not at all (charpoly, mat_mul, the matrices, permute) are imported. What is its own here is
the polynomial arithmetic of the irreducibility test: that model packs coefficients into slots of 80 bits, which a product of two
256-bit residues does not fit. Written independently of icicle_amd/csrc/poseidon2_wide_params.h and poseidon2_wide.hpp, with other
means where there is a choice (dense matrices, the Hessenberg form, packed integers, x^(p^k) by repeated exponentiation).

Elements travel as 32 little-endian bytes. tests/golden/poseidon2_vectors_wide.json holds digests of the reference, which prove
this model and the library.
"""
import functools

from tests import poseidon2_model as m31

FIELDS = {
    "bn254": 21888242871839275222246405745257275088548364400416034343698204186575808495617,
    "bls12_381": 52435875175126190479447740508185965837690552500527637822603658699938581184513,
    "bls12_377": 8444461749428370424248824938781546531375899335154063827935233455917409239041,
    "grumpkin": 21888242871839275222246405745257275088696311157297823662689037894645226208583,
    "stark252": 0x800000000000011000000000000000000000000000000000000000000000001,
}
WIDTHS = (2, 3, 4, 8)
ES = 32  # bytes of an element
# alpha, R_F, R_P per width as the reference's tables state them
EXPECTED_ROUNDS = {
    "bn254": (5, 8, (56, 56, 56, 57)), "grumpkin": (5, 8, (56, 56, 56, 57)), "bls12_381": (5, 8, (56, 56, 56, 57)),
    "bls12_377": (11, 8, (37, 37, 37, 37)), "stark252": (3, 8, (83, 83, 84, 84)),
}

# ---- polynomials over F_p, coefficients low first, multiplied as packed integers ---------------------------------------------------------
SLOT = 528  # a coefficient of a product of two polynomials of degree < 8 is below 8 * 2^512, and the reduction adds 7 more such


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
        self.high = []  # x^(t + k) mod f for k < t - 1, packed
        cur = [(-c) % p for c in f[:-1]]
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


def is_irreducible(f, p):
    """Rabin: monic f of degree t is irreducible iff x^(p^t) = x mod f and gcd(x^(p^(t/q)) - x, f) = 1 for every prime q | t"""
    t = len(f) - 1
    ring = ModPoly(f, p)
    x = [0, 1] + [0] * (t - 2)
    wanted = {t // q for q in range(2, t + 1) if t % q == 0 and all(q % r for r in range(2, q))}
    cur = x
    for k in range(1, t + 1):
        cur = ring.pow(cur, p)  # x^(p^k)
        if k in wanted:
            diff = [(c - d) % p for c, d in zip(cur, x)]
            if not m31.poly_trim(diff) or not m31.poly_gcd_is_one(f, diff, p):
                return False
    return cur == x


def diagonal_is_good(diag, p):
    t = len(diag)
    m = m31.internal_matrix(diag)
    cur = m
    for i in range(1, 2 * t + 1):
        if not is_irreducible(m31.charpoly(cur, p), p):
            return False
        if i < 2 * t:
            cur = m31.mat_mul(m, cur, p)
    return True


class Params:
    """the attributes m31.permute reads: p, t, alpha, r_f, r_p, rc, m_e, m_i; `draws` counts the diagonals tried"""

    def __init__(self, field, t):
        assert t in WIDTHS
        self.field, self.t, self.p = field, t, FIELDS[field]
        p, n = self.p, self.p.bit_length()
        self.alpha, self.r_f, self.r_p = m31.round_numbers(p, t)
        g = m31.Grain(n, t, self.r_f, self.r_p)
        self.rc = []
        while len(self.rc) < self.r_f * t + self.r_p:
            v = g.bits(n)
            if v < p:
                self.rc.append(v)
        self.draws = 0
        if t == 2:
            self.diag = [2, 3]
        elif t == 3:
            self.diag = [2, 2, 3]
        else:
            while True:
                self.diag = [g.bits(n) % p for _ in range(t)]
                self.draws += 1
                if diagonal_is_good(self.diag, p):
                    break
        self.m_e, self.m_i = m31.external_matrix(t), m31.internal_matrix(self.diag)


@functools.lru_cache(maxsize=None)
def params(field, t):
    return Params(field, t)


# ---- the hash -----------------------------------------------------------------------------------------------------------------------
def hash_one(field, t, msg, tag=None):
    """One digest (an element) of msg, a list of elements; the semantics tests/poseidon2_model.py states at its hash_one."""
    P = params(field, t)
    p = P.p
    msg = list(msg)
    if len(msg) == (t - 1 if tag is not None else t):
        return m31.permute(P, ([tag] if tag is not None else []) + msg)[1]
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
            state[1 + i] = (state[1 + i] + v) % p
        state = m31.permute(P, state)
    return state[1]


def hash_batch(field, t, elements, size, tag=None):
    """back-to-back messages of `size` elements -> list of digests"""
    assert len(elements) % size == 0
    return [hash_one(field, t, elements[i:i + size], tag) for i in range(0, len(elements), size)]


def merkle_layers(field, leaves, layer_specs):
    """leaves: list of elements (already padded); layer_specs: [(t, input elements, tag)] from the leaf layer up -> the digest layers"""
    layers, cur = [], list(leaves)
    for t, size, tag in layer_specs:
        cur = hash_batch(field, t, cur, size, tag)
        layers.append(cur)
    return layers


def to_bytes(values):
    return b"".join(int(v).to_bytes(ES, "little") for v in values)


def from_bytes(raw):
    raw = bytes(raw)
    assert len(raw) % ES == 0
    return [int.from_bytes(raw[i:i + ES], "little") for i in range(0, len(raw), ES)]
