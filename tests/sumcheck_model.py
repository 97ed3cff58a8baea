"""Python model of sumcheck as the reference's CPU backend computes it (backend/cpu/include/cpu_sumcheck.h, include/icicle/sumcheck/
sumcheck.h, sumcheck_transcript.h, include/icicle/program/*.h): programs with their degree and variable count, the transcript bytes,
the prover and the verifier. Elements are Python ints; tests/golden/sumcheck_vectors.json holds the reference's own proofs, and
tests/golden/sumcheck_vectors_large.json those of LARGE_CASES, whose inputs large_inputs() makes again from a seed (NumPy arrays)."""
import hashlib
import json
import os

import numpy as np

from tests import blake_model as bm

FIELDS = {  # p, words of an element
    "babybear": (0x78000001, 1),
    "koalabear": (0x7F000001, 1),
    "bn254": (0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001, 8),
    "bls12_381": (0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001, 8),
}
AB_MINUS_C, EQ_X_AB_MINUS_C = 0, 1
MAX_DEGREE, MAX_POLYS, MAX_VARS = 6, 8, 20


def to_bytes(field, v):
    return int(v).to_bytes(4 * FIELDS[field][1], "little")


def le32(v):
    return int(v).to_bytes(4, "little")


def from_digest(field, digest):
    """F(digest): the whole digest as one little-endian integer, mod p"""
    return int.from_bytes(digest, "little") % FIELDS[field][0]


class Program:
    """A combine function. `nodes`: a list in which node j is ["in", i], ["const", value] or [op, a, b] / ["inv", a] with op in add, sub,
    mul and a, b indices of earlier nodes; the last node is the return value. Or one of the two predefined programs."""

    def __init__(self, nof_inputs, nodes=None, predefined=None):
        self.nof_inputs, self.nodes, self.predefined = nof_inputs, nodes, predefined

    @classmethod
    def from_description(cls, d):
        if "predefined" in d:
            return cls({AB_MINUS_C: 3, EQ_X_AB_MINUS_C: 4}[d["predefined"]], predefined=d["predefined"])
        return cls(d["nof_inputs"], [[n[0]] + [int(v, 16) if n[0] == "const" else v for v in n[1:]] for n in d["nodes"]])

    def description(self):
        if self.predefined is not None:
            return {"predefined": self.predefined}
        return {"nof_inputs": self.nof_inputs, "nodes": [[n[0]] + [f"{v:x}" if n[0] == "const" else v for v in n[1:]] for n in self.nodes]}

    def _reachable(self):
        seen, stack = set(), [len(self.nodes) - 1]
        while stack:
            j = stack.pop()
            if j not in seen:
                seen.add(j)
                if self.nodes[j][0] not in ("in", "const"):
                    stack += self.nodes[j][1:]
        return seen

    def degree(self):
        """input 1, constant 0, add / sub the larger, multiply the sum, inverse -1 (and -1 wherever it is used)"""
        if self.predefined is not None:
            return {AB_MINUS_C: 2, EQ_X_AB_MINUS_C: 3}[self.predefined]
        deg = []
        for n in self.nodes:
            ops = [deg[a] for a in n[1:]] if n[0] not in ("in", "const") else []
            if n[0] == "in":
                deg.append(1)
            elif n[0] == "const":
                deg.append(0)
            elif n[0] == "inv" or min(ops) < 0:
                deg.append(-1)
            else:
                deg.append(sum(ops) if n[0] == "mul" else max(ops))
        return deg[-1]

    def nof_vars(self):
        """parameters + constants + one per operation node; the return value's node takes the output parameter's slot"""
        if self.predefined is not None:
            return self.nof_inputs + 1
        kinds = [self.nodes[j][0] for j in self._reachable()]
        ops = sum(k not in ("in", "const") for k in kinds)
        return self.nof_inputs + 1 + kinds.count("const") + ops - (self.nodes[-1][0] not in ("in", "const"))

    def evaluate(self, p, x):
        if self.predefined == AB_MINUS_C:
            return (x[0] * x[1] - x[2]) % p
        if self.predefined == EQ_X_AB_MINUS_C:
            return x[3] * (x[0] * x[1] - x[2]) % p
        v = []
        for n in self.nodes:
            if n[0] == "in":
                v.append(x[n[1]])
            elif n[0] == "const":
                v.append(n[1] % p)
            elif n[0] == "inv":
                v.append(pow(v[n[1]], p - 2, p))
            else:
                a, b = v[n[1]], v[n[2]]
                v.append((a + b if n[0] == "add" else a - b if n[0] == "sub" else a * b) % p)
        return v[-1]


def acceptable(program, nof_polys):
    d = program.degree()
    return nof_polys == program.nof_inputs and nof_polys <= MAX_POLYS and 1 <= d <= MAX_DEGREE and program.nof_vars() <= MAX_VARS


class Transcript:
    """Every u32 little-endian, a field element its canonical bytes. labels: (domain separator, round polynomial, round challenge)."""

    def __init__(self, field, hasher, labels, seed, rounds, degree, claimed_sum):
        self.field, self.hasher, self.degree = field, hasher, degree
        self.ds, self.poly, self.challenge = labels
        self.entry0 = self.poly + le32(degree + 1) + le32(0)
        # the first u32 is the number of rounds (the reference's argument is named mle_polynomial_size)
        self.head = self.ds + le32(rounds) + le32(degree) + to_bytes(field, claimed_sum) + to_bytes(field, seed) + self.challenge

    def round_input(self, r, alpha, round_poly):
        evals = b"".join(to_bytes(self.field, v) for v in round_poly)
        if r == 0:
            return self.head + evals + self.entry0  # R_0 before entry0, not inside it
        return self.entry0 + to_bytes(self.field, alpha) + self.challenge + self.poly + le32(self.degree + 1) + le32(r) + evals

    def alpha(self, r, prev_alpha, round_poly):
        return from_digest(self.field, bm.digest(self.hasher, self.round_input(r, prev_alpha, round_poly)))


def round_poly(p, program, tables, degree):
    out = [0] * (degree + 1)
    m = len(tables)
    for i in range(len(tables[0]) // 2):
        x = [t[2 * i] for t in tables]
        dx = [(t[2 * i + 1] - t[2 * i]) % p for t in tables]
        for k in range(degree + 1):
            out[k] += program.evaluate(p, x)
            x = [(x[j] + dx[j]) % p for j in range(m)]
    return [v % p for v in out]


def prove(field, polys, claimed_sum, program, hasher, labels, seed):
    """polys: lists of 2^L ints -> {"round_polys": L lists of d + 1 ints, "challenges": [0, alpha_1, ..]}"""
    p = FIELDS[field][0]
    n = len(polys[0])
    rounds, d = n.bit_length() - 1, program.degree()
    assert n >= 2 and n == 1 << rounds and acceptable(program, len(polys))
    tr = Transcript(field, hasher, labels, seed, rounds, d, claimed_sum)
    tables, rps, alphas = [list(t) for t in polys], [], []
    for r in range(rounds):
        alpha = tr.alpha(r - 1, alphas[-1], rps[-1]) if r else 0
        alphas.append(alpha)
        if r:  # adjacent elements: the low variable is bound first
            tables = [[(t[2 * j] + alpha * (t[2 * j + 1] - t[2 * j])) % p for j in range(len(t) // 2)] for t in tables]
        rps.append(round_poly(p, program, tables, d))
    return {"round_polys": rps, "challenges": alphas}


def lagrange(p, evals, x):
    total = 0
    for i, y in enumerate(evals):
        num, den = y, 1
        for j in range(len(evals)):
            if j != i:
                num, den = num * (x - j) % p, den * (i - j) % p
        total += num * pow(den, p - 2, p)
    return total % p


def verify(field, round_polys, claimed_sum, hasher, labels, seed):
    p = FIELDS[field][0]
    rounds = len(round_polys)
    if rounds == 0 or len({len(r) for r in round_polys}) != 1 or not 2 <= len(round_polys[0]) <= MAX_DEGREE + 1:
        return False
    if any(not 0 <= v < p for r in round_polys for v in r):
        return False
    if (round_polys[0][0] + round_polys[0][1]) % p != claimed_sum % p:
        return False
    tr = Transcript(field, hasher, labels, seed, rounds, len(round_polys[0]) - 1, claimed_sum)
    alpha = 0
    for r in range(rounds - 1):  # the last round polynomial is not checked against anything
        alpha = tr.alpha(r, alpha, round_polys[r])
        if lagrange(p, round_polys[r], alpha) != (round_polys[r + 1][0] + round_polys[r + 1][1]) % p:
            return False
    return True


def claimed_sum(field, polys, program):
    p = FIELDS[field][0]
    return sum(program.evaluate(p, [t[i] for t in polys]) for i in range(len(polys[0]))) % p


# ---- the fixtures (tests/golden/sumcheck_vectors.json) --------------------------------------------------------------------------------
def load_fixtures():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sumcheck_vectors.json")) as f:
        return json.load(f)["cases"]


def unhex(rows):
    return [[int(v, 16) for v in row] for row in rows]


def case_labels(case):
    return tuple(s.encode() for s in case["labels"])


# ---- the large cases (tests/golden/sumcheck_vectors_large.json): inputs from a seed, recorded by their sha256 -------------------------
# t = x0 + 5 used twice, and two more constants: (t t x1 - 7 t) + 0x77ffffff x2
CONSTANTS = Program(3, [["in", 0], ["in", 1], ["in", 2], ["const", 5], ["add", 0, 3], ["mul", 4, 4], ["mul", 5, 1], ["const", 7], ["mul", 7, 4], ["sub", 6, 8],
                        ["const", 0x77FFFFFF], ["mul", 10, 2], ["add", 9, 11]])
LARGE_LABELS = ["domain_separator_label", "round_poly_label", "round_challenge_label"]
# name, field, program, L, input seed, the rounds that walk: the smallest sizes at which a round launch without a forced cap (2048 blocks
# of 128 lanes, of 64 for a user program) walks its grid a second time. Round 1 of bn254_eq_l20 has 2^18 pairs, exactly one full grid.
LARGE_CASES = [
    ("bb_eq_l21", "babybear", Program(4, predefined=EQ_X_AB_MINUS_C), 21, 2101, (0, 1)),
    ("bn254_eq_l20", "bn254", Program(4, predefined=EQ_X_AB_MINUS_C), 20, 2102, (0,)),
    ("bb_constants_l20", "babybear", CONSTANTS, 20, 2103, (0, 1)),
]


def round_items(field, predefined, L, r):
    """what the lanes of round r's launch share out among them: the pairs of T_r, n / 2^(r+1) -- but half as many in round 0 of a predefined
    program over a one-word field, where a lane takes two pairs with one 16-byte load"""
    pairs = (1 << L) >> (r + 1)
    return pairs // 2 if predefined and FIELDS[field][1] == 1 and r == 0 and pairs > 1 else pairs


def large_inputs(field, nof_polys, n, seed):
    """nof_polys uint32 arrays [n] (one word) or [n, 8] of uniform canonical elements from one generator, without a Python loop over the
    elements; then polys[0][0] = 0 and polys[-1][-1] = p - 1. The mint script and the tests share it."""
    p, w = FIELDS[field]
    rng = np.random.default_rng(seed)
    polys = []
    for _ in range(nof_polys):
        if w == 1:
            polys.append(rng.integers(0, p, n, dtype=np.uint32))
        else:
            a = rng.integers(0, 1 << 32, size=(n, w), dtype=np.uint32)
            a[:, w - 1] %= np.uint32(p >> (32 * (w - 1)))  # top word below p's top word: the value is below p
            polys.append(a)
    polys[0][0] = 0
    polys[-1][-1] = p - 1 if w == 1 else np.array([((p - 1) >> (32 * i)) & 0xFFFFFFFF for i in range(w)], dtype=np.uint32)
    return polys


def sha256_of(arrays):
    return [hashlib.sha256(np.ascontiguousarray(a, dtype="<u4").tobytes()).hexdigest() for a in arrays]


def ints_of_array(a, w):
    """a uint32 array [n] or [n, w] as Python ints"""
    if w == 1:
        return [int(v) for v in a.tolist()]
    raw = np.ascontiguousarray(a, dtype="<u4").tobytes()
    return [int.from_bytes(raw[i:i + 4 * w], "little") for i in range(0, len(raw), 4 * w)]


def claimed_sum_u64(p, polys, program):
    """sum of program(polys[..][i]) mod p for p < 2^31 in uint64 arithmetic: every product of two reduced values fits in 64 bits"""
    assert p < 1 << 31
    P = np.uint64(p)
    x = [np.asarray(t, dtype=np.uint64) for t in polys]
    if program.predefined is not None:
        g = (x[0] * x[1] % P + P - x[2]) % P
        if program.predefined == EQ_X_AB_MINUS_C:
            g = g * x[3] % P
    else:
        v = []
        for n in program.nodes:
            if n[0] == "in":
                v.append(x[n[1]])
            elif n[0] == "const":
                v.append(np.uint64(n[1] % p))
            else:
                a, b = v[n[1]], v[n[2]]
                v.append((a + b if n[0] == "add" else a + P - b if n[0] == "sub" else a * b) % P)
        g = v[-1]
    return int(g.sum(dtype=np.uint64) % P)  # fewer than 2^33 terms below 2^31


def load_large_fixtures():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sumcheck_vectors_large.json")) as f:
        return json.load(f)["cases"]
