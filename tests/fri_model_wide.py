"""Test infrastructure: the Python model of FRI over the wide fields -- Goldilocks (8-byte elements), its quadratic extension
(16 bytes, a0 + a1 u with u^2 = 7, constant term first), and the 256-bit scalar fields stark252, BN254, BLS12-381 and BLS12-377
(32 bytes). What does not depend on the field -- transcript, sampler, plan, tree shape, proof of work -- is tests/fri_model.py's;
this file adds the six field kinds over Python integers and the prover and verifier written over a field object. It is checked
byte for byte against proofs of the reference's CPU backend (tests/golden/fri_vectors_wide.json, tests/test_fri_wide_cpu.py).
Elements are tuples of ints, one per coefficient; in bytes every coefficient is little-endian."""
import json
import os

from tests import blake_model as bm
from tests import fri_model as fm

FIELDS = {  # p, two-adicity, root of unity of order 2^two_adicity, bytes of one coefficient
    "goldilocks": (0xFFFFFFFF00000001, 32, 0x185629DCDA58878C, 8),
    "stark252": (0x0800000000000011000000000000000000000000000000000000000000000001, 192,
                 0x005282DB87529CFA3F0464519C8B0FA5AD187148E11A61616070024F42F8EF94, 32),
    "bn254": (0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001, 28,
              0x2A3C09F0A58A7E8500E0A7EB8EF62ABC402D111E41112ED49BD61B6E725B19F0, 32),
    "bls12_381": (0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001, 32,
                  0x0212D79E5B416B6F0FD56DC8D168D6C0C4024FF270B3E0941B788F500B912F1F, 32),
    "bls12_377": (0x12AB655E9A2CA55660B44D1E5C37B00159AA76FED00000010A11800000000001, 47,
                  0x11D4B7F60CB92CC160C69477D1A8A12F9B506EE363E3F04A476EF4A4EC2A895E, 32),
}
EXT_NONRESIDUE = 7  # Goldilocks only: F[u] / (u^2 - 7)
KINDS = [("goldilocks", False), ("goldilocks", True), ("stark252", False), ("bn254", False), ("bls12_381", False), ("bls12_377", False)]


def prefix(field, extension):
    return f"{field}_extension" if extension else field


class Field:
    def __init__(self, name, extension=False):
        assert not extension or name == "goldilocks", "only Goldilocks has an extension among the wide fields"
        self.name, self.ext = name, extension
        self.p, self.two_adicity, self.rou, self.coeff_bytes = FIELDS[name]
        self.coeffs = 2 if extension else 1
        self.bytes = self.coeff_bytes * self.coeffs
        self.words = self.bytes // 4  # uint32 words of one element in memory

    def omega(self, logn):
        return pow(self.rou, 1 << (self.two_adicity - logn), self.p)

    def add(self, a, b):
        return tuple((x + y) % self.p for x, y in zip(a, b))

    def sub(self, a, b):
        return tuple((x - y) % self.p for x, y in zip(a, b))

    def scale(self, a, s):
        return tuple(x * s % self.p for x in a)

    def mul(self, a, b):
        if not self.ext:
            return (a[0] * b[0] % self.p,)
        return ((a[0] * b[0] + EXT_NONRESIDUE * a[1] * b[1]) % self.p, (a[0] * b[1] + a[1] * b[0]) % self.p)

    def to_bytes(self, a):
        return b"".join(x.to_bytes(self.coeff_bytes, "little") for x in a)

    def from_bytes(self, b):
        return tuple(int.from_bytes(b[self.coeff_bytes * k:self.coeff_bytes * (k + 1)], "little") for k in range(self.coeffs))

    def from_digest(self, d):
        """a scalar: the whole digest as one little-endian integer mod p; the extension: coefficient k from bytes 8k .. 8k+7 mod p"""
        if not self.ext:
            return (int.from_bytes(d, "little") % self.p,)
        return tuple(int.from_bytes(d[8 * k:8 * k + 8], "little") % self.p for k in range(2))

    def fold1(self, lo, hi, alpha, tw):
        """(lo + hi)/2 + alpha * ((lo - hi)/2 * tw) for one pair; tw an integer"""
        half = (self.p + 1) // 2
        return self.add(self.scale(self.add(lo, hi), half), self.mul(alpha, self.scale(self.sub(lo, hi), half * tw % self.p)))

    def fold(self, layer, alpha):
        n = len(layer)
        h = n // 2
        w_inv = pow(self.omega(n.bit_length() - 1), self.p - 2, self.p)
        out, tw = [], 1
        for i in range(h):
            out.append(self.fold1(layer[i], layer[i + h], alpha, tw))
            tw = tw * w_inv % self.p
        return out

    def elements(self, raw: bytes):
        return [self.from_bytes(raw[i:i + self.bytes]) for i in range(0, len(raw), self.bytes)]

    def raw(self, elements):
        return b"".join(self.to_bytes(e) for e in elements)


def prove(F, data, transcript_hasher, labels, public_state, seed, leaves_hash, compress_hash, stopping_degree, pow_bits, nof_queries):
    """fri_model.prove over a field object: data a list of element tuples, seed an element tuple"""
    logn, rounds, final_size = fm.plan(len(data), stopping_degree, nof_queries)
    tr = fm.Transcript(transcript_hasher, labels, public_state, logn)
    layers, shapes, raw, prev = [list(data)], [], [], F.to_bytes(seed)
    for r in range(rounds):
        shapes.append(fm.tree_shape(F, leaves_hash, compress_hash, len(layers[r])))
        raw.append(F.raw(layers[r]))
        root = bm.build(shapes[r], raw[r])[-1]
        alpha = F.from_digest(tr.hash(tr.round_input(prev, root)))
        prev = F.to_bytes(alpha)
        layers.append(F.fold(layers[r], alpha))
    nonce = fm.pow_solve(transcript_hasher, tr.pow_challenge(prev), pow_bits) if pow_bits else 0
    seed32 = int.from_bytes(tr.hash(tr.query_input(pow_bits != 0, prev, nonce))[:4], "little")
    queries = fm.draw_queries(seed32, nof_queries, final_size, len(data))
    slots = []
    for q in queries:
        for sym in (0, 1):
            row = []
            for r in range(rounds):
                size = len(layers[r])
                idx = (q + sym * size // 2) % size
                leaf, path, root = bm.proof(shapes[r], raw[r], idx, False)
                row.append((idx, leaf, root, path))
            slots.append(row)
    return {"final_poly": layers[-1], "nonce": nonce, "queries": queries, "slots": slots}


def verify(F, proof, transcript_hasher, labels, public_state, seed, leaves_hash, compress_hash, stopping_degree, pow_bits, nof_queries):
    """fri_model.verify over a field object, and one rule more: a coefficient at or above p makes a wrong proof"""
    final_poly, slots = proof["final_poly"], proof["slots"]
    if len(final_poly) != stopping_degree + 1 or any(c >= F.p for e in final_poly for c in e):
        return False
    rounds = len(slots[0])
    n = len(final_poly) << rounds
    if fm.plan(n, stopping_degree, nof_queries) is None or len(slots) != 2 * nof_queries:
        return False
    if any(row[r][2] != slots[0][r][2] for row in slots for r in range(rounds)):
        return False  # one root per round
    logn = n.bit_length() - 1
    tr = fm.Transcript(transcript_hasher, labels, public_state, logn)
    prev, alphas = F.to_bytes(seed), []
    for r in range(rounds):
        alphas.append(F.from_digest(tr.hash(tr.round_input(prev, slots[0][r][2]))))
        prev = F.to_bytes(alphas[-1])
    if pow_bits and fm.pow_candidate(transcript_hasher, tr.pow_challenge(prev), proof["nonce"]) >= 1 << (64 - pow_bits):
        return False
    seed32 = int.from_bytes(tr.hash(tr.query_input(pow_bits != 0, prev, proof["nonce"]))[:4], "little")
    queries = fm.draw_queries(seed32, nof_queries, len(final_poly), n)
    w_inv = pow(F.omega(logn), F.p - 2, F.p)
    for j, q in enumerate(queries):
        for r in range(rounds):
            size = n >> r
            shape = fm.tree_shape(F, leaves_hash, compress_hash, size)
            (ia, la, ra, pa), (ib, lb, rb, pb) = slots[2 * j][r], slots[2 * j + 1][r]
            if len(la) != F.bytes or len(lb) != F.bytes:
                return False
            if not (bm.verify(shape, la, ia, pa, ra, False) and bm.verify(shape, lb, ib, pb, rb, False)):
                return False
            if ia != q % size or ib != (q + size // 2) % size:
                return False
            a, b = F.from_bytes(la), F.from_bytes(lb)
            if any(c >= F.p for c in a + b):
                return False
            folded = F.fold1(a, b, alphas[r], pow(w_inv, ia << r, F.p))
            want = final_poly[q % len(final_poly)] if r + 1 == rounds else F.from_bytes(slots[2 * j][r + 1][1])
            if tuple(want) != folded:
                return False
    return True


# ---- the fixtures (tests/golden/fri_vectors_wide.json) -------------------------------------------------------------------------------
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fri_vectors_wide.json")


def load_fixtures():
    with open(FIXTURE) as f:
        return json.load(f)["cases"]


def case_field(case):
    return Field(case["field"], case["extension"])


def case_elements(case, key="input"):
    """input, final_poly and seed are hex strings of the elements' bytes back to back"""
    return case_field(case).elements(bytes.fromhex(case[key]))


def case_protocol(case):
    """the arguments prove() and verify() share, after the data / the proof"""
    return (case["transcript_hash"], tuple(s.encode() for s in case["labels"]), bytes.fromhex(case["public_state"]), case_elements(case, "seed")[0], case["leaves_hash"],
            case["compress_hash"], case["stopping_degree"], case["pow_bits"], case["nof_queries"])


def case_proof(case):
    """the fixture's proof in the model's form"""
    slots = [[(s["leaf_idx"], bytes.fromhex(s["leaf"]), bytes.fromhex(s["root"]), bytes.fromhex(s["path"])) for s in row] for row in case["slots"]]
    return {"final_poly": case_elements(case, "final_poly"), "nonce": case["nonce"], "slots": slots}
