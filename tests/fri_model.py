"""Test infrastructure: a pure-Python model of the FRI prover and verifier over BabyBear and KoalaBear (scalar and quartic
extension), on top of the hash and Merkle models (tests/merkle_model.py, tests/blake_model.py).

It states the protocol of include/icicle_hip.h in the plainest form -- Python integers, one hash at a time -- and is checked byte
for byte against proofs of the reference's CPU backend (tests/golden/fri_vectors.json, tests/test_fri_cpu.py). Elements are ints
(scalar) or 4-tuples of ints, constant coefficient first; in bytes every word is little-endian."""
from tests import blake_model as bm

FIELDS = {  # p, W of F[x] / (x^4 - W), two-adicity, root of unity of order 2^two_adicity
    "babybear": (0x78000001, 11, 27, 0x89),
    "koalabear": (0x7F000001, 3, 24, 0x6AC49F88),
}


class Field:
    def __init__(self, name, extension):
        self.name, self.ext = name, extension
        self.p, self.w, self.two_adicity, self.rou = FIELDS[name]
        self.words = 4 if extension else 1
        self.bytes = 4 * self.words

    def omega(self, logn):
        return pow(self.rou, 1 << (self.two_adicity - logn), self.p)

    # elements are always handled as tuples of `words` ints inside the model
    def add(self, a, b):
        return tuple((x + y) % self.p for x, y in zip(a, b))

    def sub(self, a, b):
        return tuple((x - y) % self.p for x, y in zip(a, b))

    def scale(self, a, s):
        return tuple(x * s % self.p for x in a)

    def mul(self, a, b):
        r = [0] * self.words
        for i, x in enumerate(a):
            for j, y in enumerate(b):
                t = x * y * (self.w if i + j >= self.words else 1)
                r[(i + j) % self.words] = (r[(i + j) % self.words] + t) % self.p
        return tuple(r)

    def to_bytes(self, a):
        return b"".join(x.to_bytes(4, "little") for x in a)

    def from_bytes(self, b):
        return tuple(int.from_bytes(b[4 * k:4 * k + 4], "little") for k in range(self.words))

    def from_digest(self, d):
        if not self.ext:
            return (int.from_bytes(d, "little") % self.p,)
        return tuple(int.from_bytes(d[4 * k:4 * k + 4], "little") % self.p for k in range(4))

    def fold(self, layer, alpha):
        """layer: list of n element tuples -> n / 2, with w_n^(-i) from the field's root of unity (any domain holds the same powers)"""
        n = len(layer)
        h, half = n // 2, (self.p + 1) // 2
        w_inv = pow(self.omega(n.bit_length() - 1), self.p - 2, self.p)
        out, tw = [], 1
        for i in range(h):
            even = self.scale(self.add(layer[i], layer[i + h]), half)
            odd = self.scale(self.sub(layer[i], layer[i + h]), half * tw % self.p)
            out.append(self.add(even, self.mul(alpha, odd)))
            tw = tw * w_inv % self.p
        return out


# ---- MT19937 and the query draw ---------------------------------------------------------------------------------------------------
class Mt19937:
    def __init__(self, seed):
        s = [seed & 0xFFFFFFFF]
        for i in range(1, 624):
            s.append((1812433253 * (s[-1] ^ (s[-1] >> 30)) + i) & 0xFFFFFFFF)
        self.s, self.i = s, 624

    def next(self):
        if self.i >= 624:
            s = self.s
            for i in range(624):
                y = (s[i] & 0x80000000) | (s[(i + 1) % 624] & 0x7FFFFFFF)
                s[i] = s[(i + 397) % 624] ^ (y >> 1) ^ (0x9908B0DF if y & 1 else 0)
            self.i = 0
        y = self.s[self.i]
        self.i += 1
        y ^= y >> 11
        y ^= (y << 7) & 0x9D2C5680
        y ^= (y << 15) & 0xEFC60000
        y ^= y >> 18
        return y


def draw_queries(seed, count, final_size, n):
    """`count` queries from the inclusive range [final_size, n]"""
    mt, R, out = Mt19937(seed), n - final_size + 1, []
    for _ in range(count):
        m = mt.next() * R
        if (m & 0xFFFFFFFF) < R:
            while (m & 0xFFFFFFFF) < (2**32 - R) % R:
                m = mt.next() * R
        out.append(final_size + (m >> 32))
    return out


# ---- the transcript -----------------------------------------------------------------------------------------------------------------
class Transcript:
    def __init__(self, hasher, labels, public_state, logn):
        """labels: (domain separator, round challenge, commit phase, nonce), bytes each"""
        self.hasher = hasher
        self.ds, self.round, self.commit, self.nonce = labels
        self.entry0 = self.ds + logn.to_bytes(4, "little") + public_state

    def round_input(self, prev: bytes, root: bytes):
        return self.entry0 + prev + self.round + self.commit + root

    def pow_challenge(self, alpha: bytes):
        return self.entry0 + alpha + self.nonce

    def query_input(self, with_pow, alpha: bytes, nonce):
        return self.entry0 + self.nonce + (nonce & 0xFFFFFFFF).to_bytes(4, "little") if with_pow else self.entry0 + alpha

    def hash(self, msg):
        return bm.digest(self.hasher, msg)


def pow_candidate(hasher, challenge: bytes, nonce, padding=24):
    return int.from_bytes(bm.digest(hasher, challenge + nonce.to_bytes(8, "little") + bytes(padding))[:8], "little")


def pow_solve(hasher, challenge: bytes, bits):
    nonce = 0
    while pow_candidate(hasher, challenge, nonce) >= 1 << (64 - bits):
        nonce += 1
    return nonce


def tree_shape(F, leaves_hash, compress_hash, size):
    """the tree of a round of `size` elements: the leaves hasher (one element per leaf), then log2(size) compress layers"""
    out = bm.OUT_SIZE[compress_hash]
    return bm.TreeShape([(leaves_hash, F.bytes)] + [(compress_hash, 2 * out)] * (size.bit_length() - 1), F.bytes)


def plan(n, stopping_degree, nof_queries, folding_factor=2, compress_arity=2):
    """(logn, rounds, final_size), or None where the library answers INVALID_ARGUMENT"""
    fs = stopping_degree + 1
    if folding_factor != 2 or n == 0 or n & (n - 1) or n >= 1 << 32 or nof_queries == 0 or nof_queries > n // 2 or compress_arity != 2:
        return None
    if fs & (fs - 1) or fs >= n:
        return None
    logn = n.bit_length() - 1
    return logn, logn - (fs.bit_length() - 1), fs


def prove(field, extension, data, transcript_hasher, labels, public_state, seed, leaves_hash, compress_hash, stopping_degree, pow_bits, nof_queries):
    """data: list of element tuples; seed: an element tuple. Returns dict(final_poly, nonce, queries, slots) with
    slots[q][r] = (leaf_idx, leaf, root, path), q over the 2 * nof_queries slots."""
    F = Field(field, extension)
    logn, rounds, final_size = plan(len(data), stopping_degree, nof_queries)
    tr = Transcript(transcript_hasher, labels, public_state, logn)
    layers, shapes, raw, prev, alpha = [list(data)], [], [], F.to_bytes(seed), None
    for r in range(rounds):
        shape = tree_shape(F, leaves_hash, compress_hash, len(layers[r]))
        shapes.append(shape)
        raw.append(b"".join(F.to_bytes(e) for e in layers[r]))
        root = bm.build(shape, raw[r])[-1]
        alpha = F.from_digest(tr.hash(tr.round_input(prev, root)))
        prev = F.to_bytes(alpha)
        layers.append(F.fold(layers[r], alpha))
    nonce = pow_solve(transcript_hasher, tr.pow_challenge(prev), pow_bits) if pow_bits else 0
    seed32 = int.from_bytes(tr.hash(tr.query_input(pow_bits != 0, prev, nonce))[:4], "little")
    queries = draw_queries(seed32, nof_queries, final_size, len(data))
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


def verify(field, extension, proof, transcript_hasher, labels, public_state, seed, leaves_hash, compress_hash, stopping_degree, pow_bits, nof_queries):
    F = Field(field, extension)
    final_poly, slots = proof["final_poly"], proof["slots"]
    if len(final_poly) != stopping_degree + 1:
        return False
    rounds = len(slots[0])
    n = len(final_poly) << rounds
    if plan(n, stopping_degree, nof_queries) is None or len(slots) != 2 * nof_queries:
        return False
    logn = n.bit_length() - 1
    tr = Transcript(transcript_hasher, labels, public_state, logn)
    prev, alphas = F.to_bytes(seed), []
    for r in range(rounds):
        alphas.append(F.from_digest(tr.hash(tr.round_input(prev, slots[0][r][2]))))
        prev = F.to_bytes(alphas[-1])
    if pow_bits and pow_candidate(transcript_hasher, tr.pow_challenge(prev), proof["nonce"]) >= 1 << (64 - pow_bits):
        return False
    seed32 = int.from_bytes(tr.hash(tr.query_input(pow_bits != 0, prev, proof["nonce"]))[:4], "little")
    queries = draw_queries(seed32, nof_queries, len(final_poly), n)
    w_inv, half = pow(F.omega(logn), F.p - 2, F.p), (F.p + 1) // 2
    for j, q in enumerate(queries):
        for r in range(rounds):
            size = n >> r
            shape = tree_shape(F, leaves_hash, compress_hash, size)
            (ia, la, ra, pa), (ib, lb, rb, pb) = slots[2 * j][r], slots[2 * j + 1][r]
            if not (bm.verify(shape, la, ia, pa, ra, False) and bm.verify(shape, lb, ib, pb, rb, False)):
                return False
            if ia != q % size or ib != (q + size // 2) % size:
                return False
            a, b = F.from_bytes(la), F.from_bytes(lb)
            odd = F.scale(F.sub(a, b), half * pow(w_inv, ia << r, F.p) % F.p)
            folded = F.add(F.scale(F.add(a, b), half), F.mul(alphas[r], odd))
            want = final_poly[q % len(final_poly)] if r + 1 == rounds else F.from_bytes(slots[2 * j][r + 1][1])
            if tuple(want) != folded:
                return False
    return True


# ---- the fixtures (tests/golden/fri_vectors.json) --------------------------------------------------------------------------------------
def load_fixtures():
    import json
    import os

    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fri_vectors.json")) as f:
        return json.load(f)["cases"]


def case_elements(case, key="input"):
    w = 4 if case["extension"] else 1
    v = case[key]
    return [tuple(v[i:i + w]) for i in range(0, len(v), w)]


def case_protocol(case):
    """the arguments prove() and verify() share, after the data / the proof"""
    return (case["transcript_hash"], tuple(s.encode() for s in case["labels"]), bytes.fromhex(case["public_state"]), tuple(case["seed"]), case["leaves_hash"],
            case["compress_hash"], case["stopping_degree"], case["pow_bits"], case["nof_queries"])


def case_proof(case):
    """the fixture's proof in the model's form"""
    slots = [[(s["leaf_idx"], bytes.fromhex(s["leaf"]), bytes.fromhex(s["root"]), bytes.fromhex(s["path"])) for s in row] for row in case["slots"]]
    return {"final_poly": case_elements(case, "final_poly"), "nonce": case["nonce"], "slots": slots}
