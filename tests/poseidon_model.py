"""Test infrastructure: Poseidon over the 256-bit scalar fields in Python integers, in its textbook form -- every round adds its
constants, applies the S-box x^5 (to all elements in a full round, to element 0 in a partial round) and multiplies by the MDS
matrix. Written from the paper (eprint 2019/458) and not from the library's optimized schedule (icicle_amd/csrc/poseidon_params.h),
so that the two check each other; tests/golden/poseidon_vectors.json holds digests of the reference, which prove both.

  rounds      R_F = 8 (4 + 4), R_P = 56, 56, 57, 57 for t = 3, 5, 9, 12
  matrix      M[i][j] = 1 / (i + j + t); the state is a row vector: new[j] = sum_i s[i] M[i][j]
  constants   Grain LFSR seeded with field 1 (2 bits) | sbox 1 (4) | n (12) | t (12) | R_F (10) | R_P (10) | thirty 1s; 160 bits
              discarded; of every pair of bits the second is kept when the first is 1; n bits MSB first, rejected when >= p;
              n is the bit length of p, except 255 for Grumpkin (GRAIN_BITS)
  hash        state [tag, x_0 .. x_(t-2)] or [x_0 .. x_(t-1)], one permutation, digest state[1]

Elements travel as 32 little-endian bytes. Trees follow the rules tests/merkle_model.py states: the full tree over the leaves padded
to its capacity; a proof's leaf is the whole layer-0 chunk around the element, its path the groups of sibling digests layer by layer.
"""
import functools

from tests import merkle_model as mm

FIELDS = {
    "bn254": 21888242871839275222246405745257275088548364400416034343698204186575808495617,
    "bls12_381": 52435875175126190479447740508185965837690552500527637822603658699938581184513,
    "bls12_377": 8444461749428370424248824938781546531375899335154063827935233455917409239041,
    "grumpkin": 21888242871839275222246405745257275088696311157297823662689037894645226208583,
}
WIDTHS = (3, 5, 9, 12)
R_F = 8
R_P = {3: 56, 5: 56, 9: 57, 12: 57}
# the reference's table for BLS12-381 at t = 3 does not match its own round numbers: nothing defined to compute
BUILT = [(f, t) for f in FIELDS for t in WIDTHS if (f, t) != ("bls12_381", 3)]
ES = 32  # bytes of an element
# the field size the Grain LFSR is seeded with and draws, where it is not the bit length of p: the reference's constants for
# Grumpkin's scalar field (254 bits) were generated with 255 -- found by comparing digests, and the recorded digests pin it
GRAIN_BITS = {"grumpkin": 255}


def grain_constants(p, t, r_f, r_p, n=None):
    """t (r_f + r_p) constants of n bits (the bit length of p unless given), round by round"""
    n = n or p.bit_length()
    bits = []
    for value, width in ((1, 2), (1, 4), (n, 12), (t, 12), (r_f, 10), (r_p, 10), ((1 << 30) - 1, 30)):
        bits += [value >> (width - 1 - i) & 1 for i in range(width)]
    assert len(bits) == 80

    def step():
        b = bits[62] ^ bits[51] ^ bits[38] ^ bits[23] ^ bits[13] ^ bits[0]
        bits.pop(0)
        bits.append(b)
        return b

    for _ in range(160):
        step()

    def bit():
        while True:
            first, second = step(), step()
            if first:
                return second

    out = []
    while len(out) < t * (r_f + r_p):
        v = 0
        for _ in range(n):
            v = v << 1 | bit()
        if v < p:
            out.append(v)
    return out


def mds_matrix(p, t):
    return [[pow(i + j + t, -1, p) for j in range(t)] for i in range(t)]


@functools.lru_cache(maxsize=None)
def params(field, t):
    """(p, constants, matrix)"""
    p = FIELDS[field]
    return p, grain_constants(p, t, R_F, R_P[t], GRAIN_BITS.get(field)), mds_matrix(p, t)


def permute(field, t, state):
    p, rc, m = params(field, t)
    s = list(state)
    assert len(s) == t
    for r in range(R_F + R_P[t]):
        s = [(x + c) % p for x, c in zip(s, rc[r * t:(r + 1) * t])]
        if r < R_F // 2 or r >= R_F // 2 + R_P[t]:
            s = [pow(x, 5, p) for x in s]
        else:
            s[0] = pow(s[0], 5, p)
        s = [sum(s[i] * m[i][j] for i in range(t)) % p for j in range(t)]
    return s


def arity(t, tag):
    return t if tag is None else t - 1


def hash_one(field, t, msg, tag=None):
    msg = [v % FIELDS[field] for v in msg]
    assert len(msg) == arity(t, tag)
    return permute(field, t, ([tag] if tag is not None else []) + msg)[1]


def hash_batch(field, t, elements, tag=None):
    """back-to-back messages of the arity -> list of digests"""
    a = arity(t, tag)
    assert len(elements) % a == 0
    return [hash_one(field, t, elements[i:i + a], tag) for i in range(0, len(elements), a)]


def to_bytes(elements) -> bytes:
    return b"".join(int(v).to_bytes(ES, "little") for v in elements)


def from_bytes(data: bytes):
    assert len(data) % ES == 0
    return [int.from_bytes(data[i:i + ES], "little") for i in range(0, len(data), ES)]


# ---- the tree ----------------------------------------------------------------------------------------------------------------------
PAD_NONE, PAD_ZERO, PAD_LAST = mm.PAD_NONE, mm.PAD_ZERO, mm.PAD_LAST


class TreeShape(mm.TreeShape):
    """mm.TreeShape over Poseidon layers: `layers` is a sequence of (field, t, tag), leaf layer first; leaf elements of 32 bytes"""

    def __init__(self, layers):
        self.specs = tuple(layers)
        self.layers = tuple((spec, ES * arity(spec[1], spec[2])) for spec in self.specs)
        self.es = ES
        self.chunk = [c for _, c in self.layers]
        self.out = [ES] * len(self.layers)
        L = len(self.layers)
        self.count = [0] * L
        n = 1
        for i in range(L - 1, -1, -1):
            self.count[i] = n
            if i > 0:
                n *= self.chunk[i] // ES
        self.capacity = self.count[0] * self.chunk[0]
        self.full_path = sum(self.chunk[1:])
        self.pruned_path = sum(self.chunk[i] - ES for i in range(1, L))


def digest(spec, msg: bytes) -> bytes:
    field, t, tag = spec
    return to_bytes([hash_one(field, t, from_bytes(msg), tag)])


@functools.lru_cache(maxsize=64)
def _build_cached(specs, padded: bytes):
    out, data = [], padded
    for field, t, tag in specs:
        data = to_bytes(hash_batch(field, t, from_bytes(data), tag))
        out.append(data)
    return tuple(out)


def build(shape: TreeShape, leaves: bytes, policy=PAD_NONE):
    """digests of every layer (a tuple of bytes, the root last) over the padded leaves"""
    return _build_cached(shape.specs, shape.pad(bytes(leaves), policy))


def proof(shape: TreeShape, leaves: bytes, leaf_idx, pruned, policy=PAD_NONE):
    """(leaf chunk, path, root)"""
    padded = shape.pad(bytes(leaves), policy)
    layers = build(shape, leaves, policy)
    c0 = shape.chunk[0]
    chunk0 = leaf_idx * ES // c0
    steps, size = shape.proof_steps(leaf_idx, pruned)
    path = b""
    for i, (_, src, ln, skip, dst) in enumerate(steps):
        assert len(path) == dst
        group = layers[i][src:src + ln]
        path += group[:skip] + group[skip + ES:] if pruned else group
    assert len(path) == size
    return padded[chunk0 * c0:(chunk0 + 1) * c0], path, layers[-1]


def verify(shape: TreeShape, leaf: bytes, leaf_idx, path: bytes, root: bytes, pruned) -> bool:
    """the reference's verify walk (include/icicle/merkle/merkle_tree.h): one hash per layer"""
    start, in_size = leaf_idx * ES, len(leaf)
    h = digest(shape.specs[0], leaf)
    pos = 0
    for i in range(1, len(shape.specs)):
        start = start // in_size * ES
        in_size = shape.chunk[i]
        off = start % in_size
        if pruned:
            sib = path[pos:pos + in_size - ES]
            pos += in_size - ES
            inp = sib[:off] + h + sib[off:]
        else:
            inp = path[pos:pos + in_size]
            pos += in_size
            if inp[off:off + ES] != h:
                return False
        h = digest(shape.specs[i], inp)
    return h == root
