"""Test infrastructure: pure-Python / NumPy models of Blake2s-256 (RFC 7693) and Blake3 (the BLAKE3 specification, default hash
mode, 32-byte output), and a Merkle tree model over all six device hashers (tests/merkle_model.py holds the Keccak ones).

The state is 16 NumPy uint32 vectors, one entry per message, so a whole tree layer is hashed at once. The constants are derived
where they can be: the IV from integer square roots, the Blake3 message schedule from its one permutation. Blake2s is checked
against hashlib, Blake3 against digests recorded from a portable C implementation (tests/golden/blake3_vectors.json).

Blake3's tree is built here the way the specification states it -- recursively, the left subtree the largest power of two of chunks
below the total -- and not the way the device builds it (adjacent pairs level by level), so the two check each other.
"""
import functools
import math

import numpy as np

from tests import merkle_model as mm

IV = [math.isqrt(p << 64) & 0xFFFFFFFF for p in (2, 3, 5, 7, 11, 13, 17, 19)]  # frac(sqrt(p)) * 2^32

# RFC 7693 section 2.7
SIGMA = [
    [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15],
    [14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3],
    [11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4],
    [7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8],
    [9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13],
    [2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9],
    [12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11],
    [13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10],
    [6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5],
    [10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0],
]
# BLAKE3 table 2
PERM = [2, 6, 3, 10, 7, 0, 4, 13, 1, 11, 12, 5, 9, 14, 15, 8]
CHUNK_START, CHUNK_END, PARENT, ROOT = 1, 2, 4, 8
CHUNK = 1024


def _schedules():
    rows = [list(range(16))]
    for _ in range(6):
        rows.append([rows[-1][PERM[i]] for i in range(16)])
    return rows


SCHED3 = _schedules()
assert sorted(PERM) == list(range(16)) and all(sorted(r) == list(range(16)) for r in SIGMA)


def _rotr(x, n):
    return (x >> np.uint32(n)) | (x << np.uint32(32 - n))


def _g(v, a, b, c, d, x, y):
    v[a] = v[a] + v[b] + x
    v[d] = _rotr(v[d] ^ v[a], 16)
    v[c] = v[c] + v[d]
    v[b] = _rotr(v[b] ^ v[c], 12)
    v[a] = v[a] + v[b] + y
    v[d] = _rotr(v[d] ^ v[a], 8)
    v[c] = v[c] + v[d]
    v[b] = _rotr(v[b] ^ v[c], 7)


def _round(v, m, s):
    _g(v, 0, 4, 8, 12, m[s[0]], m[s[1]])
    _g(v, 1, 5, 9, 13, m[s[2]], m[s[3]])
    _g(v, 2, 6, 10, 14, m[s[4]], m[s[5]])
    _g(v, 3, 7, 11, 15, m[s[6]], m[s[7]])
    _g(v, 0, 5, 10, 15, m[s[8]], m[s[9]])
    _g(v, 1, 6, 11, 12, m[s[10]], m[s[11]])
    _g(v, 2, 7, 8, 13, m[s[12]], m[s[13]])
    _g(v, 3, 4, 9, 14, m[s[14]], m[s[15]])


def _const(n, value):
    return np.full(n, value, dtype=np.uint32)


def _blocks(msgs):
    """uint8 [n, length] -> (uint32 [n, blocks, 16] zero-filled, blocks); an empty message still has one block"""
    n, length = msgs.shape
    blocks = max(1, -(-length // 64))
    padded = np.zeros((n, blocks * 64), dtype=np.uint8)
    padded[:, :length] = msgs
    return padded.view("<u4").reshape(n, blocks, 16), blocks


def _digest_bytes(h, n):
    return np.stack(h[:8], axis=1).astype("<u4").view(np.uint8).reshape(n, 32)


# ---- Blake2s ---------------------------------------------------------------------------------------------------------------------
def blake2s_batch(msgs):
    """msgs: uint8 array [n, length] -> digests uint8 [n, 32]; no key, parameter word 0x01010020"""
    msgs = np.ascontiguousarray(msgs, dtype=np.uint8)
    n, length = msgs.shape
    words, blocks = _blocks(msgs)
    h = [_const(n, IV[i]) for i in range(8)]
    h[0] = h[0] ^ np.uint32(0x01010020)
    with np.errstate(over="ignore"):
        for blk in range(blocks):
            last = blk == blocks - 1
            t = length if last else 64 * (blk + 1)
            m = [words[:, blk, i] for i in range(16)]
            v = h[:] + [_const(n, IV[i]) for i in range(8)]
            v[12] = v[12] ^ np.uint32(t & 0xFFFFFFFF)
            v[13] = v[13] ^ np.uint32(t >> 32)
            if last:
                v[14] = ~v[14]
            for r in range(10):
                _round(v, m, SIGMA[r])
            h = [h[i] ^ v[i] ^ v[i + 8] for i in range(8)]
    return _digest_bytes(h, n)


# ---- Blake3 ----------------------------------------------------------------------------------------------------------------------
def _compress3(cv, m, counter, block_len, flags):
    n = len(cv[0])
    v = cv[:] + [_const(n, IV[i]) for i in range(4)] + [_const(n, counter & 0xFFFFFFFF), _const(n, counter >> 32), _const(n, block_len), _const(n, flags)]
    with np.errstate(over="ignore"):
        for r in range(7):
            _round(v, m, SCHED3[r])
    return [v[i] ^ v[i + 8] for i in range(8)]


def _chunk_cv(msgs, counter, root):
    """chaining value of one chunk (<= 1024 bytes) of every message; root: the message is this one chunk"""
    n, length = msgs.shape
    words, blocks = _blocks(msgs)
    cv = [_const(n, IV[i]) for i in range(8)]
    for blk in range(blocks):
        last = blk == blocks - 1
        flags = (CHUNK_START if blk == 0 else 0) | ((CHUNK_END | (ROOT if root else 0)) if last else 0)
        cv = _compress3(cv, [words[:, blk, i] for i in range(16)], counter, length - 64 * blk if last else 64, flags)
    return cv


def _subtree_cv(msgs, first_chunk, chunks, root):
    """chaining value of the subtree over chunks [first_chunk, first_chunk + chunks) of every message"""
    if chunks == 1:
        return _chunk_cv(msgs[:, first_chunk * CHUNK:(first_chunk + 1) * CHUNK], first_chunk, root)
    left = 1 << ((chunks - 1).bit_length() - 1)  # the largest power of two below `chunks`
    lcv = _subtree_cv(msgs, first_chunk, left, False)
    rcv = _subtree_cv(msgs, first_chunk + left, chunks - left, False)
    n = msgs.shape[0]
    return _compress3([_const(n, IV[i]) for i in range(8)], lcv + rcv, 0, 64, PARENT | (ROOT if root else 0))


def blake3_batch(msgs):
    """msgs: uint8 array [n, length] -> digests uint8 [n, 32]"""
    msgs = np.ascontiguousarray(msgs, dtype=np.uint8)
    n, length = msgs.shape
    return _digest_bytes(_subtree_cv(msgs, 0, max(1, -(-length // CHUNK)), True), n)


# ---- all six hashers ---------------------------------------------------------------------------------------------------------------
BLAKE = {"blake2s": blake2s_batch, "blake3": blake3_batch}
OUT_SIZE = {**{name: v[2] for name, v in mm.VARIANTS.items()}, "blake2s": 32, "blake3": 32}


def hash_batch(name, data: bytes, size: int, batch: int) -> bytes:
    """`batch` messages of `size` bytes back to back -> digests back to back"""
    if name not in BLAKE:
        return mm.hash_batch(name, data, size, batch)
    return BLAKE[name](np.frombuffer(data, dtype=np.uint8, count=size * batch).reshape(batch, size)).tobytes()


def digest(name, msg: bytes) -> bytes:
    if name not in BLAKE:
        return mm.digest(name, msg)
    return hash_batch(name, msg, len(msg), 1)


# ---- the tree ----------------------------------------------------------------------------------------------------------------------
PAD_NONE, PAD_ZERO, PAD_LAST = mm.PAD_NONE, mm.PAD_ZERO, mm.PAD_LAST


class TreeShape(mm.TreeShape):
    """mm.TreeShape with the digest sizes of all six hashers (the base class reads them from its own Keccak table)"""

    def __init__(self, layers, leaf_element_size):
        self.layers = tuple(layers)
        self.es = leaf_element_size
        self.chunk = [c for _, c in self.layers]
        self.out = [OUT_SIZE[n] for n, _ in self.layers]
        L = len(self.layers)
        self.count = [0] * L
        n = 1
        for i in range(L - 1, -1, -1):
            self.count[i] = n
            if i > 0:
                if self.chunk[i] % self.out[i - 1]:
                    raise ValueError("not a tree")
                n *= self.chunk[i] // self.out[i - 1]
        self.capacity = self.count[0] * self.chunk[0]
        self.full_path = sum(self.chunk[1:])
        self.pruned_path = sum(self.chunk[i] - self.out[i - 1] for i in range(1, L))


@functools.lru_cache(maxsize=64)
def _build_cached(layers, es, padded: bytes):
    shape = TreeShape(layers, es)
    out, data = [], padded
    for i, (name, c) in enumerate(shape.layers):
        data = hash_batch(name, data, c, shape.count[i])
        out.append(data)
    return tuple(out)


def build(shape: TreeShape, leaves: bytes, policy=PAD_NONE):
    """digests of every layer (a tuple of bytes, the root last) over the padded leaves"""
    return _build_cached(shape.layers, shape.es, shape.pad(bytes(leaves), policy))


def proof(shape: TreeShape, leaves: bytes, leaf_idx, pruned, policy=PAD_NONE):
    """(leaf chunk, path, root)"""
    padded = shape.pad(bytes(leaves), policy)
    layers = build(shape, leaves, policy)
    c0 = shape.chunk[0]
    chunk0 = leaf_idx * shape.es // c0
    steps, size = shape.proof_steps(leaf_idx, pruned)
    path = b""
    for i, (_, src, ln, skip, dst) in enumerate(steps):
        assert len(path) == dst
        group = layers[i][src:src + ln]
        path += group[:skip] + group[skip + shape.out[i]:] if pruned else group
    assert len(path) == size == (shape.pruned_path if pruned else shape.full_path)
    return padded[chunk0 * c0:(chunk0 + 1) * c0], path, layers[-1]


def verify(shape: TreeShape, leaf: bytes, leaf_idx, path: bytes, root: bytes, pruned) -> bool:
    """the reference's verify walk (include/icicle/merkle/merkle_tree.h): one hash per layer"""
    start, in_size, out_size = leaf_idx * shape.es, len(leaf), shape.out[0]
    h = digest(shape.layers[0][0], leaf)
    pos = 0
    for i in range(1, len(shape.layers)):
        start = start // in_size * out_size
        in_size, out_size = shape.chunk[i], shape.out[i]
        off = start % in_size
        if pruned:
            sib = path[pos:pos + in_size - len(h)]
            pos += in_size - len(h)
            inp = sib[:off] + h + sib[off:]
        else:
            inp = path[pos:pos + in_size]
            pos += in_size
            if inp[off:off + len(h)] != h:
                return False
        h = digest(shape.layers[i][0], inp)
    return h == root
