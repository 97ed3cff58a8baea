"""Test infrastructure: a pure-Python / NumPy model of the device hashers and of the Merkle tree built from them.

Keccak-f[1600] and the sponge are written from FIPS 202 (rotation offsets from the (x, y) -> (y, 2x + 3y) walk, round constants
from the degree-8 LFSR); the SHA3 modes are checked against hashlib in tests/test_hash_cpu.py. The state is 25 NumPy uint64
vectors, one entry per message, so a whole tree layer is hashed at once.

Tree semantics (the ones include/icicle_hip.h states): the tree is the full tree over the leaves padded to its capacity; a proof's
leaf is the whole layer-0 chunk around the element, its path the groups of sibling digests layer by layer.
"""
import functools

import numpy as np

MASK = (1 << 64) - 1


def _round_constants():
    rc, r = [], 1
    for _ in range(24):
        c = 0
        for j in range(7):
            if r & 1:
                c |= 1 << ((1 << j) - 1)
            r = ((r << 1) ^ (0x71 if r & 0x80 else 0)) & 0xFF  # x^8 + x^6 + x^5 + x^4 + 1
        rc.append(c)
    return rc


def _rotation_offsets():
    rot = [0] * 25
    x, y = 1, 0
    for t in range(24):
        rot[x + 5 * y] = ((t + 1) * (t + 2) // 2) % 64
        x, y = y, (2 * x + 3 * y) % 5
    return rot


RC = _round_constants()
ROT = _rotation_offsets()


def _rol(v, n):
    if n == 0:
        return v
    return (v << np.uint64(n)) | (v >> np.uint64(64 - n))


def keccak_f(a):
    """a: list of 25 uint64 arrays (lane x + 5 y), permuted in place"""
    for rnd in range(24):
        c = [a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20] for x in range(5)]
        d = [c[(x + 4) % 5] ^ _rol(c[(x + 1) % 5], 1) for x in range(5)]
        for i in range(25):
            a[i] = a[i] ^ d[i % 5]
        b = [None] * 25
        for x in range(5):
            for y in range(5):
                b[y + 5 * ((2 * x + 3 * y) % 5)] = _rol(a[x + 5 * y], ROT[x + 5 * y])
        for y in range(5):
            for x in range(5):
                a[x + 5 * y] = b[x + 5 * y] ^ (~b[(x + 1) % 5 + 5 * y] & b[(x + 2) % 5 + 5 * y])
        a[0] = a[0] ^ np.uint64(RC[rnd])
    return a


def keccak_f_int(a):
    """the same permutation on 25 Python ints (one message: much quicker than 1-element arrays)"""
    def rol(v, n):
        return ((v << n) | (v >> (64 - n))) & MASK if n else v

    for rnd in range(24):
        c = [a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20] for x in range(5)]
        d = [c[(x + 4) % 5] ^ rol(c[(x + 1) % 5], 1) for x in range(5)]
        b = [0] * 25
        for x in range(5):
            for y in range(5):
                b[y + 5 * ((2 * x + 3 * y) % 5)] = rol(a[x + 5 * y] ^ d[x], ROT[x + 5 * y])
        for y in range(0, 25, 5):
            for x in range(5):
                a[x + y] = b[x + y] ^ (~b[(x + 1) % 5 + y] & MASK & b[(x + 2) % 5 + y])
        a[0] ^= RC[rnd]
    return a


# name -> (rate bytes, domain suffix, digest bytes)
VARIANTS = {"keccak256": (136, 0x01, 32), "keccak512": (72, 0x01, 64), "sha3_256": (136, 0x06, 32), "sha3_512": (72, 0x06, 64)}


def sponge_batch(msgs, rate, suffix, outlen):
    """msgs: uint8 array [n, length] -> digests uint8 [n, outlen] (outlen <= rate: one squeeze)"""
    msgs = np.ascontiguousarray(msgs, dtype=np.uint8)
    n, length = msgs.shape
    blocks = length // rate + 1
    padded = np.zeros((n, blocks * rate), dtype=np.uint8)
    padded[:, :length] = msgs
    padded[:, length] ^= suffix
    padded[:, blocks * rate - 1] ^= 0x80
    words = padded.view("<u8").reshape(n, blocks, rate // 8)
    a = [np.zeros(n, dtype=np.uint64) for _ in range(25)]
    for blk in range(blocks):
        for i in range(rate // 8):
            a[i] = a[i] ^ words[:, blk, i]
        keccak_f(a)
    out = np.stack(a[: outlen // 8], axis=1).astype("<u8")
    return out.view(np.uint8).reshape(n, outlen)


def digest(name, msg: bytes) -> bytes:
    rate, suffix, outlen = VARIANTS[name]
    blocks = len(msg) // rate + 1
    padded = bytearray(msg) + bytes(blocks * rate - len(msg))
    padded[len(msg)] ^= suffix
    padded[-1] ^= 0x80
    a = [0] * 25
    for blk in range(blocks):
        for i in range(rate // 8):
            a[i] ^= int.from_bytes(padded[blk * rate + 8 * i:blk * rate + 8 * i + 8], "little")
        keccak_f_int(a)
    return b"".join(v.to_bytes(8, "little") for v in a[:outlen // 8])


def hash_batch(name, data: bytes, size: int, batch: int) -> bytes:
    """`batch` messages of `size` bytes back to back -> digests back to back"""
    rate, suffix, outlen = VARIANTS[name]
    return sponge_batch(np.frombuffer(data, dtype=np.uint8, count=size * batch).reshape(batch, size), rate, suffix, outlen).tobytes()


# ---- the tree ------------------------------------------------------------------------------------------------------------------
PAD_NONE, PAD_ZERO, PAD_LAST = 0, 1, 2


class TreeShape:
    """layers: sequence of (variant name, input chunk bytes), leaf layer first"""

    def __init__(self, layers, leaf_element_size):
        self.layers = tuple(layers)
        self.es = leaf_element_size
        self.chunk = [c for _, c in self.layers]
        self.out = [VARIANTS[n][2] for n, _ in self.layers]
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

    def arity(self, i):
        return self.chunk[i] // self.out[i - 1]

    def padding(self, leaves_size, policy):
        """(full_chunks, pad_bytes, last_off) or None where the library answers INVALID_ARGUMENT"""
        if leaves_size == 0 or leaves_size > self.capacity or policy not in (PAD_NONE, PAD_ZERO, PAD_LAST):
            return None
        last_off = 0
        if leaves_size < self.capacity:
            if policy == PAD_NONE:
                return None
            if policy == PAD_LAST:
                if leaves_size % self.es or self.chunk[0] % self.es or leaves_size < self.es:
                    return None
                last_off = leaves_size - self.es
        return leaves_size // self.chunk[0], self.capacity - leaves_size, last_off

    def pad(self, leaves: bytes, policy) -> bytes:
        assert self.padding(len(leaves), policy) is not None
        missing = self.capacity - len(leaves)
        if missing == 0:
            return leaves
        if policy == PAD_ZERO:
            return leaves + bytes(missing)
        last = leaves[len(leaves) - self.es:]
        return leaves + last * (missing // self.es)

    def proof_steps(self, leaf_idx, pruned):
        """[(node, src_off, len, skip_off, dst_off)] for layers 0 .. L-2, and the path size"""
        node = leaf_idx * self.es // self.chunk[0]
        steps, dst = [], 0
        for i in range(len(self.layers) - 1):
            a, o = self.arity(i + 1), self.out[i]
            ln = self.chunk[i + 1]
            steps.append((node, node // a * a * o, ln, node % a * o, dst))
            dst += ln - o if pruned else ln
            node //= a
        return steps, dst

    def subtree(self, leaf_idx, store_min):
        store_min = min(max(store_min, 0), len(self.layers) - 1)
        cnt = self.count[0] // self.count[store_min]
        chunk0 = leaf_idx * self.es // self.chunk[0]
        return chunk0 // cnt * cnt, cnt


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
    leaf = padded[chunk0 * c0:(chunk0 + 1) * c0]
    steps, size = shape.proof_steps(leaf_idx, pruned)
    path = b""
    for i, (_, src, ln, skip, dst) in enumerate(steps):
        assert len(path) == dst
        group = layers[i][src:src + ln]
        path += group[:skip] + group[skip + shape.out[i]:] if pruned else group
    assert len(path) == size == (shape.pruned_path if pruned else shape.full_path)
    return leaf, path, layers[-1]


def verify(shape: TreeShape, leaf: bytes, leaf_idx, path: bytes, root: bytes, pruned) -> bool:
    """the reference's verify walk (include/icicle/merkle/merkle_tree.h): one hash per layer"""
    start = leaf_idx * shape.es
    in_size = len(leaf)
    out_size = shape.out[0]
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
