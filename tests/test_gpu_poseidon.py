"""GPU: Poseidon over the scalar fields of BN254, BLS12-381, BLS12-377 and Grumpkin through the C ABI -- every recorded digest of the
reference (tests/golden/poseidon_vectors.json) byte for byte, batches on both sides of a wave and of a block of a lane-per-hash
kernel against the model (tests/poseidon_model.py), and Merkle trees whose layers are Poseidon hashers: the reference's recorded
roots and paths, roots and openings against the model, batched openings, verification and what fails it."""
import functools
import json
import os

import numpy as np
import pytest

from tests import poseidon_model as pm

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TAG = 7
BATCHES = (1, 2, 63, 64, 65, 257)  # one lane, two, a wave less one, a wave, a wave and one, a block of 256 and one
PAIRS = [pytest.param(f, t, id=f"{f}-t{t}") for f, t in pm.BUILT]


@functools.lru_cache(maxsize=None)
def golden():
    with open(os.path.join(HERE, "golden", "poseidon_vectors.json")) as f:
        return json.load(f)


def ints(hexes):
    return [int(v, 16) for v in hexes]


def as_words(elements):
    return np.frombuffer(pm.to_bytes(elements), dtype=np.uint32).copy()


def test_every_recorded_digest_with_host_operands(hip):
    from icicle_amd.hash import Hasher

    for c in golden()["cases"]:
        h = Hasher.poseidon(c["field"], c["t"], domain_tag=c["tag"])
        out = np.zeros(8 * c["batch"], dtype=np.uint32)
        h.hash(as_words(ints(c["input"])), batch=c["batch"], out=out)
        assert out.tobytes() == pm.to_bytes(ints(c["digests"])), (c["field"], c["t"], c["tag"])
        h.close()


@functools.lru_cache(maxsize=None)
def edge_reference(field, t, tag):
    """max(BATCHES) messages and their digests from the model; a smaller batch is a prefix of both. Message 0 is p - 1 in every
    position, message 1 holds 0 and 1."""
    p, n, a = pm.FIELDS[field], max(BATCHES), pm.arity(t, tag)
    rng = np.random.default_rng(1000 * t + (tag or 0))
    data = [int.from_bytes(rng.bytes(40), "little") % p for _ in range(n * a)]
    data[:a] = [p - 1] * a
    data[a:a + 2] = [0, 1]
    return as_words(data), pm.to_bytes(pm.hash_batch(field, t, data, tag))


@pytest.mark.parametrize("tag", [None, TAG], ids=["untagged", "tagged"])
@pytest.mark.parametrize("field,t", PAIRS)
def test_batches_on_both_sides_of_a_wave_and_a_block(hip, field, t, tag):
    from icicle_amd.hash import Hasher
    from icicle_amd.runtime import DeviceVec

    data, want = edge_reference(field, t, tag)
    a = pm.arity(t, tag)
    h = Hasher.poseidon(field, t, domain_tag=tag)
    d_in = DeviceVec.from_host(data)
    for batch in BATCHES:
        for src in (data[:8 * a * batch], d_in):  # host operands, device operands
            d_out = DeviceVec.from_host(np.full(8 * (batch + 1), 0xDEADBEEF, dtype=np.uint32))
            h.hash(src, size=32 * a, batch=batch, out=d_out)
            out = d_out.to_host(np.uint32)
            assert out[:8 * batch].tobytes() == want[:32 * batch], (batch, src is d_in)
            assert (out[8 * batch:] == 0xDEADBEEF).all(), batch  # the element behind the last digest stays
    h.close()


def test_one_async_call_on_a_created_stream(hip):
    import icicle_amd
    from icicle_amd.hash import Hasher
    from icicle_amd.runtime import DeviceVec, Stream

    field, t, batch = "bls12_381", 5, 65
    data, want = edge_reference(field, t, TAG)
    h = Hasher.poseidon(field, t, domain_tag=TAG)
    d_in, d_out = DeviceVec.from_host(data), DeviceVec(32 * batch)
    st = Stream()
    cfg = icicle_amd.HashConfig.default()
    cfg.stream, cfg.is_async = st.handle, True
    h.hash(d_in, size=32 * (t - 1), batch=batch, out=d_out, cfg=cfg)
    st.synchronize()
    assert d_out.to_host(np.uint32).tobytes() == want[:32 * batch]
    st.destroy()
    h.close()


# ---- Merkle trees ----------------------------------------------------------------------------------------------------------------------
def make_tree(specs):
    from icicle_amd.hash import Hasher
    from icicle_amd.merkle import MerkleTree

    hashers = [Hasher.poseidon(f, t, domain_tag=tag) for f, t, tag in specs]
    tree = MerkleTree(hashers, 32)
    for h in hashers:
        h.close()  # the tree keeps the tables alive
    return tree


def config(policy):
    import icicle_amd

    cfg = icicle_amd.MerkleTreeConfig.default()
    cfg.padding_policy = policy
    return cfg


def test_recorded_trees_reproduce_the_references_roots_and_paths(hip):
    for t in golden()["trees"]:
        leaves = np.frombuffer(pm.to_bytes(ints(t["leaves"])), dtype=np.uint8).copy()
        tree = make_tree([(t["field"], t["t"], t["tag"])] * t["layers"]).build(leaves, cfg=config(t["policy"]))
        key = (t["field"], t["t"], t["tag"], len(t["leaves"]))
        assert tree.root() == pm.to_bytes([int(t["root"], 16)]), key
        pr = tree.proof(leaves, t["leaf_idx"], cfg=config(t["policy"]))
        assert pr.path == pm.to_bytes(ints(t["path"])) and tree.verify(pr), key
        tree.close()


# arity 2 over 1, 2, 5, 64 and 65 leaves, arity 4 over 16 and 17: (t, layers, leaves given)
SHAPES = [(3, 1, 1), (3, 1, 2), (3, 3, 5), (3, 6, 64), (3, 7, 65), (5, 2, 16), (5, 3, 17)]


@pytest.mark.parametrize("t,layers,given", SHAPES, ids=[f"arity{t - 1}-{n}leaves" for t, _, n in SHAPES])
def test_tree_roots_openings_and_verification_against_the_model(hip, t, layers, given):
    from icicle_amd.merkle import MerkleProof

    field = "bls12_377" if t == 3 else "bn254"
    p = pm.FIELDS[field]
    shape = pm.TreeShape([(field, t, TAG)] * layers)
    capacity = shape.capacity // 32
    policy = pm.PAD_NONE if given == capacity else pm.PAD_ZERO
    if given == 1:  # one leaf under one arity-2 hash: half a chunk, zero-padded
        assert capacity == 2 and policy == pm.PAD_ZERO
    rng = np.random.default_rng(given)
    elems = [int.from_bytes(rng.bytes(40), "little") % p for _ in range(given)]
    elems[-1] = p - 1
    raw = pm.to_bytes(elems)
    leaves = np.frombuffer(raw, dtype=np.uint8).copy()
    tree = make_tree(shape.specs).build(leaves, cfg=config(policy))
    want_root = pm.build(shape, raw, policy)[-1]
    assert tree.root() == want_root
    indices = sorted({0, given // 2, given - 1})
    batch = tree.proofs(leaves, indices, cfg=config(policy))
    for idx, many in zip(indices, batch):
        leaf, path, root = pm.proof(shape, raw, idx, False, policy)
        single = tree.proof(leaves, idx, cfg=config(policy))
        assert (single.leaf, single.path, single.root) == (leaf, path, root), idx
        assert (many.leaf, many.path, many.root, many.leaf_idx) == (leaf, path, root, idx)
        assert tree.verify(single) and pm.verify(shape, leaf, idx, path, root, False)
        pruned = tree.proof(leaves, idx, pruned=True, cfg=config(policy))
        assert pruned.path == pm.proof(shape, raw, idx, True, policy)[1] and tree.verify(pruned)
        # one flipped word in the leaf, in a path node and in the root
        for part in ("leaf", "path", "root"):
            if part == "path" and not path:
                continue
            parts = {"leaf": bytearray(leaf), "path": bytearray(path), "root": bytearray(root)}
            parts[part][len(parts[part]) - 4] ^= 1
            forged = MerkleProof.with_data(False, idx, bytes(parts["leaf"]), bytes(parts["root"]), bytes(parts["path"]))
            assert not tree.verify(forged), (idx, part)
    assert tree.verify_batch(batch) == [True] * len(indices)
    if layers > 1:
        bad = bytearray(batch[-1].path)
        bad[0] ^= 0x40
        forged = MerkleProof.with_data(False, indices[-1], batch[-1].leaf, batch[-1].root, bytes(bad))
        assert tree.verify_batch([batch[0], forged]) == [True, False]
        assert tree.verify_batch(tree.proofs(leaves, indices, pruned=True, cfg=config(policy))) == [True] * len(indices)
    tree.close()
