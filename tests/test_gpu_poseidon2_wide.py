"""GPU: Poseidon2 over the scalar fields of BN254, BLS12-381, BLS12-377 and Grumpkin and over stark252 through the C ABI -- every
recorded digest of the reference (tests/golden/poseidon2_vectors_wide.json) byte for byte, batches at the block edges of a
lane-per-hash kernel against the model (tests/poseidon2_model_wide.py), and Merkle trees whose layers are these hashers: every
layer, the root, openings, batched openings and verification."""
import functools
import json
import os

import numpy as np
import pytest

from tests import poseidon2_model_wide as pw

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIELDS = tuple(pw.FIELDS)
TAG = 7
BATCHES = (1, 255, 256, 257)  # one lane, a block less one, a block, a block and one


@functools.lru_cache(maxsize=None)
def vectors():
    with open(os.path.join(HERE, "golden", "poseidon2_vectors_wide.json")) as f:
        return json.load(f)["cases"]


def elements(values):
    """canonical residues as the uint32 words the hashers read"""
    return np.frombuffer(pw.to_bytes(values), dtype=np.uint32).copy()


def test_every_recorded_digest_with_host_operands(hip):
    from icicle_amd.hash import Hasher

    hashers = {}
    for c in vectors():
        key = (c["field"], c["t"], c["tag"])
        if key not in hashers:
            hashers[key] = Hasher.poseidon2(c["field"], c["t"], domain_tag=c["tag"])
        out = np.zeros(8 * c["batch"], dtype=np.uint32)
        hashers[key].hash(elements([int(v, 16) for v in c["input"]]), size=32 * c["size"], batch=c["batch"], out=out)
        assert out.tobytes() == pw.to_bytes([int(v, 16) for v in c["digests"]]), key + (c["size"], c["batch"])
    assert len(hashers) == 5 * 4 * 2
    for h in hashers.values():
        h.close()


@functools.lru_cache(maxsize=None)
def edge_reference(field, t, size):
    """max(BATCHES) messages of `size` elements and their digests from the model; a smaller batch is a prefix of both"""
    p, n = pw.FIELDS[field], max(BATCHES)
    rng = np.random.default_rng(100 * t + size)
    data = [int.from_bytes(rng.bytes(40), "little") % p for _ in range(n * size)]
    data[:3] = (p - 1, 0, 1)
    return elements(data), pw.to_bytes(pw.hash_batch(field, t, data, size))


@pytest.mark.parametrize("t,size", [(3, 3), (3, 7), (8, 8), (8, 17)], ids=["t3-exact", "t3-sponge", "t8-exact", "t8-sponge"])
@pytest.mark.parametrize("field", FIELDS)
def test_batches_at_block_edges_with_device_operands_on_a_created_stream(hip, field, t, size):
    import icicle_amd
    from icicle_amd.hash import Hasher
    from icicle_amd.runtime import DeviceVec, Stream

    data, want = edge_reference(field, t, size)
    h = Hasher.poseidon2(field, t)
    d_in = DeviceVec.from_host(data)
    st = Stream()
    for batch in BATCHES:
        guard = np.full(8 * (batch + 1), 0xDEADBEEF, dtype=np.uint32)  # the element behind the last digest stays
        d_out = DeviceVec.from_host(guard)
        cfg = icicle_amd.HashConfig.default()
        cfg.stream, cfg.is_async = st.handle, True
        h.hash(d_in, size=32 * size, batch=batch, out=d_out, cfg=cfg)
        st.synchronize()
        got = d_out.to_host(np.uint32)
        assert got[:8 * batch].tobytes() == want[:32 * batch] and (got[8 * batch:] == 0xDEADBEEF).all(), batch
    st.destroy()
    h.close()


# ---- Merkle trees ----------------------------------------------------------------------------------------------------------------------
# 70 leaf elements under a leaf layer of width 4 that takes 4 elements per chunk: chunk 17 holds two elements and two of padding,
# chunks 18 .. 31 only padding; above it two-to-one nodes -- width 2, or width 3 beside a domain tag
GIVEN, LEAF_ELEMS, CHUNKS = 70, 4, 32
NODES = {"t2": (2, None), "t3-tagged": (3, TAG)}


def config():
    import icicle_amd
    from icicle_amd.merkle import PaddingPolicy

    cfg = icicle_amd.MerkleTreeConfig.default()
    cfg.padding_policy = PaddingPolicy.ZERO_PADDING
    return cfg


def make_tree(field, node_t, node_tag):
    from icicle_amd.hash import Hasher
    from icicle_amd.merkle import MerkleTree

    hashers = [Hasher.poseidon2(field, 4, input_size=LEAF_ELEMS)] + [Hasher.poseidon2(field, node_t, domain_tag=node_tag) for _ in range(5)]
    tree = MerkleTree(hashers, 32)
    for h in hashers:
        h.close()  # the tree keeps the constants alive
    return tree


@functools.lru_cache(maxsize=None)
def tree_reference(field, nodes):
    """the leaves and every digest layer from the model, over the leaves padded with zeros to the tree's capacity"""
    p, (node_t, node_tag) = pw.FIELDS[field], NODES[nodes]
    rng = np.random.default_rng(len(field) + node_t)
    leaves = [int.from_bytes(rng.bytes(40), "little") % p for _ in range(GIVEN)]
    leaves[0], leaves[-1] = 1, p - 1
    layers = pw.merkle_layers(field, leaves + [0] * (CHUNKS * LEAF_ELEMS - GIVEN), [(4, LEAF_ELEMS, None)] + [(node_t, 2, node_tag)] * 5)
    return elements(leaves), layers


def expected_path(layers, chunk):
    """full path: per layer below the root the whole group of siblings, on-path digest included"""
    out = []
    for layer in layers[:-1]:
        g = chunk // 2 * 2
        out += layer[g:g + 2]
        chunk //= 2
    return pw.to_bytes(out)


@pytest.mark.parametrize("nodes", list(NODES))
@pytest.mark.parametrize("field", FIELDS)
def test_tree_layers_root_openings_and_verification(hip, field, nodes):
    from icicle_amd.merkle import MerkleProof

    leaves, layers = tree_reference(field, nodes)
    assert [len(l) for l in layers] == [32, 16, 8, 4, 2, 1]
    root = pw.to_bytes(layers[-1])
    tree = make_tree(field, *NODES[nodes]).build(leaves, cfg=config())
    assert tree.root() == root
    # every layer: the openings of all 32 chunks between them hold every digest below the root
    raw = leaves.tobytes() + bytes(32 * (CHUNKS * LEAF_ELEMS - GIVEN))
    for chunk, pr in enumerate(tree.proofs(leaves, [LEAF_ELEMS * c for c in range(CHUNKS)], cfg=config())):
        assert pr.path == expected_path(layers, chunk) and pr.root == root, chunk
        assert pr.leaf == raw[32 * LEAF_ELEMS * chunk:32 * LEAF_ELEMS * (chunk + 1)], chunk
    # the first element, the last one given (chunk 17, which reaches into the padding) and one of the padding
    indices = [0, GIVEN - 1, 101]
    batch = tree.proofs(leaves, indices, cfg=config())
    for idx, many in zip(indices, batch):
        single = tree.proof(leaves, idx, cfg=config())
        assert single.path == expected_path(layers, idx // LEAF_ELEMS) and single.root == root, idx
        assert (many.leaf, many.root, many.path, many.leaf_idx) == (single.leaf, single.root, single.path, idx)
        assert tree.verify(single)
        for at in (0, len(single.path) - 4):  # one flipped word, in the lowest and in the highest group of the path
            bad = bytearray(single.path)
            bad[at] ^= 1
            assert not tree.verify(MerkleProof.with_data(False, idx, single.leaf, single.root, bytes(bad))), (idx, at)
        bad_leaf = bytearray(single.leaf)
        bad_leaf[36] ^= 0x10
        assert not tree.verify(MerkleProof.with_data(False, idx, bytes(bad_leaf), single.root, single.path))
    assert tree.verify_batch(batch) == [True] * 3
    bad = bytearray(batch[1].path)
    bad[40] ^= 0x40
    forged = MerkleProof.with_data(False, indices[1], batch[1].leaf, batch[1].root, bytes(bad))
    assert tree.verify_batch([batch[0], forged, batch[2]]) == [True, False, True]
    tree.close()
