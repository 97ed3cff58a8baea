"""GPU: Poseidon2 over BabyBear and KoalaBear through the C ABI -- every recorded digest of the reference
(tests/golden/poseidon2_vectors.json) byte for byte, batches at the wave and block edges of a lane-per-hash kernel against the model
(tests/poseidon2_model.py), and Merkle trees whose layers are Poseidon2 hashers: root, openings, batched openings, verification."""
import functools
import json
import os

import numpy as np
import pytest

from tests import poseidon2_model as pm

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIELDS = tuple(pm.FIELDS)
T = 16
BATCHES = (1, 63, 64, 65, 257)  # one lane, a wave less one, a wave, a wave and one, a block of 256 and one


@functools.lru_cache(maxsize=None)
def vectors():
    with open(os.path.join(HERE, "golden", "poseidon2_vectors.json")) as f:
        return json.load(f)["cases"]


def words(hexes):
    return np.array([int(v, 16) for v in hexes], dtype=np.uint32)


def make(c):
    from icicle_amd.hash import Hasher

    return Hasher.poseidon2(c["field"], c["t"], domain_tag=c["tag"])


def test_every_recorded_digest_with_host_operands(hip):
    hashers = {}
    for c in vectors():
        key = (c["field"], c["t"], c["tag"])
        if key not in hashers:
            hashers[key] = make(c)
        out = np.zeros(c["batch"], dtype=np.uint32)
        hashers[key].hash(words(c["input"]), size=4 * c["size"], batch=c["batch"], out=out)
        assert out.tobytes() == words(c["digests"]).tobytes(), key + (c["size"], c["batch"])
    assert len(hashers) == 2 * 8 * 2
    for h in hashers.values():
        h.close()


@pytest.mark.parametrize("field", FIELDS)
def test_device_operands_on_a_created_stream(hip, field):
    import icicle_amd
    from icicle_amd.runtime import DeviceVec, Stream

    c = next(c for c in vectors() if c["field"] == field and c["t"] == T and c["batch"] == 3)
    h = make(c)
    d_in, d_out = DeviceVec.from_host(words(c["input"])), DeviceVec(4 * c["batch"])
    st = Stream()
    cfg = icicle_amd.HashConfig.default()
    cfg.stream, cfg.is_async = st.handle, True
    h.hash(d_in, size=4 * c["size"], batch=c["batch"], out=d_out, cfg=cfg)
    st.synchronize()
    assert d_out.to_host(np.uint32).tobytes() == words(c["digests"]).tobytes()
    st.destroy()
    h.close()


@functools.lru_cache(maxsize=None)
def edge_reference(field, size):
    """max(BATCHES) messages of `size` elements and their digests from the model; a smaller batch is a prefix of both"""
    p, n = pm.FIELDS[field], max(BATCHES)
    data = np.random.default_rng(size).integers(0, p, size=n * size, dtype=np.uint64).astype(np.uint32)
    data[:3] = (p - 1, 0, 1)
    return data, np.array(pm.hash_batch(field, T, [int(v) for v in data], size), dtype=np.uint32)


@pytest.mark.parametrize("size", [T, 2 * T - 1], ids=["exact", "sponge"])
@pytest.mark.parametrize("field", FIELDS)
def test_batches_at_wave_and_block_edges(hip, field, size):
    from icicle_amd.hash import Hasher

    data, want = edge_reference(field, size)
    h = Hasher.poseidon2(field, T)
    for batch in BATCHES:
        out = np.zeros(batch + 1, dtype=np.uint32)
        out[batch] = 0xDEADBEEF  # the word behind the last digest stays
        h.hash(data[:batch * size], size=4 * size, batch=batch, out=out[:batch])
        assert out[:batch].tobytes() == want[:batch].tobytes() and out[batch] == 0xDEADBEEF, batch
    h.close()


# ---- Merkle trees ----------------------------------------------------------------------------------------------------------------------
LEAF_ELEMS, LEAVES = 8, 64
SPECS = [(T, LEAF_ELEMS, None)] + [(2, 2, None)] * 6  # a sponge over 8 elements per leaf, then two-to-one compressions


def make_tree(field):
    from icicle_amd.hash import Hasher
    from icicle_amd.merkle import MerkleTree

    hashers = [Hasher.poseidon2(field, T, input_size=LEAF_ELEMS)] + [Hasher.poseidon2(field, 2) for _ in range(6)]
    tree = MerkleTree(hashers, 4)
    for h in hashers:
        h.close()  # the tree keeps the constants alive
    return tree


@functools.lru_cache(maxsize=None)
def tree_reference(field, valid_elems):
    """leaves (valid_elems of them given, the rest zero padding) and every digest layer from the model"""
    p = pm.FIELDS[field]
    leaves = np.random.default_rng(valid_elems).integers(0, p, size=valid_elems, dtype=np.uint64).astype(np.uint32)
    padded = [int(v) for v in leaves] + [0] * (LEAVES * LEAF_ELEMS - valid_elems)
    return leaves, pm.merkle_layers(field, padded, SPECS)


def expected_path(layers, idx):
    """full path: per layer below the root the whole group of siblings, on-path digest included"""
    out = []
    for layer in layers[:-1]:
        g = idx // 2 * 2
        out += layer[g:g + 2]
        idx //= 2
    return np.array(out, dtype=np.uint32).tobytes()


@pytest.mark.parametrize("field", FIELDS)
def test_tree_root_openings_and_verification(hip, field):
    from icicle_amd.merkle import MerkleProof

    leaves, layers = tree_reference(field, LEAVES * LEAF_ELEMS)
    assert [len(l) for l in layers] == [64, 32, 16, 8, 4, 2, 1]
    root = np.array(layers[-1], dtype=np.uint32).tobytes()
    tree = make_tree(field).build(leaves)
    assert tree.root() == root
    # a proof is asked for by the index of a leaf element (4 bytes) and opens the leaf -- the layer-0 chunk -- that holds it: elements
    # 0, 31 and 63 lie in leaves 0, 3 and 7; the last two open leaves 31 and 63
    indices = [0, 31, 63, 31 * LEAF_ELEMS + 5, 63 * LEAF_ELEMS + 7]
    batch = tree.proofs(leaves, indices)
    for idx, many in zip(indices, batch):
        single, leaf = tree.proof(leaves, idx), idx // LEAF_ELEMS
        assert single.leaf == leaves[leaf * LEAF_ELEMS:(leaf + 1) * LEAF_ELEMS].tobytes() and single.root == root
        assert single.path == expected_path(layers, leaf), idx
        assert (many.leaf, many.root, many.path, many.leaf_idx) == (single.leaf, single.root, single.path, idx)
        assert tree.verify(single)
        pruned = tree.proof(leaves, idx, pruned=True)
        assert len(pruned.path) == len(single.path) // 2 and tree.verify(pruned)
        for at in (0, len(single.path) - 1):  # one flipped byte, in the lowest and in the highest group of the path
            bad = bytearray(single.path)
            bad[at] ^= 1
            forged = MerkleProof.with_data(False, idx, single.leaf, single.root, bytes(bad))
            assert not tree.verify(forged), (idx, at)
        bad_leaf = bytearray(single.leaf)
        bad_leaf[5] ^= 0x10
        assert not tree.verify(MerkleProof.with_data(False, idx, bytes(bad_leaf), single.root, single.path))
    assert tree.verify_batch(batch) == [True] * 5
    bad = bytearray(batch[1].path)
    bad[9] ^= 0x40
    forged = MerkleProof.with_data(False, indices[1], batch[1].leaf, batch[1].root, bytes(bad))
    assert tree.verify_batch([batch[0], forged, batch[4]]) == [True, False, True]
    assert tree.verify_batch(tree.proofs(leaves, indices, pruned=True)) == [True] * 5
    tree.close()


def test_tree_with_zero_padding_over_a_leaf_count_that_is_no_power_of_the_arity(hip):
    import icicle_amd
    from icicle_amd.merkle import PaddingPolicy

    field, valid = "babybear", 37 * LEAF_ELEMS + 3  # the leaves end inside chunk 37: chunks 37 .. 63 reach into the padding
    leaves, layers = tree_reference(field, valid)
    cfg = icicle_amd.MerkleTreeConfig.default()
    cfg.padding_policy = PaddingPolicy.ZERO_PADDING
    tree = make_tree(field).build(leaves, cfg=cfg)
    assert tree.root() == np.array(layers[-1], dtype=np.uint32).tobytes()
    for leaf in (0, 37, 63):  # wholly inside the leaves, across their end, wholly padding
        cfg = icicle_amd.MerkleTreeConfig.default()
        cfg.padding_policy = PaddingPolicy.ZERO_PADDING
        pr = tree.proof(leaves, leaf * LEAF_ELEMS, cfg=cfg)
        assert pr.path == expected_path(layers, leaf) and tree.verify(pr), leaf
    tree.close()
