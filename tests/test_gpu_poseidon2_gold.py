"""GPU: Poseidon2 over Goldilocks through the C ABI -- every recorded digest of the reference
(tests/golden/poseidon2_vectors_gold.json) byte for byte with host and with device operands, batches at the wave and block edges of
a lane-per-hash kernel against the model (tests/poseidon2_model_gold.py), Merkle trees whose layers are these hashers (root,
openings, batched openings, verification, zero padding), FRI over Goldilocks and its quadratic extension with these trees against
the proofs of the reference (tests/golden/fri_vectors_gold_poseidon2.json), and a tree over the device output of extension_ntt."""
import contextlib
import functools
import json
import os

import numpy as np
import pytest

from tests import fri_model_wide as fw
from tests import poseidon2_model_gold as pg

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
P = pg.P
TAG = 7
BATCHES = (1, 63, 64, 65, 255, 256, 257, 1025)  # one lane; around a wave; around a block of 256; past four blocks
EDGE_WIDTHS = (3, 8, 12, 24)
PERIOD = 131  # distinct messages of an edge batch: a prime above the wave, so no wave or block edge falls on a repetition


@functools.lru_cache(maxsize=None)
def vectors():
    with open(os.path.join(HERE, "golden", "poseidon2_vectors_gold.json")) as f:
        return json.load(f)["cases"]


with open(os.path.join(HERE, "golden", "fri_vectors_gold_poseidon2.json")) as _f:
    FRI_CASES = json.load(_f)["cases"]


def words(hexes):
    return np.array([int(v, 16) for v in hexes], dtype=np.uint64)


def tag_of(c):
    return None if c["tag"] is None else int(c["tag"], 16)


def make(t, tag=None, input_size=0):
    from icicle_amd.hash import Hasher

    return Hasher.poseidon2_goldilocks(t, domain_tag=tag, input_size=input_size)


def test_every_recorded_digest_with_host_operands(hip):
    hashers = {}
    for c in vectors():
        key = (c["t"], tag_of(c))
        if key not in hashers:
            hashers[key] = make(*key)
        out = np.zeros(c["batch"], dtype=np.uint64)
        hashers[key].hash(words(c["input"]), size=8 * c["size"], batch=c["batch"], out=out)
        assert out.tobytes() == words(c["digests"]).tobytes(), key + (c["size"], c["batch"])
    assert len(hashers) == 8 * 3  # no tag, tag 7 and the tag above 2^32
    for h in hashers.values():
        h.close()


def test_every_recorded_digest_with_device_operands_on_a_created_stream(hip):
    import icicle_amd
    from icicle_amd.runtime import DeviceVec, Stream

    st = Stream()
    hashers, pending = {}, []
    for c in vectors():
        key = (c["t"], tag_of(c))
        if key not in hashers:
            hashers[key] = make(*key)
        d_in, d_out = DeviceVec.from_host(words(c["input"])), DeviceVec(8 * c["batch"])
        cfg = icicle_amd.HashConfig.default()
        cfg.stream, cfg.is_async = st.handle, True
        hashers[key].hash(d_in, size=8 * c["size"], batch=c["batch"], out=d_out, cfg=cfg)
        pending.append((c, d_in, d_out))
    st.synchronize()
    for c, _, d_out in pending:
        assert d_out.to_host(np.uint64).tobytes() == words(c["digests"]).tobytes(), (c["t"], c["tag"], c["size"], c["batch"])
    st.destroy()
    for h in hashers.values():
        h.close()


def test_words_at_or_above_p_count_as_their_residue(hip):
    h = make(8)
    msg = np.array([P, P + 5, (1 << 64) - 1, 3, 0, P - 1, 1, 2], dtype=np.uint64)
    out = np.zeros(1, dtype=np.uint64)
    h.hash(msg, size=64, batch=1, out=out)
    assert int(out[0]) == pg.hash_one(8, [int(v) % P for v in msg])
    h.close()


@functools.lru_cache(maxsize=None)
def edge_reference(t, size, tag):
    """max(BATCHES) messages of `size` elements, message i a copy of message i % PERIOD, and their digests from the model; a smaller
    batch is a prefix of both"""
    n = max(BATCHES)
    base = np.random.default_rng(100 * t + size).integers(0, P, size=PERIOD * size, dtype=np.uint64)
    base[:3] = (P - 1, 0, 1)
    digests = pg.hash_batch(t, [int(v) for v in base], size, tag)
    reps = -(-n // PERIOD)
    data = np.tile(base.reshape(PERIOD, size), (reps, 1))[:n].copy()
    return data, np.array((digests * reps)[:n], dtype=np.uint64)


@pytest.mark.parametrize("shape", ["exact", "tagged", "sponge"])
@pytest.mark.parametrize("t", EDGE_WIDTHS)
def test_batches_at_wave_and_block_edges(hip, t, shape):
    size, tag = {"exact": (t, None), "tagged": (t - 1, TAG), "sponge": (2 * t - 1, None)}[shape]
    data, want = edge_reference(t, size, tag)
    h = make(t, tag)
    for batch in BATCHES:
        out = np.zeros(batch + 1, dtype=np.uint64)
        out[batch] = 0xDEADBEEFDEADBEEF  # the word behind the last digest stays
        h.hash(data[:batch].reshape(-1), size=8 * size, batch=batch, out=out[:batch])
        assert out[:batch].tobytes() == want[:batch].tobytes() and out[batch] == 0xDEADBEEFDEADBEEF, batch
    h.close()


def test_a_stride_larger_than_the_length(hip):
    """icicle_hasher_hash packs its messages back to back, so the launcher sees a stride above the length where a tree verifies a
    batch of proofs: the leaves lie in rows padded to 16 bytes, and a leaf of 9 elements (72 bytes) has a stride of 80"""
    from icicle_amd.merkle import MerkleTree

    elems = 9
    rows = np.random.default_rng(6).integers(0, P, size=64 * elems, dtype=np.uint64)
    leaf, node = make(12, input_size=elems), make(2)
    tree = MerkleTree([leaf] + [node] * 6, 8).build(rows)
    layers = pg.merkle_layers([int(v) for v in rows], [(12, elems, None)] + [(2, 2, None)] * 6)
    assert tree.root() == pg.to_bytes(layers[-1])
    proofs = tree.proofs(rows, [elems * i + i % elems for i in range(64)])
    assert tree.verify_batch(proofs) == [True] * 64
    leaf.close(), node.close(), tree.close()


# ---- Merkle trees ----------------------------------------------------------------------------------------------------------------------
LEAF_T, LEAF_ELEMS, LEAVES = 12, 8, 64
SPECS = [(LEAF_T, LEAF_ELEMS, None)] + [(2, 2, None)] * 6  # one permutation over the 8 elements of a leaf, then two-to-one compressions


def make_tree():
    from icicle_amd.merkle import MerkleTree

    hashers = [make(LEAF_T, input_size=LEAF_ELEMS)] + [make(2) for _ in range(6)]
    tree = MerkleTree(hashers, 8)
    for h in hashers:
        h.close()  # the tree keeps the constants alive
    return tree


@functools.lru_cache(maxsize=None)
def tree_reference(valid_elems):
    """leaves (valid_elems of them given, the rest zero padding) and every digest layer from the model"""
    leaves = np.random.default_rng(valid_elems).integers(0, P, size=valid_elems, dtype=np.uint64)
    padded = [int(v) for v in leaves] + [0] * (LEAVES * LEAF_ELEMS - valid_elems)
    return leaves, pg.merkle_layers(padded, SPECS)


def expected_path(layers, idx):
    """full path: per layer below the root the whole group of siblings, on-path digest included"""
    out = []
    for layer in layers[:-1]:
        g = idx // 2 * 2
        out += layer[g:g + 2]
        idx //= 2
    return pg.to_bytes(out)


def test_tree_root_openings_and_verification(hip):
    from icicle_amd.merkle import MerkleProof

    leaves, layers = tree_reference(LEAVES * LEAF_ELEMS)
    assert [len(l) for l in layers] == [64, 32, 16, 8, 4, 2, 1]
    root = pg.to_bytes(layers[-1])
    tree = make_tree().build(leaves)
    assert tree.root() == root
    # a proof is asked for by the index of a leaf element (8 bytes) and opens the leaf -- the layer-0 chunk -- that holds it
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
            assert not tree.verify(MerkleProof.with_data(False, idx, single.leaf, single.root, bytes(bad))), (idx, at)
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


def test_tree_with_zero_padding_over_37_leaves(hip):
    import icicle_amd
    from icicle_amd.merkle import PaddingPolicy

    valid = 37 * LEAF_ELEMS + 3  # the leaves end inside chunk 37: it straddles the end of the data, chunks 38 .. 63 are all padding
    leaves, layers = tree_reference(valid)
    cfg = icicle_amd.MerkleTreeConfig.default()
    cfg.padding_policy = PaddingPolicy.ZERO_PADDING
    tree = make_tree().build(leaves, cfg=cfg)
    assert tree.root() == pg.to_bytes(layers[-1])
    for leaf in (0, 37, 63):  # wholly inside the leaves, across their end, wholly padding
        cfg = icicle_amd.MerkleTreeConfig.default()
        cfg.padding_policy = PaddingPolicy.ZERO_PADDING
        pr = tree.proof(leaves, leaf * LEAF_ELEMS, cfg=cfg)
        assert pr.path == expected_path(layers, leaf) and tree.verify(pr), leaf
    tree.close()


# ---- FRI ---------------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def domain(logn):
    from icicle_amd import ntt

    ntt.release_domain("goldilocks")
    ntt.init_domain("goldilocks", ntt.get_root_of_unity("goldilocks", 1 << logn))
    try:
        yield
    finally:
        ntt.release_domain("goldilocks")


def to_array(F, elems):
    return np.frombuffer(F.raw(elems), dtype=np.uint32).reshape(-1, F.words).copy()


def fri_setup(case):
    from icicle_amd import FriConfig, FriTranscriptConfig
    from icicle_amd.hash import Hasher

    F = fw.case_field(case)
    th = Hasher.keccak256()
    lh, ch = (make(s["t"], s["tag"], s["input_size"]) for s in (case["leaves_hash"], case["compress_hash"]))
    labels = tuple(s.encode() for s in case["labels"])
    seed = np.frombuffer(bytes.fromhex(case["seed"]), dtype=np.uint32)

    def transcript():
        return FriTranscriptConfig(th, *labels, bytes.fromhex(case["public_state"]), seed)

    def config():
        c = FriConfig.default()
        c.stopping_degree, c.pow_bits, c.nof_queries = case["stopping_degree"], case["pow_bits"], case["nof_queries"]
        return c

    return F, lh, ch, transcript, config


def read_proof(F, proof):
    return {"final_poly": F.elements(proof.final_poly.tobytes()), "nonce": proof.pow_nonce,
            "slots": [[(mp.leaf_idx, mp.leaf, mp.root, mp.path) for mp in row] for row in proof.slots()]}


def rebuild(case, pr):
    """a device proof from the fixture's form, through create_with_arguments"""
    from icicle_amd import FriProof
    from icicle_amd.merkle import MerkleProof

    rows = [[MerkleProof.with_data(False, idx, leaf, root, path) for idx, leaf, root, path in row] for row in pr["slots"]]
    fp = np.frombuffer(b"".join(pr["final_poly"]), dtype=np.uint32)
    return FriProof.create_with_arguments(case["field"], rows, fp, pr["nonce"], extension=case["extension"])


def flip_first_bit(b: bytes) -> bytes:
    return bytes([b[0] ^ 1]) + b[1:]


@pytest.mark.parametrize("case", FRI_CASES, ids=[c["name"] for c in FRI_CASES])
def test_fri_prove_equals_the_reference_and_verify_rejects_a_flipped_bit(hip, case):
    import icicle_amd

    F, lh, ch, transcript, config = fri_setup(case)
    want = fw.case_proof(case)
    x = to_array(F, fw.case_elements(case))
    with domain(case["log_domain"]):
        proof = icicle_amd.fri_merkle_tree_prove("goldilocks", config(), transcript(), x, lh, ch, 0, extension=F.ext)
        got = read_proof(F, proof)
        assert got["final_poly"] == want["final_poly"] and got["nonce"] == want["nonce"] and len(got["slots"]) == len(want["slots"])
        for q, (g, w) in enumerate(zip(got["slots"], want["slots"])):
            assert len(g) == len(w), q
            for r, (a, b) in enumerate(zip(g, w)):
                assert a == b, ("slot", q, "round", r)  # leaf index, leaf, root and path, byte for byte
        assert icicle_amd.fri_merkle_tree_verify("goldilocks", config(), transcript(), proof, lh, ch, extension=F.ext)

        def recorded():
            pr = fw.case_proof(case)
            pr["final_poly"] = [F.to_bytes(e) for e in pr["final_poly"]]
            return pr

        assert icicle_amd.fri_merkle_tree_verify("goldilocks", config(), transcript(), rebuild(case, recorded()), lh, ch, extension=F.ext)
        pr = recorded()
        idx, leaf, root, path = pr["slots"][2][1]
        pr["slots"][2][1] = (idx, leaf, root, flip_first_bit(path))
        assert not icicle_amd.fri_merkle_tree_verify("goldilocks", config(), transcript(), rebuild(case, pr), lh, ch, extension=F.ext), "path bit"
        pr = recorded()
        k = pr["slots"][0][-1][0] % len(pr["final_poly"])  # the coefficient the first query reads
        pr["final_poly"][k] = flip_first_bit(pr["final_poly"][k])
        assert not icicle_amd.fri_merkle_tree_verify("goldilocks", config(), transcript(), rebuild(case, pr), lh, ch, extension=F.ext), "final polynomial bit"
    lh.close(), ch.close()


# ---- NTT -> tree, on the device -------------------------------------------------------------------------------------------------------------
def test_a_tree_over_the_device_output_of_extension_ntt(hip):
    from icicle_amd import ntt
    from icicle_amd.merkle import MerkleTree
    from icicle_amd.runtime import DeviceVec

    logn = 8
    x = np.random.default_rng(8).integers(0, P, size=2 << logn, dtype=np.uint64).view(np.uint32)
    with domain(logn):
        d_in, d_out = DeviceVec.from_host(x), DeviceVec(x.nbytes)
        ntt.ntt("goldilocks", d_in, ntt.FORWARD, out=d_out, size=1 << logn, extension=True)
        y = d_out.to_host(np.uint32)
    assert not np.array_equal(y, x)

    def tree():
        hashers = [make(3, input_size=2)] + [make(2) for _ in range(logn)]  # a leaf is one extension element: two coefficients
        t = MerkleTree(hashers, 16)
        for h in hashers:
            h.close()
        return t

    on_device, on_host = tree().build(d_out), tree().build(y)
    assert on_device.root() == on_host.root() and len(on_host.root()) == 8
    elems = pg.from_bytes(y.tobytes())
    assert on_host.root() == pg.to_bytes(pg.merkle_layers(elems, [(3, 2, None)] + [(2, 2, None)] * logn)[-1])
    on_device.close(), on_host.close()
