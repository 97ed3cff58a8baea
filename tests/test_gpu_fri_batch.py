"""GPU: FRI on the batched Merkle calls -- the query phase opens a round's slots with one icicle_hip_merkle_tree_get_proofs, the
verifier checks them with one icicle_hip_merkle_tree_verify_batch. Over the BabyBear extension and one 256-bit field at 2^8 with 8
queries: a proof from the prover verifies, its slots are what single openings of the round's tree give, and one corrupted Merkle
path byte in the LAST slot of the LAST round, then in the first slot of round 0 -- the two ends of what the verifier's batches
cover -- makes the verdict false with SUCCESS. (That the proofs did not move by a byte is the fixture tests' to say:
tests/test_gpu_fri.py, tests/test_gpu_fri_wide.py.)"""
import contextlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LOGN, QUERIES = 8, 8
KINDS = [("babybear", True, 4, 2013265921), ("bn254", False, 8, None)]


@contextlib.contextmanager
def domain(field, logn):
    from icicle_amd import ntt

    ntt.release_domain(field)
    ntt.init_domain(field, ntt.get_root_of_unity(field, 1 << logn))
    try:
        yield
    finally:
        ntt.release_domain(field)


def elements(words, p, rng):
    if p is not None:
        return rng.integers(0, p, size=(1 << LOGN, words), dtype=np.uint32)
    x = rng.integers(0, 1 << 32, size=(1 << LOGN, words), dtype=np.uint32)
    x[:, -1] &= 0x0FFFFFFF  # below every 256-bit modulus here
    return x


def rebuilt(field, ext, slots, final_poly, nonce, change=None):
    """a proof object from the slots' data; change = (slot, round, byte of the path to flip)"""
    from icicle_amd import FriProof
    from icicle_amd.merkle import MerkleProof

    rows = []
    for q, row in enumerate(slots):
        out = []
        for r, (idx, leaf, root, path) in enumerate(row):
            if change is not None and change[:2] == (q, r):
                path = path[:change[2]] + bytes([path[change[2]] ^ 0x20]) + path[change[2] + 1:]
            out.append(MerkleProof.with_data(False, idx, leaf, root, path))
        rows.append(out)
    return FriProof.create_with_arguments(field, rows, final_poly, nonce, extension=ext)


@pytest.mark.parametrize("field,ext,words,p", KINDS, ids=["babybear_ext", "bn254"])
def test_prove_and_verify_on_the_batched_calls(hip, field, ext, words, p):
    import icicle_amd
    from icicle_amd.hash import Hasher
    from icicle_amd.merkle import MerkleTree

    x = elements(words, p, np.random.default_rng(words))
    th, lh, ch = Hasher.keccak256(), Hasher.blake2s(4 * words), Hasher.blake2s(64)
    tc = icicle_amd.FriTranscriptConfig.new_default_labels(th, 1)

    def cfg():
        c = icicle_amd.FriConfig.default()
        c.nof_queries, c.pow_bits, c.stopping_degree = QUERIES, 4, 0
        return c

    with domain(field, LOGN):
        proof = icicle_amd.fri_merkle_tree_prove(field, cfg(), tc, x, lh, ch, 0, extension=ext)
    assert (proof.nof_queries, proof.nof_rounds) == (2 * QUERIES, LOGN)
    assert icicle_amd.fri_merkle_tree_verify(field, cfg(), tc, proof, lh, ch, extension=ext) is True
    slots = [[(mp.leaf_idx, mp.leaf, mp.root, mp.path) for mp in row] for row in proof.slots()]
    final_poly, nonce = proof.final_poly, proof.pow_nonce

    # round 0 commits to the input itself: its slots are what single openings of that tree give
    tree = MerkleTree([lh] + [ch] * LOGN, 4 * words).build(x.reshape(-1).view(np.uint8))
    for row in slots:
        idx, leaf, root, path = row[0]
        one = tree.proof(x.reshape(-1).view(np.uint8), idx)
        assert (one.leaf, one.root, one.path) == (leaf, root, path)
    assert tree.verify_batch([mp for row in proof.slots() for mp in row[:1]]) == [True] * (2 * QUERIES)
    tree.close()

    assert icicle_amd.fri_merkle_tree_verify(field, cfg(), tc, rebuilt(field, ext, slots, final_poly, nonce), lh, ch, extension=ext) is True
    last_path = len(slots[-1][-1][3])
    for change in ((2 * QUERIES - 1, LOGN - 1, last_path - 1), (0, 0, 0), (0, 0, len(slots[0][0][3]) - 1), (2 * QUERIES - 1, LOGN - 1, 0)):
        bad = rebuilt(field, ext, slots, final_poly, nonce, change)
        # raises unless the call returns SUCCESS
        assert icicle_amd.fri_merkle_tree_verify(field, cfg(), tc, bad, lh, ch, extension=ext) is False, change
