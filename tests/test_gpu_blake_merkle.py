"""GPU: Merkle trees over Blake2s / Blake3 layers (icicle_merkle_tree_*) against the model (tests/blake_model.py): roots, proofs byte
for byte, verify -- binary Blake3 trees on the per-layer route, the fused-top route and a switch in mid-tree; a tree that mixes
Blake2s, Blake3 and Keccak-256; Blake3 layers of more than one 1024-byte chunk, as the padded leaf layer and as an inner layer the
fused top has to start above; stored-layer choices with host and device operands; a tree built on the device output of an NTT."""
import numpy as np
import pytest

from tests import blake_model as bm

pytestmark = pytest.mark.gpu

MIXED = ([("blake2s", 100), ("blake3", 128), ("blake3", 128), ("keccak256", 64)], 20)  # 32 leaf chunks, arity 4, 4, 2
LONG_LEAVES = ([("blake3", 1536), ("blake3", 128), ("blake2s", 64)], 4)                # 8 leaf chunks of 1.5 Blake3 chunks
LONG_INNER = ([("blake3", 64), ("blake3", 2048), ("blake3", 64)], 32)                  # arity 64: inputs of two Blake3 chunks


def binary(L):
    return [("blake3", 64)] * L, 32


def make_tree(layers, es, store_min=0):
    from icicle_amd.hash import Hasher
    from icicle_amd.merkle import MerkleTree

    return MerkleTree([getattr(Hasher, name)(chunk) for name, chunk in layers], es, store_min)


def config(policy=bm.PAD_NONE, tree_on_device=False, top_max=None):
    """(cfg, ext handle to destroy or None)"""
    import icicle_amd
    from icicle_amd._lib import lib

    cfg = icicle_amd.MerkleTreeConfig.default()
    cfg.padding_policy = policy
    cfg.is_tree_on_device = tree_on_device
    ext = None
    if top_max is not None:
        ext = lib.create_config_extension()
        lib.config_extension_set_int(ext, b"hip_merkle_top_max_hashes", top_max)
        cfg.ext = ext
    return cfg, ext


def release(ext):
    from icicle_amd._lib import lib

    if ext:
        lib.destroy_config_extension(ext)


def leaves_for(size, seed):
    return np.random.default_rng(seed).integers(0, 256, size, dtype=np.uint8)


def proof_indices(shape):
    """first, second, middle, last element"""
    n = shape.capacity // shape.es
    return sorted({0, 1 % n, n // 2, n - 1})


def check_proofs(tree, shape, leaves_arg, leaves, policy, cfg, indices):
    from icicle_amd.merkle import MerkleProof

    for idx in indices:
        for pruned in (False, True):
            leaf, path, root = bm.proof(shape, leaves.tobytes(), idx, pruned, policy)
            pr = tree.proof(leaves_arg, idx, pruned, cfg, size=leaves.nbytes)
            assert (pr.pruned, pr.leaf_idx) == (pruned, idx)
            assert pr.leaf == leaf, (idx, pruned)
            assert pr.path == path, (idx, pruned)
            assert pr.root == root
            assert tree.verify(pr) is True
            bad = bytearray(path)
            bad[len(bad) // 2] ^= 0x10
            assert tree.verify(MerkleProof.with_data(pruned, idx, leaf, root, bytes(bad))) is False, (idx, pruned)


@pytest.mark.parametrize("L", [5, 12])
def test_binary_blake3_tree_fused_and_per_layer_routes_agree(hip, L):
    layers, es = binary(L)
    shape = bm.TreeShape(layers, es)
    leaves = leaves_for(shape.capacity, L)
    want = bm.build(shape, leaves.tobytes())[-1]
    roots = []
    for top_max in (0, 4, None):
        cfg, ext = config(top_max=top_max)
        tree = make_tree(layers, es).build(leaves, cfg=cfg)
        roots.append(tree.root())
        check_proofs(tree, shape, leaves, leaves, bm.PAD_NONE, cfg, proof_indices(shape) if top_max == 4 else [shape.capacity // es - 1])
        tree.close()
        release(ext)
    assert roots == [want] * 3


@pytest.mark.parametrize("top_max", [0, None, 2])
def test_mixed_blake2s_blake3_keccak_tree(hip, top_max):
    layers, es = MIXED
    shape = bm.TreeShape(layers, es)
    assert shape.count == [32, 8, 2, 1]
    for policy, size in ((bm.PAD_NONE, shape.capacity), (bm.PAD_LAST, 7 * es), (bm.PAD_ZERO, 333)):
        leaves = leaves_for(size, size)
        cfg, ext = config(policy, top_max=top_max)
        tree = make_tree(layers, es).build(leaves, cfg=cfg)
        assert tree.root() == bm.build(shape, leaves.tobytes(), policy)[-1], (policy, size)
        check_proofs(tree, shape, leaves, leaves, policy, cfg, proof_indices(shape))
        tree.close()
        release(ext)


def long_leaf_cases():
    layers, es = LONG_LEAVES
    cap = bm.TreeShape(layers, es).capacity
    # the leaves end inside the first Blake3 chunk, on a Blake3 chunk edge inside a leaf chunk, on a leaf chunk edge, one element short
    sizes = (700, 1536 + 1024, 3 * 1536, cap - es)
    return [(policy, s) for policy in (bm.PAD_ZERO, bm.PAD_LAST) for s in sizes]


@pytest.mark.parametrize("policy,size", long_leaf_cases())
def test_blake3_leaf_chunks_of_more_than_one_chunk_with_padding(hip, policy, size):
    from icicle_amd.runtime import DeviceVec

    layers, es = LONG_LEAVES
    shape = bm.TreeShape(layers, es)
    assert shape.count == [8, 2, 1]
    leaves = leaves_for(size, size)
    want = bm.build(shape, leaves.tobytes(), policy)[-1]
    for on_device in (False, True):
        cfg, ext = config(policy, top_max=None if on_device else 0)
        arg = DeviceVec.from_host(leaves) if on_device else leaves
        tree = make_tree(layers, es, store_min=1 if on_device else 0).build(arg, size=size, cfg=cfg)
        assert tree.root() == want, (policy, size, on_device)
        check_proofs(tree, shape, arg, leaves, policy, cfg, proof_indices(shape))
        tree.close()
        release(ext)


@pytest.mark.parametrize("top_max", [0, None, 1])
def test_fused_top_starts_above_a_long_blake3_layer(hip, top_max):
    """layer 1 hashes two inputs of 2048 bytes: few enough for the fused top, but not one Blake3 chunk each"""
    layers, es = LONG_INNER
    shape = bm.TreeShape(layers, es)
    assert shape.count == [128, 2, 1]
    leaves = leaves_for(shape.capacity, 3)
    cfg, ext = config(top_max=top_max)
    tree = make_tree(layers, es).build(leaves, cfg=cfg)
    assert tree.root() == bm.build(shape, leaves.tobytes())[-1]
    check_proofs(tree, shape, leaves, leaves, bm.PAD_NONE, cfg, proof_indices(shape))
    tree.close()
    release(ext)


@pytest.mark.parametrize("tree_on_device", [False, True])
@pytest.mark.parametrize("leaves_on_device", [False, True])
def test_stored_layers_do_not_change_root_or_proofs(hip, tree_on_device, leaves_on_device):
    from icicle_amd.runtime import DeviceVec

    layers, es = MIXED
    shape = bm.TreeShape(layers, es)
    size = shape.capacity - 3 * es
    leaves = leaves_for(size, 5)
    arg = DeviceVec.from_host(leaves) if leaves_on_device else leaves
    seen = []
    for store_min in (0, 2):
        cfg, _ = config(bm.PAD_LAST, tree_on_device)
        tree = make_tree(layers, es, store_min).build(arg, size=size, cfg=cfg)
        proofs = []
        for idx in proof_indices(shape):
            for pruned in (False, True):
                pr = tree.proof(arg, idx, pruned, cfg, size=size)
                assert tree.verify(pr)
                proofs.append((pr.leaf, pr.path, pr.root))
        seen.append((tree.root(), proofs))
        tree.close()
    assert seen[0] == seen[1]
    assert seen[0][0] == bm.build(shape, leaves.tobytes(), bm.PAD_LAST)[-1]
    assert seen[0][1][0] == bm.proof(shape, leaves.tobytes(), 0, False, bm.PAD_LAST)


def test_commit_to_ntt_output_on_device(hip):
    """the STARK step this exists for: a columns-batched BabyBear NTT leaves its result on the device, the Blake3 tree is built there"""
    import icicle_amd
    from icicle_amd import ntt as N
    from icicle_amd.runtime import DeviceVec
    from oracle import pyref

    logn, cols = 10, 4
    n = 1 << logn
    x = np.random.default_rng(2).integers(0, pyref.BABYBEAR.p, n * cols, dtype=np.uint32)
    N.init_domain("babybear", N.get_root_of_unity("babybear", n))
    try:
        cfg = icicle_amd.NTTConfigU32.default()
        cfg.batch_size = cols
        cfg.columns_batch = True
        d_out = DeviceVec(x.nbytes)
        N.ntt("babybear", x, N.FORWARD, cfg, out=d_out)
        # one leaf element = one row of the trace (4 columns x 4 bytes); two rows per 32-byte layer-0 input
        layers, es = [("blake3", 32)] + [("blake3", 64)] * (logn - 1), 16
        shape = bm.TreeShape(layers, es)
        assert shape.capacity == x.nbytes
        tree = make_tree(layers, es).build(d_out, cfg=config(tree_on_device=True)[0])
        result = d_out.to_host(np.uint8)
        assert tree.root() == bm.build(shape, result.tobytes())[-1]
        pr = tree.proof(d_out, 515, True, config(tree_on_device=True)[0])
        assert (pr.leaf, pr.path, pr.root) == bm.proof(shape, result.tobytes(), 515, True)
        assert tree.verify(pr)
        tree.close()
    finally:
        N.release_domain("babybear")
