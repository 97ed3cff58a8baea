"""GPU: Merkle trees (icicle_merkle_tree_*) against the model (tests/merkle_model.py): roots, proofs byte for byte, verify, for
binary Keccak-256 trees of 1 .. 12 layers on the per-layer route, the fused-top route and a switch in mid-tree; a tree of mixed
hashers and one of arity 3; the three padding policies; stored-layer choices; host and device leaves; the error cases; and a tree
built directly on the device output of an NTT."""
import ctypes

import numpy as np
import pytest

from tests import merkle_model as mm

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT = 11
MIXED = ([("sha3_512", 100), ("sha3_256", 256), ("sha3_256", 128), ("sha3_512", 64)], 20)
ARITY3 = ([("keccak256", 96)] * 3, 32)


def binary(L):
    return [("keccak256", 64)] * L, 32


def make_tree(layers, es, store_min=0):
    from icicle_amd.hash import Hasher
    from icicle_amd.merkle import MerkleTree

    hashers = [getattr(Hasher, name)(chunk) for name, chunk in layers]
    return MerkleTree(hashers, es, store_min)


def config(policy=mm.PAD_NONE, tree_on_device=False, top_max=None):
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


def leaves_for(shape, size, seed):
    return np.random.default_rng(seed).integers(0, 256, size, dtype=np.uint8)


def check_proofs(tree, shape, leaves_arg, leaves, policy, cfg, indices):
    from icicle_amd.merkle import MerkleProof

    for idx in indices:
        for pruned in (False, True):
            leaf, path, root = mm.proof(shape, leaves.tobytes(), idx, pruned, policy)
            pr = tree.proof(leaves_arg, idx, pruned, cfg, size=leaves.nbytes)
            assert (pr.pruned, pr.leaf_idx) == (pruned, idx)
            assert pr.leaf == leaf, (idx, pruned)
            assert pr.path == path, (idx, pruned)
            assert pr.root == root
            assert tree.verify(pr) is True
            for what in ("leaf", "path", "root"):
                parts = {"leaf": bytearray(leaf), "path": bytearray(path), "root": bytearray(root)}
                if not parts[what]:
                    continue  # a one-layer tree has no path
                parts[what][len(parts[what]) // 2] ^= 0x10
                bad = MerkleProof.with_data(pruned, idx, bytes(parts["leaf"]), bytes(parts["root"]), bytes(parts["path"]))
                assert tree.verify(bad) is False, (idx, pruned, what)


def proof_indices(shape, leaves_size):
    n = shape.capacity // shape.es
    picks = {0, 1 % n, n // 2, n - 1}
    if leaves_size < shape.capacity:
        picks.add(min(n - 1, leaves_size // shape.es + 1))  # inside the padding
    return sorted(picks)


@pytest.mark.parametrize("top_max", [0, None, 4])
@pytest.mark.parametrize("L", [1, 2, 3, 6, 11, 12])
def test_binary_keccak_tree(hip, L, top_max):
    from icicle_amd._lib import lib

    layers, es = binary(L)
    shape = mm.TreeShape(layers, es)
    leaves = leaves_for(shape, shape.capacity, L)
    cfg, ext = config(top_max=top_max)
    tree = make_tree(layers, es).build(leaves, cfg=cfg)
    assert tree.root() == mm.build(shape, leaves.tobytes())[-1]
    check_proofs(tree, shape, leaves, leaves, mm.PAD_NONE, cfg, proof_indices(shape, leaves.nbytes) if L in (3, 12) else [shape.capacity // es - 1])
    tree.close()
    if ext:
        lib.destroy_config_extension(ext)


@pytest.mark.parametrize("layers,es", [MIXED, ARITY3], ids=["mixed", "arity3"])
@pytest.mark.parametrize("top_max", [0, None, 2])
def test_other_shapes(hip, layers, es, top_max):
    from icicle_amd._lib import lib

    shape = mm.TreeShape(layers, es)
    leaves = leaves_for(shape, shape.capacity, 77)
    cfg, ext = config(top_max=top_max)
    tree = make_tree(layers, es).build(leaves, cfg=cfg)
    assert tree.root() == mm.build(shape, leaves.tobytes())[-1]
    check_proofs(tree, shape, leaves, leaves, mm.PAD_NONE, cfg, proof_indices(shape, leaves.nbytes))
    tree.close()
    if ext:
        lib.destroy_config_extension(ext)


def padding_cases():
    layers, es = binary(6)
    cap = mm.TreeShape(layers, es).capacity
    return ([(mm.PAD_ZERO, s) for s in (1, cap - 35, cap // 2)] + [(mm.PAD_LAST, s) for s in (es, cap - es, cap // 3 // es * es)])


@pytest.mark.parametrize("policy,size", padding_cases())
@pytest.mark.parametrize("top_max", [0, None])
def test_padding(hip, policy, size, top_max):
    from icicle_amd._lib import lib
    from icicle_amd.runtime import DeviceVec

    layers, es = binary(6)
    shape = mm.TreeShape(layers, es)
    leaves = leaves_for(shape, size, size)
    want = mm.build(shape, leaves.tobytes(), policy)[-1]
    for on_device in (False, True):
        cfg, ext = config(policy, top_max=top_max)
        arg = DeviceVec.from_host(leaves) if on_device else leaves
        tree = make_tree(layers, es, store_min=2 if on_device else 0).build(arg, size=size, cfg=cfg)
        assert tree.root() == want, (policy, size, on_device)
        check_proofs(tree, shape, arg, leaves, policy, cfg, proof_indices(shape, size))
        tree.close()
        if ext:
            lib.destroy_config_extension(ext)


def test_padding_mixed_shape_last_value(hip):
    """20-byte elements in 100-byte chunks, 64-byte digests below 32-byte ones"""
    layers, es = MIXED
    shape = mm.TreeShape(layers, es)
    for policy, size in ((mm.PAD_LAST, 7 * es), (mm.PAD_ZERO, 333), (mm.PAD_LAST, shape.capacity - es)):
        leaves = leaves_for(shape, size, size)
        cfg, _ = config(policy)
        tree = make_tree(layers, es, store_min=1).build(leaves, cfg=cfg)
        assert tree.root() == mm.build(shape, leaves.tobytes(), policy)[-1]
        check_proofs(tree, shape, leaves, leaves, policy, cfg, proof_indices(shape, size))
        tree.close()


@pytest.mark.parametrize("tree_on_device", [False, True])
@pytest.mark.parametrize("leaves_on_device", [False, True])
def test_stored_layers_do_not_change_root_or_proofs(hip, tree_on_device, leaves_on_device):
    from icicle_amd.runtime import DeviceVec

    layers, es = binary(6)
    shape = mm.TreeShape(layers, es)
    size = shape.capacity - 3 * es
    leaves = leaves_for(shape, size, 5)
    arg = DeviceVec.from_host(leaves) if leaves_on_device else leaves
    seen = []
    for store_min in (0, 1, 3):
        cfg, _ = config(mm.PAD_LAST, tree_on_device)
        tree = make_tree(layers, es, store_min).build(arg, size=size, cfg=cfg)
        proofs = []
        for idx in proof_indices(shape, size):
            for pruned in (False, True):
                pr = tree.proof(arg, idx, pruned, cfg, size=size)
                assert tree.verify(pr)
                proofs.append((pr.leaf, pr.path, pr.root))
        seen.append((tree.root(), proofs))
        tree.close()
    assert seen[0] == seen[1] == seen[2]
    assert seen[0][0] == mm.build(shape, leaves.tobytes(), mm.PAD_LAST)[-1]
    check = mm.proof(shape, leaves.tobytes(), 0, False, mm.PAD_LAST)
    assert seen[0][1][0] == check


def test_error_cases(hip):
    import icicle_amd
    from icicle_amd.merkle import MerkleProof

    layers, es = binary(4)
    shape = mm.TreeShape(layers, es)
    leaves = leaves_for(shape, shape.capacity, 1)

    def refused(fn):
        with pytest.raises(icicle_amd.IcicleError) as e:
            fn()
        assert e.value.code == INVALID_ARGUMENT

    tree = make_tree(layers, es)
    assert tree.root() is None  # before build
    refused(lambda: tree.proof(leaves, 0))  # proof before build
    refused(lambda: tree.build(leaves[:-es], cfg=config(mm.PAD_NONE)[0]))  # short leaves, no policy
    refused(lambda: tree.build(leaves, size=0, cfg=config(mm.PAD_ZERO)[0]))  # no leaves at all
    refused(lambda: tree.build(leaves[:es + 1], cfg=config(mm.PAD_LAST)[0]))  # LastValue: size no multiple of the element
    refused(lambda: tree.build(np.zeros(shape.capacity + 1, np.uint8), cfg=config(mm.PAD_ZERO)[0]))  # beyond the capacity
    assert tree.root() is None  # none of these built anything
    tree.build(leaves)
    refused(lambda: tree.build(leaves))  # second build
    refused(lambda: tree.proof(leaves, shape.capacity // es))  # element at the capacity
    tree.proof(leaves, shape.capacity // es - 1).close()
    # verify refuses a path of the wrong size rather than reading past it
    good = tree.proof(leaves, 3, True)
    refused(lambda: tree.verify(MerkleProof.with_data(True, 3, good.leaf, good.root, good.path[:-1])))
    tree.close()
    # LastValue needs c_0 to be a multiple of the element size (48-byte elements in 64-byte chunks)
    odd = make_tree(layers, 48)
    refused(lambda: odd.build(leaves[:96], cfg=config(mm.PAD_LAST)[0]))
    odd.close()


def test_async_build_on_a_created_stream(hip):
    from icicle_amd.runtime import DeviceVec, Stream

    layers, es = binary(8)
    shape = mm.TreeShape(layers, es)
    leaves = leaves_for(shape, shape.capacity, 8)
    d = DeviceVec.from_host(leaves)
    st = Stream()
    cfg, _ = config(tree_on_device=True)
    cfg.stream = st.handle
    cfg.is_async = True
    tree = make_tree(layers, es).build(d, cfg=cfg)
    st.synchronize()  # the rule for the root after an asynchronous build
    assert tree.root() == mm.build(shape, leaves.tobytes())[-1]
    pr = tree.proof(d, 17, True, cfg)
    assert (pr.leaf, pr.path, pr.root) == mm.proof(shape, leaves.tobytes(), 17, True)
    tree.close()
    st.destroy()


def test_commit_to_ntt_output_on_device(hip):
    """the STARK step this exists for: a columns-batched BabyBear NTT leaves its result on the device, the tree is built there"""
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
        layers, es = [("keccak256", 32)] + [("keccak256", 64)] * (logn - 1), 16
        shape = mm.TreeShape(layers, es)
        assert shape.capacity == x.nbytes
        tree = make_tree(layers, es).build(d_out, cfg=config(tree_on_device=True)[0])
        result = d_out.to_host(np.uint8)
        assert tree.root() == mm.build(shape, result.tobytes())[-1]
        pr = tree.proof(d_out, 515, True, config(tree_on_device=True)[0])
        assert (pr.leaf, pr.path, pr.root) == mm.proof(shape, result.tobytes(), 515, True)
        assert tree.verify(pr)
        tree.close()
    finally:
        N.release_domain("babybear")
