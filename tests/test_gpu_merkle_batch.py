"""GPU: batched Merkle openings and verification (icicle_hip_merkle_tree_get_proofs / _verify_batch) against the model of all six
hashers (tests/blake_model.py) field by field (leaf, leaf_idx, path, root, pruned) for every index opened and every verdict -- the
single calls are the same code with count == 1, so they are no oracle --, and the single calls against the batch of one at the C ABI
on the smallest shapes that reach each branch: chunks of one and of four elements, an arity-4 layer, Keccak-512 and Blake2s layers
in one tree; one layer (an empty path), two layers, 2^6 and 2^10 leaf chunks; single indices, every index, 300 unsorted indices with repeats; the padded tail under both policies; host and device
leaves, leaves off a 16-byte boundary, a tree in pinned memory, layers below the first stored one re-hashed for 1, 2 and many
sub-trees; refusals that leave the proofs empty; a stream of its own; and verify_batch for all six hashers with one bit flipped
in one proof at a time."""
import ctypes

import numpy as np
import pytest

from tests import blake_model as bm
from tests import merkle_model as mm

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT = 11
OUT = {"keccak256": 32, "keccak512": 64, "sha3_256": 32, "sha3_512": 64, "blake2s": 32, "blake3": 32}
ES = 4


def tree_layers(kind, L):
    """(name, chunk) per layer, leaf layer first; elements of 4 bytes"""
    if kind == "k1":  # a chunk of one element
        return [("keccak256", 4)] + [("keccak256", 64)] * (L - 1)
    if kind == "k4":  # a chunk of four elements
        return [("keccak256", 16)] + [("keccak256", 64)] * (L - 1)
    if kind == "arity4":  # layer 1 takes four digests
        return [("keccak256", 4)] + [("keccak256", 128)] * min(L - 1, 1) + [("keccak256", 64)] * max(L - 2, 0)
    if kind == "mixed":  # 64-byte Keccak-512 digests under Blake2s, 32-byte Blake2s digests under Keccak-512
        return [("keccak512", 16)] + [("blake2s", 128) if i % 2 else ("keccak512", 64) for i in range(1, L)]
    raise ValueError(kind)


class Shape:
    """what the tests need of a tree's arithmetic, for all six hashers (merkle_model.TreeShape knows the Keccak ones)"""

    def __init__(self, layers, es=ES):
        self.layers, self.es = layers, es
        self.chunk = [c for _, c in layers]
        self.out = [OUT[n] for n, _ in layers]
        n = 1
        for i in range(len(layers) - 1, 0, -1):
            n *= self.chunk[i] // self.out[i - 1]
        self.n0 = n
        self.capacity = n * self.chunk[0]
        self.elements = self.capacity // es

    def group_offsets(self, pruned):
        """offset of every layer's group in the path"""
        offs, at = [], 0
        for i in range(1, len(self.layers)):
            offs.append(at)
            at += self.chunk[i] - (self.out[i - 1] if pruned else 0)
        return offs


def make_tree(layers, store_min=0, es=ES):
    from icicle_amd.hash import Hasher
    from icicle_amd.merkle import MerkleTree

    return MerkleTree([getattr(Hasher, name)(chunk) for name, chunk in layers], es, store_min)


def config(policy=mm.PAD_NONE, tree_on_device=True):
    import icicle_amd

    cfg = icicle_amd.MerkleTreeConfig.default()
    cfg.padding_policy, cfg.is_tree_on_device = policy, tree_on_device
    return cfg


def fields(p):
    return p.leaf, p.leaf_idx, p.path, p.root, p.pruned


def model_of(layers, leaves, policy=mm.PAD_NONE, es=ES):
    """(shape, leaves bytes, policy) as check_against_model takes it; the model's build of the tree is cached"""
    return bm.TreeShape(layers, es), leaves.tobytes(), policy


def check_against_model(tree, arg, size, indices, pruned, cfg, model):
    """every proof of the batch equals the model's proof for its index; model: (shape, leaves bytes, policy)"""
    got = tree.proofs(arg, indices, pruned, cfg, size=size)
    assert len(got) == len(indices)
    shape, leaves, policy = model
    want = {}
    for i, pr in zip(indices, got):
        if i not in want:
            leaf, path, root = bm.proof(shape, leaves, i, pruned, policy)
            want[i] = (leaf, i, path, root, pruned)
        assert fields(pr) == want[i], (i, pruned)
    return got


def verdict(shape, pr):
    """the model's verdict on a proof (MerkleProof or its fields)"""
    leaf, idx, path, root, pruned = pr if isinstance(pr, tuple) else fields(pr)
    return bm.verify(shape, leaf, idx, path, root, pruned)


def random_leaves(size, seed):
    return np.random.default_rng(seed).integers(0, 256, size, dtype=np.uint8)


@pytest.mark.parametrize("on_device", [False, True], ids=["host_leaves", "device_leaves"])
@pytest.mark.parametrize("pruned", [False, True], ids=["full", "pruned"])
@pytest.mark.parametrize("kind", ["k1", "k4", "arity4", "mixed"])
def test_batch_equals_single_calls(hip, kind, pruned, on_device):
    """every proof of every batch against the model (the single calls run the batch's code: test_single_calls_are_batches_of_one)"""
    from icicle_amd.runtime import DeviceVec

    rng = np.random.default_rng(17)
    for L in (1, 2, 7, 11):
        layers = tree_layers(kind, L)
        shape = Shape(layers)
        leaves = random_leaves(shape.capacity, L)
        arg = DeviceVec.from_host(leaves) if on_device else leaves
        cfg = config()
        tree = make_tree(layers).build(arg, cfg=cfg)
        n = shape.elements
        model = model_of(layers, leaves)
        sets = [[0], [n - 1], [n // 2, n // 2]]
        if L == 7:
            sets.append(list(range(n)))  # every index of the 2^6 tree
        if L == 11:
            sets.append([int(v) for v in rng.integers(0, n, 300)])  # unsorted, with repeats, several blocks of the gather
            assert len(set(sets[-1])) < 300
        for indices in sets:
            got = check_against_model(tree, arg, leaves.nbytes, indices, pruned, cfg, model)
            assert all(len(p.path) == (0 if L == 1 else sum(shape.chunk[1:]) - (sum(shape.out[:-1]) if pruned else 0)) for p in got)
            assert tree.verify_batch(got[:70]) == [True] * len(got[:70])
        tree.close()


@pytest.mark.parametrize("on_device", [False, True], ids=["host_leaves", "device_leaves"])
@pytest.mark.parametrize("policy,size", [(mm.PAD_ZERO, 503), (mm.PAD_LAST, 500), (mm.PAD_ZERO, 1), (mm.PAD_LAST, 4)], ids=["zero_503", "last_500", "zero_1", "last_4"])
def test_padded_tail(hip, policy, size, on_device):
    """a short input: the chunk the input ends in, chunks wholly in the padding, the last element, the last index"""
    from icicle_amd.runtime import DeviceVec

    layers = tree_layers("k4", 7)  # 64 chunks of 16 bytes
    shape = Shape(layers)
    leaves = random_leaves(size, size)
    arg = DeviceVec.from_host(leaves) if on_device else leaves
    for store_min in (0, 2):
        cfg = config(policy)
        tree = make_tree(layers, store_min).build(arg, size=size, cfg=cfg)
        last = (size - 1) // ES
        indices = [shape.elements - 1, last, 0, min(last + 1, shape.elements - 1), min(last + 9, shape.elements - 1), shape.elements // 2, last]
        for pruned in (False, True):
            got = check_against_model(tree, arg, size, indices, pruned, cfg, model_of(layers, leaves, policy))
            assert tree.verify_batch(got) == [True] * len(got)
        tree.close()


@pytest.mark.parametrize("tree_on_device", [False, True], ids=["pinned_tree", "device_tree"])
@pytest.mark.parametrize("on_device", [False, True], ids=["host_leaves", "device_leaves"])
def test_stored_layers(hip, tree_on_device, on_device):
    """is_tree_on_device false, and output_store_min_layer 2 (sub-trees of 4 chunks = 16 elements), the top layer and beyond it, with
    indices that fall into one sub-tree, two, and many"""
    from icicle_amd.runtime import DeviceVec

    layers = tree_layers("k4", 7)
    shape = Shape(layers)
    size = shape.capacity - 5 * ES
    leaves = random_leaves(size, 3)
    arg = DeviceVec.from_host(leaves) if on_device else leaves
    rng = np.random.default_rng(5)
    sets = [[35, 32, 47, 35], [3, 200], [int(v) for v in rng.integers(0, shape.elements, 90)] + [shape.elements - 1]]
    for store_min in (0, 2, 6, 9):
        cfg = config(mm.PAD_LAST, tree_on_device)
        tree = make_tree(layers, store_min).build(arg, size=size, cfg=cfg)
        for indices in sets:
            for pruned in (False, True):
                check_against_model(tree, arg, size, indices, pruned, cfg, model_of(layers, leaves, mm.PAD_LAST))
        tree.close()
    # the mixed tree, whose layers below the first stored one have digests of both sizes
    layers = tree_layers("mixed", 6)
    shape = Shape(layers)
    leaves = random_leaves(shape.capacity, 4)
    arg = DeviceVec.from_host(leaves) if on_device else leaves
    cfg = config(tree_on_device=tree_on_device)
    tree = make_tree(layers, 3).build(arg, cfg=cfg)
    for pruned in (False, True):
        check_against_model(tree, arg, leaves.nbytes, [int(v) for v in rng.integers(0, shape.elements, 40)], pruned, cfg, model_of(layers, leaves))
    tree.close()


@pytest.mark.parametrize("shift", [1, 4, 8])
def test_leaves_off_a_16_byte_boundary(hip, shift):
    from icicle_amd._lib import lib, check
    from icicle_amd.runtime import DeviceVec

    for kind, policy in (("k4", mm.PAD_LAST), ("k1", mm.PAD_ZERO)):
        layers = tree_layers(kind, 7)
        shape = Shape(layers)
        size = shape.capacity - 12
        host = random_leaves(size + shift, shift)
        leaves = host[shift:]  # a host pointer off the boundary as well
        d = DeviceVec(size + 32)
        check(lib.icicle_copy_to_device(d.ptr + shift, leaves.ctypes.data, size))
        model = model_of(layers, leaves, policy)
        for arg in (leaves, d.ptr + shift):
            for store_min in (0, 2):
                cfg = config(policy)
                tree = make_tree(layers, store_min).build(arg, size=size, cfg=cfg)
                for pruned in (False, True):
                    check_against_model(tree, arg, size, [0, 1, 5, shape.elements - 1, shape.elements - 4, 77 % shape.elements], pruned, cfg, model)
                tree.close()


def handles(proofs):
    return (ctypes.c_void_p * len(proofs))(*[p.handle for p in proofs])


def test_refusals_leave_every_proof_empty(hip):
    import icicle_amd
    from icicle_amd._lib import lib
    from icicle_amd.merkle import MerkleProof

    layers = tree_layers("k1", 5)
    shape = Shape(layers)
    leaves = random_leaves(shape.capacity, 1)
    cfg = config()
    n = shape.elements
    tree = make_tree(layers)
    empty = fields(MerkleProof())
    for built in (False, True):
        if built:
            tree.build(leaves, cfg=cfg)
        for indices in ([0, n, 3], [0, 3, n], [0, 3, 1 << 63]) if built else ([0, 3, 5],):
            prs = [MerkleProof() for _ in indices]
            rc = lib.icicle_hip_merkle_tree_get_proofs(tree.handle, leaves.ctypes.data, leaves.nbytes, (ctypes.c_uint64 * len(indices))(*indices), len(indices), False,
                                                       ctypes.byref(cfg), handles(prs))
            assert rc == INVALID_ARGUMENT, (built, indices)
            assert all(fields(p) == empty for p in prs), (built, indices)
        with pytest.raises(icicle_amd.IcicleError) as e:
            tree.proofs(leaves, [0, n] if built else [0], cfg=cfg)
        assert e.value.code == INVALID_ARGUMENT
    bad = config(mm.PAD_NONE)
    with pytest.raises(icicle_amd.IcicleError) as e:
        tree.proofs(leaves[:-ES], [0], cfg=bad)  # short leaves without a policy, as the single call
    assert e.value.code == INVALID_ARGUMENT
    assert len(tree.proofs(leaves, [0, n - 1], cfg=cfg)) == 2
    tree.close()


def test_a_stream_of_its_own(hip):
    """a non-default stream with is_async, right behind an asynchronous build on it: the proofs are complete on return"""
    from icicle_amd.runtime import DeviceVec, Stream

    layers = tree_layers("k4", 9)
    shape = Shape(layers)
    leaves = random_leaves(shape.capacity, 8)
    d = DeviceVec.from_host(leaves)
    st = Stream()
    cfg = config()
    cfg.stream, cfg.is_async = st.handle, True
    tree = make_tree(layers).build(d, cfg=cfg)
    indices = [17, 1000, 0, 513, 17]
    for pruned in (False, True):
        got = tree.proofs(d, indices, pruned, cfg)  # no synchronisation by the caller
        for i, pr in zip(indices, got):
            leaf, path, root = mm.proof(mm.TreeShape(layers, ES), leaves.tobytes(), i, pruned)
            assert fields(pr) == (leaf, i, path, root, pruned)
    st.synchronize()
    tree.close()
    st.destroy()


# ---- verify_batch -----------------------------------------------------------------------------------------------------------------------
def flip(b: bytes, at: int) -> bytes:
    return b[:at] + bytes([b[at] ^ 0x04]) + b[at + 1:]


def corrupt(shape, pr, what):
    """one bit of proof `pr` (leaf, idx, path, root, pruned) flipped; None where the proof has no such place"""
    from icicle_amd.merkle import MerkleProof

    leaf, idx, path, root, pruned = pr
    offs = shape.group_offsets(pruned)
    steps = len(offs)
    node = idx * shape.es // shape.chunk[0]
    if what == "leaf":
        leaf = flip(leaf, len(leaf) - 1)
    elif what == "root":
        root = flip(root, 5)
    elif what == "index":
        idx ^= 1
    else:
        layer = {"lowest": 0, "middle": steps // 2, "top": steps - 1, "on_path": steps // 2}[what]
        for _ in range(layer):
            node //= 2
        o = shape.out[layer]
        if what == "on_path":
            if pruned:
                return None  # a pruned path does not carry it
            at = offs[layer] + (node % 2) * o + 7
        else:  # the sibling
            at = offs[layer] + (0 if pruned else (1 - node % 2) * o) + 9
        path = flip(path, at)
    return MerkleProof.with_data(pruned, idx, leaf, root, path)


@pytest.mark.parametrize("pruned", [False, True], ids=["full", "pruned"])
@pytest.mark.parametrize("name", sorted(OUT))
def test_verify_batch_finds_exactly_the_corrupted_proof(hip, name, pruned):
    """a 2^8 tree whose compress layers use `name`: 64 valid proofs, then one bit of one proof at a time"""
    o = OUT[name]
    layers = [("keccak256", 4), (name, 64)] + [(name, 2 * o)] * 7
    shape = Shape(layers)
    assert shape.elements == 256
    leaves = random_leaves(shape.capacity, o)
    cfg = config()
    tree = make_tree(layers).build(leaves, cfg=cfg)
    indices = [int(v) for v in np.random.default_rng(6).permutation(256)[:64]]
    good = tree.proofs(leaves, indices, pruned, cfg)
    assert tree.verify_batch(good) == [True] * 64
    plain = [fields(p) for p in good]
    for k, what in enumerate(("leaf", "lowest", "middle", "top", "on_path", "root", "index")):
        at = (9 * k + 63) % 64  # position 63 first, then others
        bad = corrupt(shape, plain[at], what)
        if bad is None:
            continue
        batch = good[:at] + [bad] + good[at + 1:]
        assert verdict(bm.TreeShape(layers, ES), bad) is False, what  # what the model says
        assert tree.verify_batch(batch) == [i != at for i in range(64)], what
    tree.close()


def test_verify_batch_wrong_sizes_and_more_than_one_block(hip):
    import icicle_amd
    from icicle_amd._lib import lib
    from icicle_amd.merkle import MerkleProof

    layers = tree_layers("k4", 7)  # 256 elements in 64 chunks of 16 bytes
    shape = Shape(layers)
    leaves = random_leaves(shape.capacity, 2)
    cfg = config()
    tree = make_tree(layers).build(leaves, cfg=cfg)
    for pruned in (False, True):
        indices = list(range(256)) + [100]  # 257 proofs
        good = tree.proofs(leaves, indices, pruned, cfg)
        assert tree.verify_batch(good) == [True] * 257
        plain = [fields(p) for p in good]
        batch = list(good)
        wrong = {0: "leaf", 255: "top", 256: "root", 131: "lowest"}
        for at, what in wrong.items():
            batch[at] = corrupt(shape, plain[at], what)
            assert verdict(bm.TreeShape(layers, ES), batch[at]) is False, what
        # a root of another length: that entry is false, and no error
        leaf, idx, path, root, _ = plain[77]
        batch[77] = MerkleProof.with_data(pruned, idx, leaf, root[:-1], path)
        # leaves of other sizes in the same batch (a 4-byte leaf, a 32-byte leaf in a tree of 16-byte chunks): whatever the model says of each
        batch[40] = MerkleProof.with_data(pruned, plain[40][1], plain[40][0][:4], plain[40][3], plain[40][2])
        batch[41] = MerkleProof.with_data(pruned, plain[41][1], plain[41][0] + b"\0" * 16, plain[41][3], plain[41][2])
        model = {at: verdict(bm.TreeShape(layers, ES), batch[at]) for at in (40, 41, 77)}
        assert model[77] is False
        want = [model.get(i, i not in wrong) for i in range(257)]
        assert tree.verify_batch(batch) == want
        # a path of the wrong length: the error, and every verdict false
        batch[200] = MerkleProof.with_data(pruned, plain[200][1], plain[200][0], plain[200][3], plain[200][2][:-1])
        ok = (ctypes.c_bool * 257)(*[True] * 257)
        assert lib.icicle_hip_merkle_tree_verify_batch(tree.handle, handles(batch), 257, ok) == INVALID_ARGUMENT
        assert list(ok) == [False] * 257
        with pytest.raises(icicle_amd.IcicleError) as e:
            tree.verify_batch(batch)
        assert e.value.code == INVALID_ARGUMENT
    # the tree need not be built: its shape and hashers are all verification uses
    fresh = make_tree(layers)
    assert fresh.verify_batch(good[:5]) == [True] * 5
    fresh.close()
    tree.close()


# ---- the single calls are batches of one ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pruned", [False, True], ids=["full", "pruned"])
@pytest.mark.parametrize("case", ["one_layer", "two_layers", "rehashed_subtree", "host_leaves_pinned_tree", "index_in_the_padding"])
def test_single_calls_are_batches_of_one(hip, case, pruned):
    """include/icicle_hip.h: get_proofs gives proofs[i] "byte for byte as icicle_merkle_tree_get_proof", verify_batch sets valid[i] to
    "what icicle_merkle_tree_verify would set" -- held at the C ABI on the smallest trees that reach each branch of the one path: an
    empty path, one group, one re-hashed sub-tree, a call that touches no device memory, and a leaf chunk made of padding alone. The
    model says what both must give."""
    from icicle_amd.merkle import MerkleProof
    from icicle_amd.runtime import DeviceVec

    # (layers, store_min, leaves on the device, tree on the device, policy, bytes of leaves or None for the capacity, indices)
    L, store_min, dev_leaves, dev_tree, policy, size, indices = {
        "one_layer": (1, 0, True, True, mm.PAD_NONE, None, [0, 3]),
        "two_layers": (2, 0, True, True, mm.PAD_NONE, None, [0, 7]),
        "rehashed_subtree": (3, 1, True, True, mm.PAD_NONE, None, [0, 9, 15]),
        "host_leaves_pinned_tree": (3, 0, False, False, mm.PAD_NONE, None, [0, 6, 15]),
        "index_in_the_padding": (3, 0, True, True, mm.PAD_LAST, 20, [4, 5, 15]),  # 20 of 64 bytes: chunk 1 half padding, chunks 2 and 3 all of it
    }[case]
    layers = tree_layers("k4", L)  # at most 4 chunks of 16 bytes
    shape = Shape(layers)
    leaves = random_leaves(size or shape.capacity, L)
    arg = DeviceVec.from_host(leaves) if dev_leaves else leaves
    cfg = config(policy, dev_tree)
    tree = make_tree(layers, store_min).build(arg, size=leaves.nbytes, cfg=cfg)
    model = bm.TreeShape(layers, ES)
    for i in indices:
        single, batch = tree.proof(arg, i, pruned, cfg, size=leaves.nbytes), tree.proofs(arg, [i], pruned, cfg, size=leaves.nbytes)[0]
        leaf, path, root = bm.proof(model, leaves.tobytes(), i, pruned, policy)
        assert fields(single) == fields(batch) == (leaf, i, path, root, pruned), i
        bad = MerkleProof.with_data(pruned, i, flip(leaf, 0), root, path)
        for pr, want in ((single, True), (bad, False)):
            assert verdict(model, pr) is want
            assert tree.verify(pr) is tree.verify_batch([pr])[0] is want, i
    tree.close()
