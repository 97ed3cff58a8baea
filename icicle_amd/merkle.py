"""Merkle trees on the device: mirror of wrappers/rust/icicle-core/src/merkle (MerkleTree, MerkleProof, MerkleTreeConfig,
PaddingPolicy) over icicle_merkle_tree_* / icicle_merkle_proof_* (include/icicle_hip.h), and this backend's batched openings and verification
(MerkleTree.proofs, MerkleTree.verify_batch)."""
import ctypes

import numpy as np

from ._lib import lib, check, IcicleError, MerkleTreeConfig
from .hash import _ptr
from .runtime import DeviceVec


class PaddingPolicy:
    NONE = 0
    ZERO_PADDING = 1
    LAST_VALUE = 2


def _bytes_at(ptr, size):
    return ctypes.string_at(ptr, size) if ptr and size else b""


class MerkleProof:
    def __init__(self, handle=None):
        self.handle = handle or lib.icicle_merkle_proof_create()
        if not self.handle:
            raise MemoryError("proof creation failed")

    @classmethod
    def with_data(cls, pruned, leaf_idx, leaf: bytes, root: bytes, path: bytes):
        return cls(lib.icicle_merkle_proof_create_with_data(pruned, leaf_idx, leaf, len(leaf), root, len(root), path, len(path)))

    @property
    def pruned(self) -> bool:
        return bool(lib.icicle_merkle_proof_is_pruned(self.handle))

    def _leaf(self):
        n, idx = ctypes.c_size_t(), ctypes.c_uint64()
        p = lib.icicle_merkle_proof_get_leaf(self.handle, ctypes.byref(n), ctypes.byref(idx))
        return _bytes_at(p, n.value), idx.value

    @property
    def leaf(self) -> bytes:
        return self._leaf()[0]

    @property
    def leaf_idx(self) -> int:
        return self._leaf()[1]

    @property
    def root(self) -> bytes:
        n = ctypes.c_size_t()
        return _bytes_at(lib.icicle_merkle_proof_get_root(self.handle, ctypes.byref(n)), n.value)

    @property
    def path(self) -> bytes:
        n = ctypes.c_size_t()
        return _bytes_at(lib.icicle_merkle_proof_get_path(self.handle, ctypes.byref(n)), n.value)

    def close(self):
        if self.handle is not None:
            check(lib.icicle_merkle_proof_delete(self.handle), "icicle_merkle_proof_delete")
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _leaves(leaves, size):
    ptr, on_device = _ptr(leaves)
    if size is None:
        size = leaves.nbytes if isinstance(leaves, (np.ndarray, DeviceVec)) else None
    if size is None:
        raise ValueError("a raw device address needs size=")
    return ptr, on_device, size


class MerkleTree:
    """layer_hashers: one Hasher per layer, leaf layer first, each created with its layer's input chunk size; the layers may mix all
    six byte hashers (Keccak / SHA3 256 and 512, Blake2s, Blake3); Poseidon2 layers (leaf elements of 4 bytes, 8 over Goldilocks, digests of one
    element) build, open and verify the same way, and so do Poseidon layers over the 256-bit scalar fields (leaf elements and
    digests of 32 bytes, arity t, or t - 1 beside a domain tag)"""

    def __init__(self, layer_hashers, leaf_element_size, output_store_min_layer=0):
        arr = (ctypes.c_void_p * len(layer_hashers))(*[h.handle for h in layer_hashers])
        self.handle = lib.icicle_merkle_tree_create(arr, len(layer_hashers), leaf_element_size, output_store_min_layer)
        if not self.handle:
            raise IcicleError(11, "icicle_merkle_tree_create: the layers do not form a tree")

    def build(self, leaves, size=None, cfg=None):
        cfg = cfg or MerkleTreeConfig.default()
        ptr, cfg.is_leaves_on_device, size = _leaves(leaves, size)
        check(lib.icicle_merkle_tree_build(self.handle, ptr, size, ctypes.byref(cfg)), "icicle_merkle_tree_build")
        return self

    def root(self):
        """the root's bytes, None before build; after an asynchronous build synchronise the stream first"""
        n = ctypes.c_size_t()
        p = lib.icicle_merkle_tree_get_root(self.handle, ctypes.byref(n))
        return _bytes_at(p, n.value) if p else None

    def proof(self, leaves, leaf_idx, pruned=False, cfg=None, size=None) -> MerkleProof:
        cfg = cfg or MerkleTreeConfig.default()
        ptr, cfg.is_leaves_on_device, size = _leaves(leaves, size)
        pr = MerkleProof()
        check(lib.icicle_merkle_tree_get_proof(self.handle, ptr, size, leaf_idx, pruned, ctypes.byref(cfg), pr.handle), "icicle_merkle_tree_get_proof")
        return pr

    def verify(self, proof: MerkleProof) -> bool:
        ok = ctypes.c_bool(False)
        check(lib.icicle_merkle_tree_verify(self.handle, proof.handle, ctypes.byref(ok)), "icicle_merkle_tree_verify")
        return bool(ok.value)

    def proofs(self, leaves, leaf_indices, pruned=False, cfg=None, size=None) -> list:
        """one MerkleProof per index, each as proof() returns it, from one call (icicle_hip_merkle_tree_get_proofs): the indices
        may repeat and come in any order"""
        cfg = cfg or MerkleTreeConfig.default()
        ptr, cfg.is_leaves_on_device, size = _leaves(leaves, size)
        idx = [int(i) for i in leaf_indices]
        out = [MerkleProof() for _ in idx]
        check(lib.icicle_hip_merkle_tree_get_proofs(self.handle, ptr, size, (ctypes.c_uint64 * len(idx))(*idx), len(idx), pruned, ctypes.byref(cfg),
                                                    (ctypes.c_void_p * len(idx))(*[p.handle for p in out])), "icicle_hip_merkle_tree_get_proofs")
        return out

    def verify_batch(self, proofs) -> list:
        """verify() of every proof, from one call (icicle_hip_merkle_tree_verify_batch); all pruned or all full"""
        proofs = list(proofs)
        ok = (ctypes.c_bool * len(proofs))()
        check(lib.icicle_hip_merkle_tree_verify_batch(self.handle, (ctypes.c_void_p * len(proofs))(*[p.handle for p in proofs]), len(proofs), ok),
              "icicle_hip_merkle_tree_verify_batch")
        return [bool(v) for v in ok]

    def close(self):
        if self.handle is not None:
            check(lib.icicle_merkle_tree_delete(self.handle), "icicle_merkle_tree_delete")
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
