"""FRI on the device: mirror of wrappers/rust/icicle-core/src/fri (FriConfig, FriTranscriptConfig with new_default_labels, FriProof,
fri_merkle_tree_prove, fri_merkle_tree_verify) over <field>[_extension]_fri_* / <field>[_extension]_icicle_*_fri_proof
(include/icicle_hip.h). Elements are canonical uint32 words. BabyBear and KoalaBear, scalar and quartic extension: arrays of shape [n]
(scalar) or [n, 4] (extension, constant coefficient first). The wider fields: [n, 2] for goldilocks, [n, 4] for its quadratic
extension (a0 + a1 u, u^2 = 7, two words per coefficient, constant term first; extension=True is valid for goldilocks only among
them), [n, 8] for stark252, bn254, bls12_381 and bls12_377. The NTT domain of the field must be initialised for the input size
(icicle_amd.ntt.init_domain)."""
import ctypes

import numpy as np

from ._lib import lib, check, FriConfig, FFIFriTranscriptConfig, NTT_FIELDS, FRI_WIDE_WORDS
from .hash import _ptr
from .merkle import MerkleProof
from .runtime import DeviceVec

__all__ = ["FriConfig", "FriTranscriptConfig", "FriProof", "fri_merkle_tree_prove", "fri_merkle_tree_verify", "fri_fold"]


def _prefix(field, extension):
    p = f"{field}_extension" if extension else field
    assert field in NTT_FIELDS or p in FRI_WIDE_WORDS, p
    return p


def _words(field, extension):
    """uint32 words of one element"""
    if field is None or field in NTT_FIELDS:
        return 4 if extension else 1
    return FRI_WIDE_WORDS[_prefix(field, extension)]


def _fn(field, extension, name):
    return getattr(lib, f"{_prefix(field, extension)}_{name}")


class FriTranscriptConfig:
    """Labels, public state and seed of the Fiat-Shamir transcript. `seed_rng`: one element of F, an int (scalar; the constant
    coefficient of an extension element) or a sequence of words. seed_words and _ffi take the field where an element is wider than
    BabyBear's and KoalaBear's (field=None: those two)."""

    def __init__(self, hasher, domain_separator_label, round_challenge_label, commit_phase_label, nonce_label, public_state, seed_rng):
        self.hasher = hasher
        as_bytes = lambda s: s.encode() if isinstance(s, str) else bytes(s)
        self.domain_separator_label = as_bytes(domain_separator_label)
        self.round_challenge_label = as_bytes(round_challenge_label)
        self.commit_phase_label = as_bytes(commit_phase_label)
        self.nonce_label = as_bytes(nonce_label)
        self.public_state = as_bytes(public_state)
        self.seed_rng = seed_rng

    @classmethod
    def new_default_labels(cls, hasher, seed_rng):
        return cls(hasher, "domain_separator_label", "round_challenge_label", "commit_phase_label", "nonce_label", b"", seed_rng)

    def seed_words(self, extension, field=None):
        words = _words(field, extension)
        if isinstance(self.seed_rng, (int, np.integer)):
            coeff = words // _words(field, False) if extension else 1  # coefficients of an element: 4, 2 (goldilocks) or 1
            s = [(int(self.seed_rng) >> (32 * i)) & 0xFFFFFFFF for i in range(words // coeff)]  # the constant coefficient, little-endian words
        else:
            s = [int(v) for v in np.asarray(self.seed_rng).reshape(-1)]
        assert len(s) <= words, "seed_rng has more words than an element"
        return s + [0] * (words - len(s))

    def _ffi(self, extension, field=None):
        """(struct, objects that must outlive the call)"""
        keep = [ctypes.create_string_buffer(b, max(len(b), 1)) for b in (self.domain_separator_label, self.round_challenge_label, self.commit_phase_label,
                                                                        self.nonce_label, self.public_state)]
        seed = (ctypes.c_uint32 * _words(field, extension))(*self.seed_words(extension, field))
        lens = [len(self.domain_separator_label), len(self.round_challenge_label), len(self.commit_phase_label), len(self.nonce_label), len(self.public_state)]
        args = [self.hasher.handle]
        for buf, n in zip(keep, lens):
            args += [ctypes.cast(buf, ctypes.c_void_p), n]
        return FFIFriTranscriptConfig(*args, ctypes.cast(seed, ctypes.c_void_p)), keep + [seed]


class FriProof:
    """Owns a proof handle. `slots[q][r]` of a proof are read through MerkleProof views that borrow from it."""

    def __init__(self, field, extension=False, handle=None):
        self.field, self.extension = field, extension
        self.handle = handle or _fn(field, extension, "icicle_initialize_fri_proof")()
        if not self.handle:
            raise MemoryError("FRI proof creation failed")

    @classmethod
    def create_with_arguments(cls, field, query_proofs, final_poly, pow_nonce, extension=False):
        """query_proofs[q][r]: MerkleProof objects, q over the 2 * nof_queries slots; final_poly: uint32 array [size] or [size, words]"""
        nq, nr = len(query_proofs), len(query_proofs[0]) if query_proofs else 0
        rows = [(ctypes.c_void_p * nr)(*[p.handle for p in row]) for row in query_proofs]
        table = (ctypes.c_void_p * nq)(*[ctypes.cast(r, ctypes.c_void_p) for r in rows])
        fp = np.ascontiguousarray(final_poly, dtype=np.uint32)
        size = fp.size // _words(field, extension)
        h = _fn(field, extension, "icicle_create_with_arguments_fri_proof")(table, nq, nr, fp.ctypes.data, size, pow_nonce)
        if not h:
            raise MemoryError("FRI proof creation failed")
        return cls(field, extension, h)

    def _size(self, name):
        v = ctypes.c_size_t()
        check(_fn(self.field, self.extension, name)(self.handle, ctypes.byref(v)), name)
        return int(v.value)

    @property
    def nof_queries(self) -> int:
        """the number of slots: two per query (the query and its symmetric position), as the reference counts"""
        return self._size("fri_proof_get_nof_queries")

    @property
    def nof_rounds(self) -> int:
        return self._size("fri_proof_get_nof_rounds")

    @property
    def final_poly_size(self) -> int:
        return self._size("fri_proof_get_final_poly_size")

    @property
    def final_poly(self) -> np.ndarray:
        p = ctypes.c_void_p()
        check(_fn(self.field, self.extension, "fri_proof_get_final_poly")(self.handle, ctypes.byref(p)), "fri_proof_get_final_poly")
        n, w = self.final_poly_size, _words(self.field, self.extension)
        if not n:
            return np.zeros((0, w) if w > 1 else 0, dtype=np.uint32)
        a = np.frombuffer(ctypes.string_at(p.value, 4 * n * w), dtype=np.uint32).copy()
        return a.reshape(n, w) if w > 1 else a

    @property
    def pow_nonce(self) -> int:
        v = ctypes.c_uint64()
        check(_fn(self.field, self.extension, "fri_proof_get_pow_nonce")(self.handle, ctypes.byref(v)), "fri_proof_get_pow_nonce")
        return int(v.value)

    def round_proofs_for_query(self, query_idx):
        """the slot's MerkleProofs, one per round; views borrowed from this proof (they keep it alive)"""
        arr = (ctypes.c_void_p * max(self.nof_rounds, 1))()
        check(_fn(self.field, self.extension, "fri_proof_get_round_proofs_for_query")(self.handle, query_idx, arr), "fri_proof_get_round_proofs_for_query")
        return [_BorrowedMerkleProof(arr[r], self) for r in range(self.nof_rounds)]

    def slots(self):
        return [self.round_proofs_for_query(q) for q in range(self.nof_queries)]

    def close(self):
        if self.handle is not None:
            check(_fn(self.field, self.extension, "icicle_delete_fri_proof")(self.handle), "icicle_delete_fri_proof")
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _BorrowedMerkleProof(MerkleProof):
    def __init__(self, handle, owner):
        self.handle, self._owner = handle, owner

    def close(self):  # the FRI proof deletes it
        self.handle = None


def _copy(cfg):
    return type(cfg).from_buffer_copy(cfg)


def _elements(data, field, extension):
    ptr, on_device = _ptr(data)
    return ptr, on_device, data.nbytes // (4 * _words(field, extension))


def fri_merkle_tree_prove(field, cfg, tcfg, data, leaves_hash, compress_hash, min_layer=0, extension=False, proof=None, size=None) -> FriProof:
    """The FRI proof of `data` (NumPy uint32 array on the host or DeviceVec; a raw device address with size= elements). leaves_hash:
    Hasher with chunk = one element (4 or 16 bytes; 8, 16 or 32 for the wider fields); compress_hash: arity 2 (chunk = 2 * its
    digest). Returns with cfg.stream drained."""
    cfg = _copy(cfg) if cfg is not None else FriConfig.default()  # are_inputs_on_device follows `data`; the caller's config stays as it is
    if isinstance(data, int):
        assert size is not None, "a raw device address needs size="
        ptr, cfg.are_inputs_on_device = data, True
    else:
        ptr, cfg.are_inputs_on_device, n = _elements(data, field, extension)
        size = n if size is None else size
    ffi, keep = tcfg._ffi(extension, field)
    proof = proof or FriProof(field, extension)
    check(_fn(field, extension, "fri_merkle_tree_prove")(ctypes.byref(cfg), ctypes.byref(ffi), ptr, size, leaves_hash.handle, compress_hash.handle, min_layer,
                                                        proof.handle), "fri_merkle_tree_prove")
    del keep
    return proof


def fri_merkle_tree_verify(field, cfg, tcfg, proof, leaves_hash, compress_hash, extension=False) -> bool:
    cfg = cfg or FriConfig.default()
    ffi, keep = tcfg._ffi(extension, field)
    ok = ctypes.c_bool(False)
    check(_fn(field, extension, "fri_merkle_tree_verify")(ctypes.byref(cfg), ctypes.byref(ffi), proof.handle, leaves_hash.handle, compress_hash.handle,
                                                         ctypes.byref(ok)), "fri_merkle_tree_verify")
    del keep
    return bool(ok.value)


def fri_fold(field, data, alpha, extension=False, out=None, stream=None):
    """One fold (backend-specific helper): n elements -> n / 2 with the challenge `alpha`. Host arrays in, host array out; with a
    DeviceVec `data`, `alpha` is a DeviceVec too and the result a DeviceVec (`out`, or a new one)."""
    ptr, on_device, n = _elements(data, field, extension)
    w = _words(field, extension)
    if on_device:
        if not isinstance(alpha, (DeviceVec, int)):
            raise TypeError("fri_fold: device data needs alpha on the device (DeviceVec)")
        if out is None:
            out = DeviceVec(data.nbytes // 2)
        elif not isinstance(out, (DeviceVec, int)):
            raise TypeError("fri_fold: device data needs out on the device (DeviceVec)")
        ap, op = _ptr(alpha)[0], _ptr(out)[0]
    else:
        alpha = np.ascontiguousarray(alpha, dtype=np.uint32).reshape(-1)
        if out is None:
            out = np.zeros((n // 2, w) if w > 1 else n // 2, dtype=np.uint32)
        ap, op = alpha.ctypes.data, out.ctypes.data
    check(_fn(field, extension, "hip_fri_fold")(ptr, n, ap, op, on_device, stream), "hip_fri_fold")
    return out
