"""Keccak / SHA3 / Blake2s / Blake3 / Poseidon2 / Poseidon batch hashing on the device: mirror of wrappers/rust/icicle-core/src/hash
(Hasher, HashConfig) over icicle_create_keccak_256 .. icicle_create_blake3, <field>_create_poseidon2_hasher,
<field>_create_poseidon_hasher / icicle_hasher_hash (include/icicle_hip.h)."""
import ctypes

import numpy as np

from ._lib import lib, check, HashConfig, POSEIDON2_FIELDS, POSEIDON2_WIDE_FIELDS, POSEIDON2_GOLD_FIELDS, POSEIDON_FIELDS
from .runtime import DeviceVec


def _ptr(x):
    """(address, on device): NumPy uint8 / uint32 / uint64 arrays are host memory, DeviceVec and raw addresses device memory"""
    if isinstance(x, DeviceVec):
        return x.ptr, True
    if isinstance(x, int):
        return x, True
    assert isinstance(x, np.ndarray) and x.dtype in (np.uint8, np.uint32, np.uint64) and x.flags["C_CONTIGUOUS"]
    return x.ctypes.data, False


def _tag_words(domain_tag):
    """a domain tag over a 256-bit field, an int or 8 words, as the 8 words the factories take; None stays None"""
    if domain_tag is None:
        return None
    if isinstance(domain_tag, (int, np.integer)):
        if not 0 <= int(domain_tag) < 1 << 256:
            raise ValueError("a domain tag is one field element")
        words = [int(domain_tag) >> (32 * i) & 0xFFFFFFFF for i in range(8)]
    else:
        words = [int(w) for w in np.asarray(domain_tag, dtype=np.uint32).reshape(8)]
    return (ctypes.c_uint32 * 8)(*words)


class Hasher:
    """One of the four Keccak-f[1600] sponges, Blake2s-256, Blake3, Poseidon2 over a 31-bit field, Goldilocks or a 256-bit scalar
    field, or Poseidon over a 256-bit scalar field; `chunk` is the default message size in bytes (a Merkle layer's input size)."""

    def __init__(self, handle, chunk):
        if not handle:
            raise MemoryError("hasher creation failed")
        self.handle = handle
        self.chunk = chunk

    @classmethod
    def keccak256(cls, chunk=0):
        return cls(lib.icicle_create_keccak_256(chunk), chunk)

    @classmethod
    def keccak512(cls, chunk=0):
        return cls(lib.icicle_create_keccak_512(chunk), chunk)

    @classmethod
    def sha3_256(cls, chunk=0):
        return cls(lib.icicle_create_sha3_256(chunk), chunk)

    @classmethod
    def sha3_512(cls, chunk=0):
        return cls(lib.icicle_create_sha3_512(chunk), chunk)

    @classmethod
    def blake2s(cls, chunk=0):
        return cls(lib.icicle_create_blake2s(chunk), chunk)

    @classmethod
    def blake3(cls, chunk=0):
        return cls(lib.icicle_create_blake3(chunk), chunk)

    @classmethod
    def poseidon2(cls, field, t, domain_tag=None, input_size=0):
        """Poseidon2 of width t (2, 3, 4, 8, 12, 16, 20, 24) over "babybear" or "koalabear": messages and digests are uint32 canonical
        residues, the digest one element. `input_size` is in elements, 0 = t (t - 1 beside a `domain_tag`, which is one element).
        Of width t (2, 3, 4, 8) over the scalar field of "bn254", "bls12_381", "bls12_377" or "grumpkin" or over "stark252": elements
        are canonical residues of 8 little-endian uint32 words, the `domain_tag` an int or an array of 8 words.
        "goldilocks" is refused here: its elements are a third size, and its call is `Hasher.poseidon2_goldilocks`."""
        if field in POSEIDON2_WIDE_FIELDS:
            es, tag = 32, _tag_words(domain_tag)
        elif field in POSEIDON2_FIELDS:
            es, tag = 4, None if domain_tag is None else ctypes.byref(ctypes.c_uint32(int(domain_tag)))
        else:
            hint = "; Goldilocks has Hasher.poseidon2_goldilocks" if field in POSEIDON2_GOLD_FIELDS else ""
            raise ValueError(f"Poseidon2 is built over {POSEIDON2_FIELDS + POSEIDON2_WIDE_FIELDS}, not {field!r}{hint}")
        handle = getattr(lib, f"{field}_create_poseidon2_hasher")(t, tag, input_size)
        if not handle:
            raise ValueError(f"Poseidon2 over {field} has no width {t}" + (" with this tag" if es == 32 and domain_tag is not None else ""))
        return cls(handle, es * (input_size or (t if domain_tag is None else t - 1)))

    @classmethod
    def poseidon2_goldilocks(cls, t, domain_tag=None, input_size=0):
        """Poseidon2 of width t (2, 3, 4, 8, 12, 16, 20, 24) over Goldilocks, p = 2^64 - 2^32 + 1: messages and digests are uint64
        canonical residues (or pairs of little-endian uint32 words), the digest one element of 8 bytes. `input_size` is in elements,
        0 = t (t - 1 beside a `domain_tag`, which is one element: an int below p). A call of its own, not a field name of
        `Hasher.poseidon2`: that one keeps refusing "goldilocks", as it did before this hash existed."""
        tag = None
        if domain_tag is not None:
            if not 0 <= int(domain_tag) < 1 << 64:
                raise ValueError("a domain tag is one field element")
            tag = (ctypes.c_uint32 * 2)(int(domain_tag) & 0xFFFFFFFF, int(domain_tag) >> 32)
        handle = lib.goldilocks_create_poseidon2_hasher(t, tag, input_size)
        if not handle:
            raise ValueError(f"Poseidon2 over goldilocks has no width {t}" + (" with this tag" if domain_tag is not None else ""))
        return cls(handle, 8 * (input_size or (t if domain_tag is None else t - 1)))

    @classmethod
    def poseidon(cls, field, t, domain_tag=None, input_size=0):
        """Poseidon of width t (3, 5, 9, 12) over the scalar field of "bn254", "bls12_381" (not t = 3), "bls12_377" or "grumpkin":
        messages and digests are canonical residues of 8 little-endian uint32 words, the digest one element. A message is exactly
        the arity: t elements, or t - 1 beside a `domain_tag` (an int, or an array of 8 words); `input_size` is 0 or the arity."""
        if field not in POSEIDON_FIELDS:
            raise ValueError(f"Poseidon is built over {POSEIDON_FIELDS}, not {field!r}")
        tag = _tag_words(domain_tag)
        handle = getattr(lib, f"{field}_create_poseidon_hasher")(t, tag, input_size)
        if not handle:
            raise ValueError(f"Poseidon over {field} has no width {t} with this tag and input size")
        return cls(handle, 32 * (t if domain_tag is None else t - 1))

    @property
    def output_size(self) -> int:
        return int(lib.icicle_hasher_output_size(self.handle))

    def hash(self, inp, size=None, batch=1, out=None, cfg=None):
        """`batch` messages of `size` bytes back to back in `inp` -> digests back to back. size=None: the whole host array is
        `batch` equal messages; a device operand needs `size` (or the hasher's default chunk, size=0)."""
        cfg = cfg or HashConfig.default()
        ip, cfg.are_inputs_on_device = _ptr(inp)
        if size is None:
            size = inp.nbytes // batch if isinstance(inp, np.ndarray) else 0
        cfg.batch = batch
        if out is None:
            out = np.zeros(batch * self.output_size, dtype=np.uint8)
        op, cfg.are_outputs_on_device = _ptr(out)
        check(lib.icicle_hasher_hash(self.handle, ip, size, ctypes.byref(cfg), op), "icicle_hasher_hash")
        return out

    def close(self):
        if self.handle is not None:
            check(lib.icicle_hasher_delete(self.handle), "icicle_hasher_delete")
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
