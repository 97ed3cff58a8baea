"""Proof of work on the device: mirror of wrappers/rust/icicle-hash/src/pow.rs (pow_solver, pow_verify) over proof_of_work /
proof_of_work_verify (include/icicle_hip.h). The message of nonce n is challenge | n as 8 little-endian bytes | cfg.padding_size zero
bytes; n solves when the first 8 digest bytes, read as a little-endian word, are below 2^(64 - bits)."""
import ctypes

from ._lib import lib, check, PowConfig
from .hash import _ptr


def _challenge(challenge, size):
    ptr, on_device = _ptr(challenge)
    if size is None:
        assert not isinstance(challenge, int), "a raw device address needs size="
        size = challenge.nbytes
    return (ptr if size else None), size, on_device


def pow_solve(hasher, challenge, bits, cfg=None, size=None):
    """(found, nonce, mined_hash): the smallest solving nonce and its candidate; (False, None, None) when the nonces searched hold none.
    `challenge`: a NumPy uint8 array (host), a DeviceVec or a raw device address (then with size=). Returns with cfg.stream drained."""
    cfg = cfg or PowConfig.default()
    ptr, size, cfg.is_challenge_on_device = _challenge(challenge, size)
    found, nonce, mined = ctypes.c_bool(False), ctypes.c_uint64(0), ctypes.c_uint64(0)
    check(lib.proof_of_work(hasher.handle, ptr, size, bits, ctypes.byref(cfg), ctypes.byref(found), ctypes.byref(nonce), ctypes.byref(mined)), "proof_of_work")
    return (True, int(nonce.value), int(mined.value)) if found.value else (False, None, None)


def pow_verify(hasher, challenge, bits, nonce, cfg=None, size=None):
    """(ok, mined_hash): the candidate of `nonce` and whether it is below the threshold"""
    cfg = cfg or PowConfig.default()
    ptr, size, cfg.is_challenge_on_device = _challenge(challenge, size)
    ok, mined = ctypes.c_bool(False), ctypes.c_uint64(0)
    check(lib.proof_of_work_verify(hasher.handle, ptr, size, bits, ctypes.byref(cfg), nonce, ctypes.byref(ok), ctypes.byref(mined)), "proof_of_work_verify")
    return bool(ok.value), int(mined.value)
