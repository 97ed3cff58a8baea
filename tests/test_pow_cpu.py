"""CPU: the proof-of-work part of the C ABI without a GPU -- the two symbols in header, library and binding, the PowConfig layout,
every argument error (returned before the device is touched), loud failure of the compute paths, and the device's message reader
(ReadPow of icicle_amd/csrc/hash_readers.hpp under the Blake absorb code of blake.hpp, compiled with g++: tests/pow_host_harness.cpp)
against hashlib and the Blake3 model on messages built here."""
import ctypes
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

from tests import blake_model as bm

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

INVALID_POINTER, INVALID_ARGUMENT = 3, 11
SIZES = [0, 1, 7, 8, 21, 31, 32, 33, 56, 60, 64, 120]
PADDINGS = [0, 3, 7, 24]
NONCES = [0, 1, 2**32 - 1, 2**32, 2**64 - 1]


def message(challenge: bytes, nonce: int, padding: int) -> bytes:
    return challenge + nonce.to_bytes(8, "little") + bytes(padding)


# ---- header, library, binding ------------------------------------------------------------------------------------------------------
def test_pow_functions_are_declared_exported_and_bound():
    from icicle_amd import _lib
    import icicle_amd

    text = subprocess.check_output(["gcc", "-E", "-P", os.path.join(ROOT, "include", "icicle_hip.h")], text=True)
    text = re.sub(r"\s+", " ", text)
    head = r"icicle_error_t %s\s*\(\s*icicle_hasher_handle_t \w+, const uint8_t\s*\* \w+, uint32_t \w+, uint8_t \w+, const icicle_pow_config_t\s*\* \w+, "
    assert re.search(head % "proof_of_work" + r"_Bool\s*\* \w+, uint64_t\s*\* \w+, uint64_t\s*\* \w+\s*\)\s*;", text)
    assert re.search(head % "proof_of_work_verify" + r"uint64_t \w+, _Bool\s*\* \w+, uint64_t\s*\* \w+\s*\)\s*;", text)
    for name, nargs in (("proof_of_work", 8), ("proof_of_work_verify", 8)):
        fn = getattr(_lib.lib, name)  # exported
        assert name in _lib.API_SYMBOLS and len(fn.argtypes) == nargs
    assert _lib.lib.proof_of_work_verify.argtypes[5] is ctypes.c_uint64  # the nonce by value
    assert callable(icicle_amd.pow_solve) and callable(icicle_amd.pow_verify)
    assert icicle_amd.PowConfig is _lib.PowConfig


def test_pow_config_layout():
    from icicle_amd import _lib

    P = _lib.PowConfig
    assert ctypes.sizeof(P) == 32
    assert [(f, getattr(P, f).offset) for f, _ in P._fields_] == [("stream", 0), ("is_challenge_on_device", 8), ("padding_size", 12), ("is_async", 16), ("ext", 24)]
    d = P.default()
    assert (d.stream, d.is_challenge_on_device, d.padding_size, d.is_async, d.ext) == (None, False, 24, False, None)
    # the header's struct, as the C compiler lays it out
    prog = ('#include <stddef.h>\n#include <stdio.h>\n#include "icicle_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu", sizeof(icicle_pow_config_t), '
            + ", ".join(f"offsetof(icicle_pow_config_t, {f})" for f, _ in P._fields_) + "); return 0; }\n")
    build = os.path.join(HERE, "_build")
    os.makedirs(build, exist_ok=True)
    src, exe = os.path.join(build, "pow_layout.c"), os.path.join(build, "pow_layout")
    with open(src, "w") as f:
        f.write(prog)
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
    assert subprocess.check_output([exe], text=True).split() == ["32", "0", "8", "12", "16", "24"]


# ---- argument errors, with or without a device ---------------------------------------------------------------------------------------
def raw_solve(handle, challenge, size, bits, cfg, outs=(True, True, True)):
    from icicle_amd._lib import lib

    found, nonce, mined = ctypes.c_bool(False), ctypes.c_uint64(77), ctypes.c_uint64(78)
    ptrs = [ctypes.byref(v) if keep else None for v, keep in zip((found, nonce, mined), outs)]
    rc = lib.proof_of_work(handle, challenge, size, bits, ctypes.byref(cfg) if cfg is not None else None, *ptrs)
    assert (nonce.value, mined.value) == (77, 78) or rc == 0
    return rc


def raw_verify(handle, challenge, size, bits, cfg, nonce=5, outs=(True, True)):
    from icicle_amd._lib import lib

    ok, mined = ctypes.c_bool(False), ctypes.c_uint64(78)
    ptrs = [ctypes.byref(v) if keep else None for v, keep in zip((ok, mined), outs)]
    return lib.proof_of_work_verify(handle, challenge, size, bits, ctypes.byref(cfg) if cfg is not None else None, nonce, *ptrs)


def test_argument_errors_need_no_gpu():
    from icicle_amd import PowConfig
    from icicle_amd._lib import lib
    from icicle_amd.hash import Hasher

    ch = np.arange(32, dtype=np.uint8)
    p = ch.ctypes.data
    for make in (Hasher.keccak256, Hasher.keccak512, Hasher.sha3_256, Hasher.sha3_512, Hasher.blake2s, Hasher.blake3):
        h = make()
        for bits in (0, 61, 64, 255):
            assert raw_solve(h.handle, p, 32, bits, PowConfig.default()) == INVALID_ARGUMENT, bits
            assert raw_verify(h.handle, p, 32, bits, PowConfig.default()) == INVALID_ARGUMENT, bits
        assert raw_solve(None, p, 32, 8, PowConfig.default()) == INVALID_POINTER
        assert raw_verify(None, p, 32, 8, PowConfig.default()) == INVALID_POINTER
        assert raw_solve(h.handle, p, 32, 8, None) == INVALID_POINTER
        assert raw_verify(h.handle, p, 32, 8, None) == INVALID_POINTER
        assert raw_solve(h.handle, None, 32, 8, PowConfig.default()) == INVALID_POINTER
        assert raw_verify(h.handle, None, 32, 8, PowConfig.default()) == INVALID_POINTER
        for k in range(3):
            assert raw_solve(h.handle, p, 32, 8, PowConfig.default(), outs=[j != k for j in range(3)]) == INVALID_POINTER, k
        for k in range(2):
            assert raw_verify(h.handle, p, 32, 8, PowConfig.default(), outs=[j != k for j in range(2)]) == INVALID_POINTER, k
        # extension keys out of range
        for key, bad in ((b"hip_pow_span_log2", -1), (b"hip_pow_span_log2", 33), (b"hip_pow_count_log2", -1), (b"hip_pow_count_log2", 65)):
            ext = lib.create_config_extension()
            lib.config_extension_set_int(ext, key, bad)
            cfg = PowConfig.default()
            cfg.ext = ext
            assert raw_solve(h.handle, p, 32, 8, cfg) == INVALID_ARGUMENT, (key, bad)
            lib.destroy_config_extension(ext)
        h.close()


def test_blake3_beyond_one_chunk_is_refused_without_a_gpu():
    from icicle_amd import PowConfig
    from icicle_amd.hash import Hasher

    h = Hasher.blake3()
    big = np.zeros(1017, dtype=np.uint8)
    for size, padding in ((1017, 0), (993, 24), (32, 985), (0, 1017)):  # challenge + 8 + padding == 1025
        cfg = PowConfig.default()
        cfg.padding_size = padding
        assert raw_solve(h.handle, big.ctypes.data, size, 8, cfg) == INVALID_ARGUMENT, (size, padding)
        assert raw_verify(h.handle, big.ctypes.data, size, 8, cfg) == INVALID_ARGUMENT, (size, padding)
    h.close()


def test_no_gpu_means_loud_failure():
    import icicle_amd
    from icicle_amd import PowConfig, runtime
    from icicle_amd.hash import Hasher

    if runtime.get_device_count() > 0:
        return  # with a device these calls succeed (tests/test_gpu_pow.py)
    ch = np.arange(32, dtype=np.uint8)
    for make in (Hasher.keccak256, Hasher.sha3_512, Hasher.blake2s, Hasher.blake3):
        h = make()
        with pytest.raises(icicle_amd.IcicleError):
            icicle_amd.pow_solve(h, ch, 4)
        with pytest.raises(icicle_amd.IcicleError):
            icicle_amd.pow_verify(h, ch, 4, 12)
        cfg = PowConfig.default()
        cfg.padding_size = 984  # 32 + 8 + 984 = 1024: Blake3 at exactly one chunk is an accepted argument: the failure is the missing device
        with pytest.raises(icicle_amd.IcicleError) as e:
            icicle_amd.pow_solve(h, ch, 4, cfg)
        assert e.value.code != INVALID_ARGUMENT
        h.close()


# ---- ReadPow on the host --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness():
    so = os.path.join(HERE, "_build", "libpow_host.so")
    os.makedirs(os.path.dirname(so), exist_ok=True)
    src = os.path.join(HERE, "pow_host_harness.cpp")
    hdrs = [os.path.join(ROOT, "icicle_amd", "csrc", h) for h in ("blake.hpp", "hash_readers.hpp")]
    if not os.path.exists(so) or max(os.path.getmtime(f) for f in [src] + hdrs) > os.path.getmtime(so):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", src, "-o", so])
    lib = ctypes.CDLL(so)
    lib.ph_hash.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p]
    lib.ph_message.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p]
    return lib


def challenge_of(size):
    return np.array([(37 * i + 11 + size) & 0xFF for i in range(size)], dtype=np.uint8)


def test_reader_serves_the_message_through_every_accessor(harness):
    """byte(), word() from every offset mod 8 (a word that mixes challenge tail and nonce, nonce and padding) and pair()"""
    for size in SIZES:
        ch = challenge_of(size)
        for padding in PADDINGS:
            for nonce in NONCES + [0x0123456789ABCDEF]:
                want = message(ch.tobytes(), nonce, padding)
                out = np.zeros(len(want), dtype=np.uint8)
                for how, shifts in ((0, [0]), (1, range(8)), (2, range(8))):
                    for shift in shifts:
                        out[:] = 0xAA
                        assert harness.ph_message(ch.ctypes.data, size, nonce, len(want), how, shift, out.ctypes.data) == 0
                        assert out.tobytes() == want, (size, padding, hex(nonce), how, shift)


def test_blake2s_over_the_reader_matches_hashlib(harness):
    out = np.zeros(32, dtype=np.uint8)
    for size in SIZES:
        ch = challenge_of(size)
        for padding in PADDINGS:
            for nonce in NONCES:
                msg = message(ch.tobytes(), nonce, padding)
                assert harness.ph_hash(1, ch.ctypes.data, size, nonce, len(msg), out.ctypes.data) == 0
                assert out.tobytes() == hashlib.blake2s(msg).digest(), (size, padding, hex(nonce))


def test_blake3_over_the_reader_matches_the_model(harness):
    out = np.zeros(32, dtype=np.uint8)
    for size in SIZES:
        ch = challenge_of(size)
        for padding in PADDINGS:
            for nonce in NONCES:
                msg = message(ch.tobytes(), nonce, padding)
                assert harness.ph_hash(2, ch.ctypes.data, size, nonce, len(msg), out.ctypes.data) == 0
                assert out.tobytes() == bm.digest("blake3", msg), (size, padding, hex(nonce))


def test_the_known_answer_of_the_reference_on_the_host(harness):
    """wrappers/rust/icicle-hash/src/tests.rs (blake3_pow): challenge [20] * 32, 25 bits -> nonce 40825909, hash 364385878471"""
    ch = np.full(32, 20, dtype=np.uint8)
    out = np.zeros(32, dtype=np.uint8)
    assert harness.ph_hash(2, ch.ctypes.data, 32, 40825909, 64, out.ctypes.data) == 0
    got = int.from_bytes(out.tobytes()[:8], "little")
    assert got == 364385878471 and got < 1 << (64 - 25)
    assert out.tobytes() == bm.digest("blake3", message(ch.tobytes(), 40825909, 24))
