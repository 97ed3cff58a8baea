"""GPU: the proof-of-work solver and verifier (proof_of_work, proof_of_work_verify) for all six hashers -- the known answer recorded in
the reference's Rust test, the smallest solving nonce against hashlib (SHA3, Blake2s) and the models (Keccak, Blake3: tests/merkle_model.py,
tests/blake_model.py), the same searches cut into spans of 2^8 and 2^12 nonces with solutions on a span's first and last nonce, an
independent minimality check through the batch kernels, message sizes around every block edge with the nonce across one, a search
that starts below 2^32 and ends above it, a bounded count, and device / unaligned / stream operands."""
import ctypes
import functools
import hashlib

import numpy as np
import pytest

from tests import blake_model as bm

pytestmark = pytest.mark.gpu

NAMES = ["keccak256", "keccak512", "sha3_256", "sha3_512", "blake2s", "blake3"]
HASHLIB = {"sha3_256": hashlib.sha3_256, "sha3_512": hashlib.sha3_512, "blake2s": hashlib.blake2s}
CHALLENGE = bytes(range(32))
BLOCK = 4096  # nonces per cached block of reference candidates


def make(name):
    from icicle_amd.hash import Hasher

    return getattr(Hasher, name)()


def messages(challenge: bytes, padding: int, lo: int, n: int) -> np.ndarray:
    """uint8 [n, challenge + 8 + padding]: the messages of nonces lo .. lo + n - 1"""
    cs = len(challenge)
    m = np.zeros((n, cs + 8 + padding), dtype=np.uint8)
    m[:, :cs] = np.frombuffer(challenge, dtype=np.uint8)
    m[:, cs:cs + 8] = (np.uint64(lo) + np.arange(n, dtype=np.uint64)).astype("<u8").view(np.uint8).reshape(n, 8)
    return m


def first_words(digests: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(digests[:, :8]).view("<u8").reshape(-1)


@functools.lru_cache(maxsize=None)
def ref_candidates(name, challenge: bytes, padding: int, lo: int, n: int = BLOCK) -> np.ndarray:
    """reference candidates of nonces lo .. lo + n - 1: hashlib where the standard library has the hash, the model otherwise"""
    if name in HASHLIB:
        f, tail = HASHLIB[name], bytes(padding)
        out = np.fromiter((int.from_bytes(f(challenge + k.to_bytes(8, "little") + tail).digest()[:8], "little") for k in range(lo, lo + n)), dtype=np.uint64, count=n)
    else:
        m = messages(challenge, padding, lo, n)
        out_len = 64 if name.endswith("512") else 32
        out = first_words(np.frombuffer(bm.hash_batch(name, m.tobytes(), m.shape[1], n), dtype=np.uint8).reshape(n, out_len))
    out.setflags(write=False)
    return out


def ref_candidate(name, challenge: bytes, padding: int, nonce: int) -> int:
    return int(ref_candidates(name, challenge, padding, nonce, 1)[0])


def ref_first(name, challenge: bytes, padding: int, bits: int, start: int = 0):
    """(smallest solving nonce >= start, its candidate), scanning aligned blocks"""
    thr = np.uint64(1 << (64 - bits))
    lo = start - start % BLOCK
    while True:
        c = ref_candidates(name, challenge, padding, lo)
        hit = np.flatnonzero(c[max(start - lo, 0):] < thr)
        if hit.size:
            k = max(start - lo, 0) + int(hit[0])
            return lo + k, int(c[k])
        lo += BLOCK


def config(padding=24, **keys):
    """(PowConfig, extension handle to destroy): keys = hip_pow_* extension ints"""
    from icicle_amd import PowConfig
    from icicle_amd._lib import lib

    cfg = PowConfig.default()
    cfg.padding_size = padding
    ext = None
    if keys:
        ext = lib.create_config_extension()
        for k, v in keys.items():
            lib.config_extension_set_int(ext, k.encode(), v)
        cfg.ext = ext
    return cfg, ext


def solve(h, challenge: bytes, bits, padding=24, **keys):
    import icicle_amd
    from icicle_amd._lib import lib

    cfg, ext = config(padding, **keys)
    got = icicle_amd.pow_solve(h, np.frombuffer(challenge, dtype=np.uint8), bits, cfg)
    if ext:
        lib.destroy_config_extension(ext)
    return got


def verify(h, challenge: bytes, bits, nonce, padding=24):
    import icicle_amd

    return icicle_amd.pow_verify(h, np.frombuffer(challenge, dtype=np.uint8), bits, nonce, config(padding)[0])


def start_keys(start):
    lo = start & 0xFFFFFFFF
    return {"hip_pow_start_lo": lo - (1 << 32) if lo >= 1 << 31 else lo, "hip_pow_start_hi": start >> 32}  # C ints


def bits_of(name):
    return [4, 8, 12, 16, 20] if name in HASHLIB else [4, 8, 12]


# ---- known answers ---------------------------------------------------------------------------------------------------------------
def test_blake3_known_answer_of_the_reference(hip):
    """wrappers/rust/icicle-hash/src/tests.rs (blake3_pow): challenge [20] * 32, 25 bits, default config"""
    ch = bytes([20] * 32)
    h = make("blake3")
    assert solve(h, ch, 25) == (True, 40825909, 364385878471)
    assert verify(h, ch, 25, 40825909) == (True, 364385878471)
    ok, mined = verify(h, ch, 25, 40825908)
    assert not ok and mined == ref_candidate("blake3", ch, 24, 40825908) >= 1 << 39
    h.close()


def test_keccak_shape_of_the_reference(hip):
    """tests.rs (keccak_pow): Keccak-256, challenge [20] * 21, padding 3, 25 bits -- found, and verify returns the same hash"""
    ch = bytes([20] * 21)
    h = make("keccak256")
    found, nonce, mined = solve(h, ch, 25, padding=3)
    assert found and mined < 1 << 39
    assert verify(h, ch, 25, nonce, padding=3) == (True, mined)
    assert mined == ref_candidate("keccak256", ch, 3, nonce)
    h.close()


# ---- the smallest nonce, whole and in spans -------------------------------------------------------------------------------------------
def test_reference_answers_on_file():
    """the SHA3-256 nonces the search below must return, as hashlib gives them"""
    assert [ref_first("sha3_256", CHALLENGE, 24, b)[0] for b in (4, 8, 12, 16, 20)] == [12, 884, 1877, 73175, 1049404]


@pytest.mark.parametrize("span", [None, 8, 12])
@pytest.mark.parametrize("name", NAMES)
def test_smallest_nonce(hip, name, span):
    """span 8 / 12: the solution lies in a later span than the first; at 4 bits some 260 nonces of one 4096-nonce span solve"""
    h = make(name)
    keys = {} if span is None else {"hip_pow_span_log2": span}
    for bits in bits_of(name):
        want, cand = ref_first(name, CHALLENGE, 24, bits)
        assert solve(h, CHALLENGE, bits, **keys) == (True, want, cand), (name, bits, span)
        assert verify(h, CHALLENGE, bits, want) == (True, cand)
    h.close()


@pytest.mark.parametrize("span", [8, 12])
@pytest.mark.parametrize("name", NAMES)
def test_solution_on_the_first_and_the_last_nonce_of_a_span(hip, name, span):
    h = make(name)
    bits = bits_of(name)[-1]
    want, cand = ref_first(name, CHALLENGE, 24, bits)
    n = 1 << span
    for back in (3 * n, 3 * n + n - 1, n - 1, 0):  # first of the fourth span, last of the fourth, last of the first, first of all
        start = want - back
        if start < 0:
            continue
        assert solve(h, CHALLENGE, bits, hip_pow_span_log2=span, **start_keys(start)) == (True, want, cand), (name, span, back)
    h.close()


@pytest.mark.parametrize("name", NAMES)
def test_no_smaller_nonce_solves_by_the_batch_kernels(hip, name):
    """20 bits: every message below the returned nonce goes through Hasher.hash; none is under the threshold, the returned one is"""
    h = make(name)
    found, nonce, mined = solve(h, CHALLENGE, 20)
    assert found and mined < 1 << 44
    out_len = h.output_size
    step = 1 << 19
    for lo in range(0, nonce + 1, step):
        n = min(step, nonce + 1 - lo)
        m = messages(CHALLENGE, 24, lo, n)
        c = first_words(h.hash(m.reshape(-1), size=64, batch=n).reshape(n, out_len))
        below = np.flatnonzero(c < np.uint64(1 << 44)) + lo
        assert list(below) == ([nonce] if lo + n == nonce + 1 else []), (name, lo)
        if lo + n == nonce + 1:
            assert int(c[-1]) == mined
    h.close()


# ---- message edges --------------------------------------------------------------------------------------------------------------
def edge_shapes(name):
    """(challenge size, padding): message sizes around the hash's block edges, the nonce across an edge, no challenge at all"""
    if name in ("keccak512", "sha3_512"):  # rate 72
        return [(32, 31), (32, 32), (32, 33), (68, 0), (68, 3), (0, 24), (7, 0)]
    if name in ("keccak256", "sha3_256"):  # rate 136
        return [(100, 27), (100, 28), (100, 29), (132, 0), (132, 3), (0, 24), (7, 0)]
    shapes = [(32, 23), (32, 24), (32, 25), (32, 88), (32, 89), (60, 0), (60, 24), (0, 24), (7, 0)]  # 63 64 65 128 129; nonce over byte 64
    return shapes + ([(32, 984), (1016, 0)] if name == "blake3" else [])  # one whole chunk


@pytest.mark.parametrize("name", NAMES)
def test_message_edges(hip, name):
    h = make(name)
    for cs, padding in edge_shapes(name):
        ch = bytes((29 * i + cs) & 0xFF for i in range(cs))
        want, cand = ref_first(name, ch, padding, 8)
        assert solve(h, ch, 8, padding=padding) == (True, want, cand), (name, cs, padding)
        for nonce in (1 << 32, (1 << 32) + 0x01020304, (1 << 63) + 5, (1 << 64) - 1):
            c = ref_candidate(name, ch, padding, nonce)
            assert verify(h, ch, 8, nonce, padding=padding) == (c < 1 << 56, c), (name, cs, padding, hex(nonce))
    h.close()


def test_blake3_beyond_one_chunk_is_refused(hip):
    import icicle_amd

    h = make("blake3")
    with pytest.raises(icicle_amd.IcicleError) as e:
        solve(h, CHALLENGE, 8, padding=985)
    assert e.value.code == 11
    h.close()


# ---- start, count, the carry into the upper word ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_search_across_2_to_the_32(hip, name):
    """10 bits from a start just below 2^32, chosen so that the reference's answer is at or above 2^32"""
    edge = 1 << 32
    solving = np.flatnonzero(ref_candidates(name, CHALLENGE, 24, edge - 64, 64) < np.uint64(1 << 54))
    start = edge - 64 + (int(solving[-1]) + 1 if solving.size else 0)  # behind the last nonce below 2^32 that solves
    assert start < edge, f"{name}: nonce 2^32 - 1 solves at 10 bits, no start below 2^32 has its answer above"
    want, cand = ref_first(name, CHALLENGE, 24, 10, start)
    assert start < edge <= want
    h = make(name)
    for span in (None, 8):
        keys = {} if span is None else {"hip_pow_span_log2": span}
        assert solve(h, CHALLENGE, 10, **keys, **start_keys(start)) == (True, want, cand), (name, span)
    assert verify(h, CHALLENGE, 10, want) == (True, cand)
    h.close()


@pytest.mark.parametrize("name", NAMES)
def test_count_bounds_the_search(hip, name):
    from icicle_amd import PowConfig
    from icicle_amd._lib import lib

    h = make(name)
    # 40 bits: no nonce below 4096 solves (the reference confirms it), so the search reports nothing and writes nothing
    assert int(ref_candidates(name, CHALLENGE, 24, 0).min()) >= 1 << 24
    for span in (None, 8):
        keys = {} if span is None else {"hip_pow_span_log2": span}
        assert solve(h, CHALLENGE, 40, hip_pow_count_log2=12, **keys) == (False, None, None)
    cfg, ext = config(24, hip_pow_count_log2=12)
    ch = np.frombuffer(CHALLENGE, dtype=np.uint8)
    found, nonce, mined = ctypes.c_bool(True), ctypes.c_uint64(77), ctypes.c_uint64(78)
    assert lib.proof_of_work(h.handle, ch.ctypes.data, 32, 40, ctypes.byref(cfg), ctypes.byref(found), ctypes.byref(nonce), ctypes.byref(mined)) == 0
    assert (found.value, nonce.value, mined.value) == (False, 77, 78)
    lib.destroy_config_extension(ext)
    # the count ends in front of the solution, or just behind it
    want, cand = ref_first(name, CHALLENGE, 24, 8)
    c = want.bit_length()  # 2^(c-1) <= want < 2^c
    assert want >= 1, "nonce 0 solves: no count excludes it"
    assert solve(h, CHALLENGE, 8, hip_pow_count_log2=c - 1) == (False, None, None)
    assert solve(h, CHALLENGE, 8, hip_pow_count_log2=c) == (True, want, cand)
    # counted from the start, not from 0
    assert solve(h, CHALLENGE, 8, hip_pow_count_log2=0, **start_keys(want)) == (True, want, cand)
    assert solve(h, CHALLENGE, 8, hip_pow_count_log2=0, **start_keys(want - 1)) == (False, None, None)
    h.close()


# ---- operands -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sha3_256", "keccak512", "blake2s", "blake3"])
def test_device_challenges_and_a_created_stream(hip, name):
    import icicle_amd
    from icicle_amd.runtime import DeviceVec, Stream

    h = make(name)
    ch = bytes((5 * i + 3) & 0xFF for i in range(37))
    want, cand = ref_first(name, ch, 11, 12)
    arr = np.frombuffer(ch, dtype=np.uint8)
    d = DeviceVec.from_host(arr)
    shifted = DeviceVec.from_host(np.concatenate([np.full(3, 0xEE, np.uint8), arr, np.full(12, 0xEE, np.uint8)]))
    st = Stream()
    for stream in (None, st.handle):
        cfg = config(11)[0]
        cfg.stream, cfg.is_async = stream, stream is not None
        assert icicle_amd.pow_solve(h, d, 12, cfg) == (True, want, cand)
        assert icicle_amd.pow_solve(h, shifted.ptr + 3, 12, cfg, size=37) == (True, want, cand)  # an odd device address
        assert icicle_amd.pow_verify(h, d, 12, want, cfg) == (True, cand)
        assert icicle_amd.pow_verify(h, shifted.ptr + 3, 12, want, cfg, size=37) == (True, cand)
        assert icicle_amd.pow_solve(h, arr, 12, cfg) == (True, want, cand)
        assert not cfg.is_challenge_on_device
    st.destroy()
    h.close()
