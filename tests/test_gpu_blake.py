"""GPU: the Blake2s and Blake3 hashers (icicle_hasher_hash) against hashlib / the model (tests/blake_model.py, whose Blake3 is checked
against recorded digests) -- message lengths around every block edge and, for Blake3, around the chunk edges and the shapes of its
tree (2, 3, 4, 5 and 9 chunks), batches across the wave and block edges, host / device operands, the byte path for unaligned device
pointers, the default chunk size, an asynchronous call on a created stream."""
import functools
import hashlib

import numpy as np
import pytest

from tests import blake_model as bm

pytestmark = pytest.mark.gpu

NAMES = ["blake2s", "blake3"]
SHORT = [1, 55, 63, 64, 65, 127, 128, 129, 191, 192, 193, 300, 1000]
LENGTHS = {"blake2s": SHORT, "blake3": SHORT + [1023, 1024, 1025, 2049, 3073, 5120, 9216]}


def batches(size):
    return [1, 3, 65, 257] if size <= 1025 else [1, 65]


def make(name, chunk=0):
    from icicle_amd.hash import Hasher

    return getattr(Hasher, name)(chunk)


@functools.lru_cache(maxsize=None)
def data_bytes(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def data(n, seed):
    return np.frombuffer(data_bytes(n, seed), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def _expect(name, n, seed, size, batch):
    buf = data_bytes(n, seed)
    if name == "blake2s":  # ground truth where the standard library has it
        return b"".join(hashlib.blake2s(buf[i * size:(i + 1) * size]).digest() for i in range(batch))
    return bm.hash_batch(name, buf, size, batch)


def expect(name, n, seed, size, batch, skip=0):
    """digests of `batch` messages of `size` bytes from byte `skip` of data(n, seed) on"""
    if skip == 0:
        return _expect(name, n, seed, size, batch)
    buf = data_bytes(n, seed)[skip:]
    if name == "blake2s":
        return b"".join(hashlib.blake2s(buf[i * size:(i + 1) * size]).digest() for i in range(batch))
    return bm.hash_batch(name, buf, size, batch)


@pytest.mark.parametrize("name", NAMES)
def test_lengths_and_batches_host_operands(hip, name):
    h = make(name)
    for size in LENGTHS[name]:
        for batch in batches(size):
            n, seed = size * batch, size * 1000 + batch
            got = h.hash(data(n, seed), size=size, batch=batch)
            assert got.tobytes() == expect(name, n, seed, size, batch), (name, size, batch)
    h.close()


def test_known_answers(hip):
    """the reference's own tests (icicle/tests/test_hash_api.cpp:82-83, :105-108)"""
    msg = np.frombuffer(b"Hello world I am blake2s", dtype=np.uint8)
    assert make("blake2s").hash(msg).tobytes().hex() == "291c4b3648438cc57d1e965ee52e5572e8dc4938bc960e22d6ebe3a280aea759"
    text = ("Hello world I am blake3. This is a semi-long C++ test with a lot of characters. "
            "0123456789abcdef0123456789abcdef0123456789abcdef0123456789abcdef0123456789abcdef0123456789abcdef")
    msg = np.frombuffer(text.encode(), dtype=np.uint8)
    assert make("blake3").hash(msg).tobytes().hex() == "4b71f2c5cb7c26da2ba67cc742228e55b66c8b64b2b250e7ccce6f7f6d17c9ae"


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("in_dev,out_dev", [(False, False), (False, True), (True, False), (True, True)])
def test_operand_locations(hip, name, in_dev, out_dev):
    from icicle_amd.runtime import DeviceVec

    h = make(name)
    cases = [(65, 65), (64, 257), (128, 3)] + ([(3073, 65), (2049, 1)] if name == "blake3" else [])
    for size, batch in cases:
        n, seed = size * batch, size + batch
        buf = data(n, seed)
        inp = DeviceVec.from_host(buf) if in_dev else buf
        out = DeviceVec(batch * h.output_size) if out_dev else None
        got = h.hash(inp, size=size, batch=batch, out=out)
        got = got.to_host(np.uint8) if out_dev else got
        assert got.tobytes() == expect(name, n, seed, size, batch), (name, size, batch, in_dev, out_dev)
    h.close()


@pytest.mark.parametrize("name", NAMES)
def test_default_chunk_size(hip, name):
    import icicle_amd

    h = make(name, 96)
    n, seed = 96 * 5, 5
    buf = data(n, seed)
    assert h.hash(buf, size=0, batch=5).tobytes() == expect(name, n, seed, 96, 5)
    assert h.hash(buf, size=32, batch=15).tobytes() == expect(name, n, seed, 32, 15)  # an explicit size wins
    h.close()
    none = make(name)
    with pytest.raises(icicle_amd.IcicleError) as e:
        none.hash(buf, size=0, batch=5)
    assert e.value.code == 11  # INVALID_ARGUMENT
    none.close()


@pytest.mark.parametrize("name,size", [("blake2s", 33), ("blake3", 33), ("blake3", 2081)])
def test_unaligned_device_pointers_take_the_byte_path(hip, name, size):
    """messages of an odd size from a device address one byte off the allocation, digests to an odd address as well; 2081 bytes: three
    Blake3 chunks, the root level of the tree writes the unaligned digests"""
    from icicle_amd.runtime import DeviceVec

    h = make(name)
    batch = 130
    n, seed = 1 + size * batch, size
    d_in = DeviceVec.from_host(data(n, seed))
    d_out = DeviceVec(1 + batch * h.output_size)
    h.hash(d_in.ptr + 1, size=size, batch=batch, out=d_out.ptr + 1)
    got = d_out.to_host(np.uint8)[1:]
    assert got.tobytes() == expect(name, n, seed, size, batch, skip=1)
    h.close()


@pytest.mark.parametrize("name,size", [("blake2s", 64), ("blake3", 64), ("blake3", 2048)])
def test_aligned_and_byte_path_agree(hip, name, size):
    from icicle_amd.runtime import DeviceVec

    h = make(name)
    batch = 1000 if size == 64 else 67
    n, seed = size * batch, size
    msgs = data(n, seed)
    want = expect(name, n, seed, size, batch)
    aligned = DeviceVec.from_host(msgs)
    shifted = DeviceVec.from_host(np.concatenate([np.zeros(3, np.uint8), msgs]))
    a = h.hash(aligned, size=size, batch=batch)
    b = h.hash(shifted.ptr + 3, size=size, batch=batch)
    assert a.tobytes() == b.tobytes() == want
    # 8-aligned but not 16-aligned: 64-bit loads only
    shifted8 = DeviceVec.from_host(np.concatenate([np.zeros(8, np.uint8), msgs]))
    assert h.hash(shifted8.ptr + 8, size=size, batch=batch).tobytes() == want
    h.close()


@pytest.mark.parametrize("name,size", [("blake2s", 200), ("blake3", 200), ("blake3", 4100)])
def test_async_call_on_a_created_stream(hip, name, size):
    import icicle_amd
    from icicle_amd.runtime import DeviceVec, Stream

    h = make(name)
    batch = 513 if size == 200 else 33
    n, seed = size * batch, 9
    d_in = DeviceVec.from_host(data(n, seed))
    d_out = DeviceVec(batch * 32)
    st = Stream()
    cfg = icicle_amd.HashConfig.default()
    cfg.stream = st.handle
    cfg.is_async = True
    h.hash(d_in, size=size, batch=batch, out=d_out, cfg=cfg)
    st.synchronize()
    assert d_out.to_host(np.uint8).tobytes() == expect(name, n, seed, size, batch)
    st.destroy()
    h.close()
