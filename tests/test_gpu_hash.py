"""GPU: the four Keccak-f[1600] hashers (icicle_hasher_hash) against the model (tests/merkle_model.py; its SHA3 modes are hashlib's) --
message lengths around every absorb boundary, batches across the wave and block edges, host / device operands, the byte path for
unaligned device pointers, an asynchronous call on a created stream."""
import hashlib

import numpy as np
import pytest

from tests import merkle_model as mm

pytestmark = pytest.mark.gpu

VARIANT_NAMES = ["keccak256", "keccak512", "sha3_256", "sha3_512"]
LENGTHS = {136: [1, 7, 8, 9, 31, 32, 64, 135, 136, 137, 271, 272, 273, 300], 72: [1, 71, 72, 73, 143, 144, 145]}
BATCHES = [1, 3, 65, 257]


def make(name, chunk=0):
    from icicle_amd.hash import Hasher

    return getattr(Hasher, name)(chunk)


def data(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def expect(name, buf, size, batch):
    if name.startswith("sha3"):  # ground truth where the standard library has it
        f = hashlib.sha3_256 if name == "sha3_256" else hashlib.sha3_512
        return b"".join(f(buf[i * size:(i + 1) * size].tobytes()).digest() for i in range(batch))
    return mm.hash_batch(name, buf.tobytes(), size, batch)


@pytest.mark.parametrize("name", VARIANT_NAMES)
def test_lengths_and_batches_host_operands(hip, name):
    h = make(name)
    rate = mm.VARIANTS[name][0]
    for size in LENGTHS[rate]:
        for batch in BATCHES:
            buf = data(size * batch, size * 1000 + batch)
            got = h.hash(buf, size=size, batch=batch)
            assert got.tobytes() == expect(name, buf, size, batch), (name, size, batch)
    h.close()


@pytest.mark.parametrize("name", VARIANT_NAMES)
@pytest.mark.parametrize("in_dev,out_dev", [(False, False), (False, True), (True, False), (True, True)])
def test_operand_locations(hip, name, in_dev, out_dev):
    from icicle_amd.runtime import DeviceVec

    h = make(name)
    rate = mm.VARIANTS[name][0]
    for size, batch in ((rate + 1, 65), (64, 257), (2 * rate, 3)):
        buf = data(size * batch, size + batch)
        inp = DeviceVec.from_host(buf) if in_dev else buf
        out = DeviceVec(batch * h.output_size) if out_dev else None
        got = h.hash(inp, size=size, batch=batch, out=out)
        got = got.to_host(np.uint8) if out_dev else got
        assert got.tobytes() == expect(name, buf, size, batch), (name, size, batch, in_dev, out_dev)
    h.close()


@pytest.mark.parametrize("name", VARIANT_NAMES)
def test_default_chunk_size(hip, name):
    from icicle_amd.hash import Hasher  # noqa: F401
    import icicle_amd

    h = make(name, 96)
    buf = data(96 * 5, 5)
    assert h.hash(buf, size=0, batch=5).tobytes() == expect(name, buf, 96, 5)
    assert h.hash(buf, size=32, batch=15).tobytes() == expect(name, buf, 32, 15)  # an explicit size wins
    h.close()
    none = make(name)
    with pytest.raises(icicle_amd.IcicleError) as e:
        none.hash(buf, size=0, batch=5)
    assert e.value.code == 11  # INVALID_ARGUMENT
    none.close()


@pytest.mark.parametrize("name", VARIANT_NAMES)
def test_unaligned_device_pointers_take_the_byte_path(hip, name):
    """33-byte messages from a device address one byte off the allocation, digests to an odd address as well"""
    from icicle_amd.runtime import DeviceVec

    h = make(name)
    batch = 130
    buf = data(1 + 33 * batch, 33)
    d_in = DeviceVec.from_host(buf)
    d_out = DeviceVec(1 + batch * h.output_size)
    h.hash(d_in.ptr + 1, size=33, batch=batch, out=d_out.ptr + 1)
    got = d_out.to_host(np.uint8)[1:]
    assert got.tobytes() == expect(name, buf[1:], 33, batch)
    h.close()


@pytest.mark.parametrize("name", VARIANT_NAMES)
def test_aligned_and_byte_path_agree(hip, name):
    from icicle_amd.runtime import DeviceVec

    h = make(name)
    batch = 1000
    msgs = data(64 * batch, 64)
    want = expect(name, msgs, 64, batch)
    aligned = DeviceVec.from_host(msgs)
    shifted = DeviceVec.from_host(np.concatenate([np.zeros(3, np.uint8), msgs]))
    a = h.hash(aligned, size=64, batch=batch)
    b = h.hash(shifted.ptr + 3, size=64, batch=batch)
    assert a.tobytes() == b.tobytes() == want
    # 8-aligned but not 16-aligned: 64-bit loads only
    shifted8 = DeviceVec.from_host(np.concatenate([np.zeros(8, np.uint8), msgs]))
    assert h.hash(shifted8.ptr + 8, size=64, batch=batch).tobytes() == want
    h.close()


def test_async_call_on_a_created_stream(hip):
    import icicle_amd
    from icicle_amd.runtime import DeviceVec, Stream

    h = make("keccak256")
    batch, size = 513, 200
    buf = data(size * batch, 9)
    d_in = DeviceVec.from_host(buf)
    d_out = DeviceVec(batch * 32)
    st = Stream()
    cfg = icicle_amd.HashConfig.default()
    cfg.stream = st.handle
    cfg.is_async = True
    h.hash(d_in, size=size, batch=batch, out=d_out, cfg=cfg)
    st.synchronize()
    assert d_out.to_host(np.uint8).tobytes() == expect("keccak256", buf, size, batch)
    st.destroy()
    h.close()


def test_foreign_extension_keys_are_tolerated(hip):
    import icicle_amd
    from icicle_amd._lib import lib

    ext = lib.create_config_extension()
    lib.config_extension_set_int(ext, b"n_threads", 4)  # the CPU backend's key
    cfg = icicle_amd.HashConfig.default()
    cfg.ext = ext
    h = make("sha3_256")
    buf = data(100, 1)
    assert h.hash(buf, cfg=cfg).tobytes() == hashlib.sha3_256(buf.tobytes()).digest()
    lib.destroy_config_extension(ext)
    h.close()
