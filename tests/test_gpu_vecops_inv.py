"""GPU: vector_inv / vector_div / vector_sum / vector_product against the reference CPU backend (oracle/_ref/libicicle_field_<F>.so,
src/vec_ops.cpp:9, 40, 217, 250), byte for byte, and against Python integers. The inverse of zero is zero: the reference returns that
for every one of the eight fields (checked on the CPU when these tests were written, goldilocks included), so zeros are compared against
the reference like every other value, and against the documented rule through Python's pow(0, p - 2, p) == 0.

T = icicle_hip_vector_inv_tile(words) elements share one inversion: lane l of a wave holds elements tile + j * 64 + l, j < T / 64. The
sizes and the zero positions below are taken from T, not from a copy of the constant."""
import ctypes
import functools
import os

import numpy as np
import pytest

from oracle import pyref

pytestmark = pytest.mark.gpu
FIELDS = {"babybear": 1, "koalabear": 1, "goldilocks": 2, "bn254": 8, "bls12_381": 8, "bls12_377": 8, "stark252": 8, "grumpkin": 8}  # words
ALL = list(FIELDS)
GRID_Y_MAX = 65535  # reduce_run launches one row of blocks per entry (per group of 64 entries in the along_k form), at most this many (the
#                     most a launch can have), and a block walks on from entry k to entry k + gridDim.y
INV_MAX_GRID = 2048  # k_vec_inv launches at most this many blocks of four waves (one tile per wave at a time) and loops beyond


def modulus(f):
    """a curve name stands for its scalar field"""
    return pyref.CURVES[f].r if f in pyref.CURVES else pyref.NTT_FIELDS[f].p


def words(vals, w):
    return np.frombuffer(b"".join(int(v).to_bytes(4 * w, "little") for v in vals), np.uint32).reshape(-1, w).copy()


def ints(arr, w):
    return [int.from_bytes(r.tobytes(), "little") for r in np.ascontiguousarray(arr).reshape(-1, w)]


def tile(f):
    from icicle_amd._lib import lib

    return lib.icicle_hip_vector_inv_tile(FIELDS[f])


def rand_vals(rng, n, p, nonzero=False):
    """n uniform values below p behind the directed prefix 0, 1, 2, p-1, (p+1)/2 (without it if nonzero)"""
    raw = rng.bytes(40 * n)
    vals = [int.from_bytes(raw[40 * i:40 * i + 40], "little") % p for i in range(n)]
    if nonzero:
        return [v or 1 for v in vals]
    pre = [0, 1, 2, p - 1, (p + 1) // 2]
    vals[:min(n, len(pre))] = pre[:min(n, len(pre))]
    return vals


def rand_words_nonzero(rng, n, f):
    """n x words uniform non-zero canonical elements, without a Python loop: for the large sizes"""
    p, w = modulus(f), FIELDS[f]
    if w == 1:
        return rng.integers(1, p, size=(n, 1), dtype=np.uint32)
    x = rng.integers(0, 1 << 32, size=(n, w), dtype=np.uint32)
    x[:, w - 1] %= np.uint32(p >> (32 * (w - 1)))  # top word below p's top word: the value is below p
    x[:, 0] |= 1
    return x


@functools.lru_cache(maxsize=None)
def _ref_lib(f):
    from oracle.ref import REF_DIR

    return ctypes.CDLL(os.path.join(REF_DIR, f"libicicle_field_{f}.so"))


def ref_op(f, op, a, b=None, size=None, batch=1, columns=False):
    """<field>_<op> of the reference on its CPU device, loaded the way tests/test_gpu_vecops.py loads vector_mul"""
    from oracle.ref import VecOpsConfig

    w = FIELDS[f]
    a = np.ascontiguousarray(a)
    if size is None:
        size = a.size // w // batch
    cfg = VecOpsConfig(None, False, False, False, False, batch, columns, None)
    out = np.zeros((batch, w), np.uint32) if op in ("vector_sum", "vector_product") else np.zeros_like(a)
    fn = getattr(_ref_lib(f), f"{f}_{op}")
    if op == "vector_div":
        b = np.ascontiguousarray(b)
        fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
        assert fn(a.ctypes.data, b.ctypes.data, size, ctypes.byref(cfg), out.ctypes.data) == 0
    else:
        fn.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
        assert fn(a.ctypes.data, size, ctypes.byref(cfg), out.ctypes.data) == 0
    return out


def batch_cfg(hip, batch=1, columns=False):
    cfg = hip.VecOpsConfig.default()
    cfg.batch_size, cfg.columns_batch = batch, columns
    return cfg


# ---- 1. inv / div equal the reference -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", ALL)
def test_inv_and_div_equal_the_reference(hip, f):
    from icicle_amd import vecops as V

    p, w, T = modulus(f), FIELDS[f], tile(f)
    rng = np.random.default_rng(1103)
    for n in (1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3):
        bv, av = rand_vals(rng, n, p), rand_vals(rng, n, p)[::-1]  # numerators reversed: the directed values meet other partners
        a, b = words(av, w), words(bv, w)
        inv = V.vector_inv(f, b)
        assert np.array_equal(inv, ref_op(f, "vector_inv", b)), (f, n)
        assert ints(inv, w) == [pow(x, p - 2, p) for x in bv], (f, n)
        div = V.vector_div(f, a, b)
        assert np.array_equal(div, ref_op(f, "vector_div", a, b)), (f, n)
        assert ints(div, w) == [x * pow(y, p - 2, p) % p for x, y in zip(av, bv)], (f, n)


# ---- 2. zeros do not spread ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", ["babybear", "goldilocks", "bn254"])
def test_zeros_do_not_spread(hip, f):
    from icicle_amd import vecops as V

    p, w, T = modulus(f), FIELDS[f], tile(f)
    K = T // 64
    rng = np.random.default_rng(1109)

    def check(vals, what):
        b = words(vals, w)
        a = words(rand_vals(rng, len(vals), p, nonzero=True), w)
        want = [pow(x, p - 2, p) for x in vals]  # 0 for 0
        assert all((x == 0) == (y == 0) for x, y in zip(vals, want))
        assert ints(V.vector_inv(f, b), w) == want, (f, what)
        assert ints(V.vector_div(f, a, b), w) == [x * y % p for x, y in zip(ints(a, w), want)], (f, what)

    n = 2 * T + 5
    # first and last of the vector, of lane 0, of lane 63 and of the first two tiles; the last tile is a partial one
    positions = sorted({0, n - 1, (K - 1) * 64, 63, T - 1, T, T + (K - 1) * 64, T + 63, 2 * T - 1, 2 * T})
    for pos in positions:  # one zero at a time
        vals = rand_vals(rng, n, p, nonzero=True)
        vals[pos] = 0
        check(vals, f"zero at {pos}")
    vals = rand_vals(rng, n, p, nonzero=True)
    for pos in positions:  # and all of them together
        vals[pos] = 0
    check(vals, "zeros at every directed position")
    vals = [0] * T + rand_vals(rng, T, p, nonzero=True)
    check(vals, "a tile of zeros before an ordinary tile")
    check(vals[::-1], "a tile of zeros after an ordinary tile")
    check([0] * (T + 7), "all zero")
    lane = rand_vals(rng, n, p, nonzero=True)
    for j in range(K):  # every element of lane 5 of the first tile
        lane[j * 64 + 5] = 0
    check(lane, "a whole lane of zeros")


# ---- 3. round trip at size ----------------------------------------------------------------------------------------------------------
def _assert_all_ones(arr, w, what):
    one = np.zeros(w, np.uint32)
    one[0] = 1
    assert (np.asarray(arr).reshape(-1, w) == one).all(), what


@pytest.mark.parametrize("f", ["babybear", "bn254"])
def test_round_trip_at_size(hip, f):
    from icicle_amd import vecops as V

    w, n = FIELDS[f], 1 << 16
    a = rand_words_nonzero(np.random.default_rng(1117), n, f)
    inv = V.vector_inv(f, a)
    _assert_all_ones(V.vector_mul(f, a, inv), w, (f, "a * inv(a)"))
    _assert_all_ones(V.vector_div(f, a, a.copy()), w, (f, "a / a"))


def test_round_trip_beyond_the_capped_grid(hip):
    """the launch caps its grid at INV_MAX_GRID blocks of four waves, a tile per wave, and a wave walks on to the tile one grid further:
    one element past cap * T puts exactly one element into the second round"""
    from icicle_amd import vecops as V
    from icicle_amd.runtime import DeviceVec

    f = "babybear"
    n = INV_MAX_GRID * 4 * tile(f) + 1
    if n > 1 << 24:
        pytest.skip("cap * T is beyond 2^24 elements")
    a = rand_words_nonzero(np.random.default_rng(1123), n, f)
    a[5] = a[n - 1] = 0  # a zero in each round
    da, dinv = DeviceVec.from_host(a), DeviceVec(a.nbytes)
    V.vector_inv(f, da, out=dinv, size=n)
    V.vector_mul(f, da, dinv, out=dinv, size=n)
    got = dinv.to_host()
    want = np.ones(n, np.uint32)
    want[5] = want[n - 1] = 0
    assert np.array_equal(got, want)
    V.vector_div(f, da, da, out=dinv, size=n)
    assert np.array_equal(dinv.to_host(), want)


# ---- 4. placement -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", ["babybear", "bn254"])
def test_placement(hip, f):
    from icicle_amd import vecops as V
    from icicle_amd.runtime import DeviceVec, Stream

    p, w, T = modulus(f), FIELDS[f], tile(f)
    rng = np.random.default_rng(1129)
    n = T + 37
    a, b = words(rand_vals(rng, n, p)[::-1], w), words(rand_vals(rng, n, p), w)
    want_inv, want_div = ref_op(f, "vector_inv", b), ref_op(f, "vector_div", a, b)

    def fetch(out):
        return out.to_host(shape=(n, w)) if isinstance(out, DeviceVec) else out

    # every mix of host and device for the operands and the output
    for a_dev in (False, True):
        for b_dev in (False, True):
            for o_dev in (False, True):
                xa, xb = (DeviceVec.from_host(a) if a_dev else a), (DeviceVec.from_host(b) if b_dev else b)
                out = DeviceVec(a.nbytes) if o_dev else np.zeros_like(a)
                assert np.array_equal(fetch(V.vector_div(f, xa, xb, out=out, size=n)), want_div), (f, "div", a_dev, b_dev, o_dev)
                if not a_dev:
                    out = DeviceVec(a.nbytes) if o_dev else np.zeros_like(a)
                    assert np.array_equal(fetch(V.vector_inv(f, xb, out=out, size=n)), want_inv), (f, "inv", b_dev, o_dev)
    # in place on the device
    d = DeviceVec.from_host(b)
    V.vector_inv(f, d, out=d, size=n)
    assert np.array_equal(fetch(d), want_inv)
    da, db = DeviceVec.from_host(a), DeviceVec.from_host(b)
    V.vector_div(f, da, db, out=da, size=n)
    assert np.array_equal(fetch(da), want_div)
    da = DeviceVec.from_host(a)
    V.vector_div(f, da, db, out=db, size=n)
    assert np.array_equal(fetch(db), want_div)
    # views one element into their allocations (4 bytes past a 16-byte boundary for a one-word field)
    eb = 4 * w
    pad = np.zeros((1, w), np.uint32)
    va, vb, vo = DeviceVec.from_host(np.concatenate([pad, a])), DeviceVec.from_host(np.concatenate([pad, b])), DeviceVec.from_host(np.concatenate([pad, a]))
    V.vector_div(f, va.ptr + eb, vb.ptr + eb, out=vo.ptr + eb, size=n)
    assert np.array_equal(vo.to_host(shape=(n + 1, w)), np.concatenate([pad, want_div]))
    V.vector_inv(f, vb.ptr + eb, out=vo.ptr + eb, size=n)
    assert np.array_equal(vo.to_host(shape=(n + 1, w)), np.concatenate([pad, want_inv]))
    s_dev = DeviceVec(eb)
    V.vector_sum(f, vb.ptr + eb, out=s_dev, size=n)
    assert np.array_equal(s_dev.to_host(shape=(1, w)), ref_op(f, "vector_sum", b))
    # a stream of its own, asynchronous, then a synchronise
    st = Stream()
    try:
        cfg = hip.VecOpsConfig.default()
        cfg.stream, cfg.is_async = st.handle, True
        da, db, do, di = DeviceVec.from_host(a), DeviceVec.from_host(b), DeviceVec(a.nbytes), DeviceVec(a.nbytes)
        V.vector_div(f, da, db, cfg, out=do, size=n)
        V.vector_inv(f, db, cfg, out=di, size=n)
        dsum, dprod = DeviceVec(eb), DeviceVec(eb)
        V.vector_sum(f, db, cfg, out=dsum, size=n)
        V.vector_product(f, da, cfg, out=dprod, size=n)
        st.synchronize()
        assert np.array_equal(fetch(do), want_div) and np.array_equal(fetch(di), want_inv)
        assert np.array_equal(dsum.to_host(shape=(1, w)), ref_op(f, "vector_sum", b))
        assert np.array_equal(dprod.to_host(shape=(1, w)), ref_op(f, "vector_product", a))
    finally:
        st.destroy()
    # a batch is only more elements: both layouts give what the flat call gives
    m = T // 2 + 11
    a3, b3 = words(rand_vals(rng, 3 * m, p), w), words(rand_vals(rng, 3 * m, p)[::-1], w)
    flat_inv, flat_div = V.vector_inv(f, b3), V.vector_div(f, a3, b3)
    assert np.array_equal(flat_inv, ref_op(f, "vector_inv", b3)) and np.array_equal(flat_div, ref_op(f, "vector_div", a3, b3))
    for columns in (False, True):
        assert np.array_equal(V.vector_inv(f, b3, batch_cfg(hip, 3, columns), size=m), flat_inv), (f, columns)
        assert np.array_equal(V.vector_div(f, a3, b3, batch_cfg(hip, 3, columns), size=m), flat_div), (f, columns)
        assert np.array_equal(ref_op(f, "vector_inv", b3, size=m, batch=3, columns=columns), flat_inv)


# ---- 5. sum / product equal the reference -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", ALL)
def test_sum_and_product_equal_the_reference(hip, f):
    from icicle_amd import vecops as V
    from icicle_amd.runtime import DeviceVec

    p, w = modulus(f), FIELDS[f]
    rng = np.random.default_rng(1151)

    def both(a, size, batch=1, columns=False, what=""):
        for op, fn in (("vector_sum", V.vector_sum), ("vector_product", V.vector_product)):
            got = fn(f, a, batch_cfg(hip, batch, columns), size=size)
            assert got.shape == (batch, w) and np.array_equal(got, ref_op(f, op, a, size=size, batch=batch, columns=columns)), (f, op, size, batch, columns, what)
        return got  # the product

    for size in (1, 2, 63, 64, 65, 257, 4099):
        vals = rand_vals(rng, size, p, nonzero=True)
        got = both(words(vals, w), size)
        if size <= 257:
            prod = 1
            for v in vals:
                prod = prod * v % p
            assert ints(got, w) == [prod], (f, size)
    for batch in (3, 64, 65):
        a = words(rand_vals(rng, 257 * batch, p, nonzero=True), w)
        for columns in (False, True):
            both(a, 257, batch, columns)
    # many short entries in one call
    both(words(rand_vals(rng, 64 * 130, p, nonzero=True), w), 64, 130, False, "short rows")
    both(words(rand_vals(rng, 64 * 130, p, nonzero=True), w), 64, 130, True, "short columns")
    # a zero in the vector: the product is zero
    vals = rand_vals(rng, 300, p, nonzero=True)
    vals[123] = 0
    assert not both(words(vals, w), 300, what="a zero").any()
    # all p - 1: the sum wraps at every step, the product is +-1
    for size in (300, 301):
        got = both(words([p - 1] * size, w), size, what="all p-1")
        assert ints(got, w) == [1 if size % 2 == 0 else p - 1]
    # device-resident input with a host result, and the other way round
    a = words(rand_vals(rng, 1000, p, nonzero=True), w)
    d = DeviceVec.from_host(a)
    for op, fn in (("vector_sum", V.vector_sum), ("vector_product", V.vector_product)):
        want = ref_op(f, op, a)
        assert np.array_equal(fn(f, d, size=1000), want), (f, op, "device in, host out")
        o = DeviceVec(4 * w)
        fn(f, a, out=o)
        assert np.array_equal(o.to_host(shape=(1, w)), want), (f, op, "host in, device out")


# ---- 6. beyond one block's partials -------------------------------------------------------------------------------------------------
def _column_sum(x, p):
    """the sum of n x w little-endian elements as a Python integer mod p"""
    cols = x.astype(np.uint64).sum(axis=0)  # n < 2^32 elements: no overflow
    return sum(int(c) << (32 * k) for k, c in enumerate(cols)) % p


@pytest.mark.parametrize("f", ["babybear", "bn254"])
def test_reductions_beyond_one_block_of_partials(hip, f):
    from icicle_amd import vecops as V
    from icicle_amd.runtime import DeviceVec

    p, w = modulus(f), FIELDS[f]
    rng = np.random.default_rng(1163)
    n = 1 << 20
    x = rand_words_nonzero(rng, n, f)
    d = DeviceVec.from_host(x)
    first = V.vector_sum(f, d, size=n)
    assert ints(first, w) == [_column_sum(x, p)]
    assert np.array_equal(V.vector_sum(f, d, size=n), first)  # the same bytes on every run
    rows = V.vector_sum(f, d, batch_cfg(hip, 4), size=n // 4)
    assert ints(rows, w) == [_column_sum(x[k * (n // 4):(k + 1) * (n // 4)], p) for k in range(4)]
    cols = V.vector_sum(f, d, batch_cfg(hip, 4, True), size=n // 4)
    assert ints(cols, w) == [_column_sum(x[k::4], p) for k in range(4)]

    m = 1 << 16
    y = x[:m]
    yi = ints(y, w)

    def prod(vals):
        r = 1
        for v in vals:
            r = r * v % p
        return r

    assert ints(V.vector_product(f, y), w) == [prod(yi)]
    assert ints(V.vector_product(f, y, batch_cfg(hip, 4), size=m // 4), w) == [prod(yi[k * (m // 4):(k + 1) * (m // 4)]) for k in range(4)]
    assert ints(V.vector_product(f, y, batch_cfg(hip, 4, True), size=m // 4), w) == [prod(yi[k::4]) for k in range(4)]


# ---- 7. more entries than the launch has rows of blocks -----------------------------------------------------------------------------
@pytest.mark.parametrize("size", [3, 65])
@pytest.mark.parametrize("f", ["babybear", "goldilocks", "bn254"])
def test_reductions_over_more_entries_than_rows_of_blocks(hip, f, size):
    """GRID_Y_MAX + 4 entries: the blocks of rows 0 to 3 reduce a second entry each. Rows layout: size 3 with one wave per block, size 65
    with four waves, which share the LDS buffer between the two syncs inside the loop over the entries. Columns layout: the along_k form,
    a lane per entry (its groups of 64 entries stay below the cap at this batch; the test below walks them)."""
    from icicle_amd import vecops as V
    from icicle_amd.runtime import DeviceVec

    p, w = modulus(f), FIELDS[f]
    batch = GRID_Y_MAX + 4
    assert batch > GRID_Y_MAX  # a second trip, for entries 0 to 3
    a = rand_words_nonzero(np.random.default_rng(1171 + size), size * batch, f)
    d = DeviceVec.from_host(a)
    for columns in (False, True):
        for op, fn in (("vector_sum", V.vector_sum), ("vector_product", V.vector_product)):
            want = ref_op(f, op, a, size=size, batch=batch, columns=columns)
            got = fn(f, a, batch_cfg(hip, batch, columns), size=size)
            assert got.shape == (batch, w) and np.array_equal(got, want), (f, op, size, columns, "host")
            o = DeviceVec(4 * w * batch)
            fn(f, d, batch_cfg(hip, batch, columns), size=size, out=o)
            assert np.array_equal(o.to_host(shape=(batch, w)), want), (f, op, size, columns, "device")
            if op == "vector_sum":  # and without the reference, where the trips meet
                for k in (0, 3, 4, GRID_Y_MAX - 1, GRID_Y_MAX, batch - 1):
                    entry = a[k::batch][:size] if columns else a[k * size:(k + 1) * size]
                    assert ints(got[k], w) == [_column_sum(entry, p)], (f, size, columns, k)


def test_column_reductions_over_more_groups_than_rows_of_blocks(hip):
    """the along_k form past the cap: GRID_Y_MAX * 64 + 1 entries in columns layout, so group 0's block (four waves, the LDS buffer)
    walks on to the group that holds the last entry alone; the second launch walks its own grid of 2^20 blocks as well"""
    from icicle_amd import vecops as V

    f, size = "babybear", 3
    batch = GRID_Y_MAX * 64 + 1
    assert (batch + 63) // 64 > GRID_Y_MAX
    a = rand_words_nonzero(np.random.default_rng(1181), size * batch, f)
    for op, fn in (("vector_sum", V.vector_sum), ("vector_product", V.vector_product)):
        got = fn(f, a, batch_cfg(hip, batch, True), size=size)
        assert np.array_equal(got, ref_op(f, op, a, size=size, batch=batch, columns=True)), op
