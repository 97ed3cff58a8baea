"""GPU: the extension-field vector operations (babybear, koalabear, goldilocks) byte for byte against the reference's recorded results
(tests/golden/vecops_ext_vectors.json), against the reference CPU backend itself (oracle/_ref/libicicle_field_<F>.so through ctypes, as
tests/test_gpu_vecops_inv.py does) and against Python integers (tests/vecops_ext_model.py).

T = icicle_hip_extension_vector_inv_tile(base words) elements share one base-field inversion of their norms: lane l of a wave holds
elements tile + j * 64 + l, j < T / 64. The sizes and the zero positions below are taken from T, not from a copy of the constant."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

from tests import vecops_ext_model as M

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ALL = list(M.FIELDS)
REDUCES = ("vector_sum", "vector_product")
GRID_Y_MAX = 65535  # reduce_run launches at most this many rows of blocks (one per entry; per 64 entries in the along_k form); a block walks on
INV_MAX_GRID = 2048  # k_vec_inv launches at most this many blocks of four waves (one tile per wave at a time) and loops beyond


@functools.lru_cache(maxsize=None)
def fixture():
    with open(os.path.join(HERE, "golden", "vecops_ext_vectors.json")) as fh:
        return json.load(fh)


def tile(f):
    from icicle_amd._lib import lib

    return lib.icicle_hip_extension_vector_inv_tile(M.BASE_WORDS[f])


def rand_ext(rng, n, f, nonzero=False):
    """[n, 4] uniform canonical extension elements, without a Python loop"""
    p = M.modulus(f)
    if M.BASE_WORDS[f] == 1:
        x = rng.integers(0, p, size=(n, 4), dtype=np.uint32)
    else:
        x = rng.integers(0, p, size=(n, 2), dtype=np.uint64).view(np.uint32).reshape(n, 4)
    if nonzero:
        x[~x.any(axis=1), 0] = 1
    return np.ascontiguousarray(x)


def rand_base(rng, n, f):
    p = M.modulus(f)
    if M.BASE_WORDS[f] == 1:
        return rng.integers(0, p, size=(n, 1), dtype=np.uint32)
    return np.ascontiguousarray(rng.integers(0, p, size=(n, 1), dtype=np.uint64).view(np.uint32).reshape(n, 2))


@functools.lru_cache(maxsize=None)
def _ref_lib(f):
    from oracle.ref import REF_DIR

    return ctypes.CDLL(os.path.join(REF_DIR, f"libicicle_field_{f}.so"))


def ref_op(f, op, a, b=None, size=None, batch=1, columns=False):
    """<field>_extension_<op> of the reference on its CPU device"""
    from oracle.ref import VecOpsConfig

    a = np.ascontiguousarray(a)
    if size is None:
        size = (b if op.startswith("scalar_") else a).size // 4 // batch
    cfg = VecOpsConfig(None, False, False, False, False, batch, columns, None)
    out = np.zeros((batch if op in REDUCES else size * batch, 4), np.uint32)
    fn = getattr(_ref_lib(f), f"{f}_extension_{op}")
    if b is not None:
        b = np.ascontiguousarray(b)
        fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
        assert fn(a.ctypes.data, b.ctypes.data, size, ctypes.byref(cfg), out.ctypes.data) == 0
    else:
        fn.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
        assert fn(a.ctypes.data, size, ctypes.byref(cfg), out.ctypes.data) == 0
    return out


def hip_op(f, op, a, b=None, size=None, batch=1, columns=False, out=None, cfg=None):
    from icicle_amd import VecOpsConfig, vecops as V

    cfg = cfg or VecOpsConfig.default()
    cfg.batch_size, cfg.columns_batch = batch, columns
    if op == "vector_mixed_mul":
        return V.vector_mixed_mul(f, a, b, cfg, out, size)
    fn = getattr(V, op)
    if b is not None:
        return fn(f, a, b, cfg, out, size, extension=True)
    return fn(f, a, cfg, out, size, extension=True)


def model_rows(f, op, a, b, idx):
    """the model's result of an element-wise op at the positions idx, as [len(idx), 4] words"""
    ea = M.from_words(f, a[idx])
    if op == "vector_inv":
        return M.to_words(f, [M.inv(f, x) for x in ea])
    if op == "vector_mixed_mul":
        cb = 4 * M.BASE_WORDS[f]
        raw = np.ascontiguousarray(b[idx]).tobytes()
        return M.to_words(f, [M.mul_base(f, x, int.from_bytes(raw[cb * i:cb * i + cb], "little")) for i, x in enumerate(ea)])
    g = {"vector_add": M.add, "vector_sub": M.sub, "vector_mul": M.mul, "vector_div": M.div}[op]
    return M.to_words(f, [g(f, x, y) for x, y in zip(ea, M.from_words(f, b[idx]))])


# ---- 1. every recorded case, host operands and device operands ----------------------------------------------------------------------
@pytest.mark.parametrize("f", ALL)
def test_fixture_cases(hip, f):
    from icicle_amd.runtime import DeviceVec

    for c in (c for c in fixture()["cases"] if c["field"] == f):
        op, size, batch, columns = c["op"], c["size"], c["batch"], c["columns"]
        a = np.frombuffer(bytes.fromhex(c["a"]), np.uint32).reshape(-1, 4).copy()
        b = None if c["b"] is None else np.frombuffer(bytes.fromhex(c["b"]), np.uint32).copy()
        want = np.frombuffer(bytes.fromhex(c["out"]), np.uint32).reshape(-1, 4)
        what = (f, op, size, batch, columns)
        assert np.array_equal(hip_op(f, op, a, b, size, batch, columns, out=np.zeros_like(want)), want), what
        da, db, do = DeviceVec.from_host(a), None if b is None else DeviceVec.from_host(b), DeviceVec(want.nbytes)
        hip_op(f, op, da, db, size, batch, columns, out=do)
        assert np.array_equal(do.to_host(shape=want.shape), want), what + ("device",)


# ---- 2. sizes around a wave, a block and a tile -------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", ALL)
def test_sizes(hip, f):
    T = tile(f)
    rng = np.random.default_rng(2203)
    for n in (1, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 2 * T + 3):
        a, b, base, s = rand_ext(rng, n, f), rand_ext(rng, n, f), rand_base(rng, n, f), rand_ext(rng, 1, f)
        b[n // 2] = 0  # a zero among the divisors
        idx = np.unique(np.array([0, n // 2, n - 1] + list(rng.integers(0, n, size=3))))
        for op in ("vector_add", "vector_sub", "vector_mul", "vector_div", "vector_mixed_mul", "vector_inv"):
            y = base if op == "vector_mixed_mul" else None if op == "vector_inv" else b
            x = b if op == "vector_inv" else a
            got = hip_op(f, op, x, y, out=np.zeros_like(a))
            assert np.array_equal(got, ref_op(f, op, x, y)), (f, op, n)
            assert np.array_equal(got[idx], model_rows(f, op, x, y, idx)), (f, op, n, "model")
        for op in ("scalar_add_vec", "scalar_sub_vec", "scalar_mul_vec"):
            assert np.array_equal(hip_op(f, op, s, b), ref_op(f, op, s, b)), (f, op, n)


# ---- 3. zeros ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", ALL)
def test_zeros(hip, f):
    T = tile(f)
    rng = np.random.default_rng(2207)
    n = 3 * T + 5
    a, clean = rand_ext(rng, n, f), rand_ext(rng, n, f, nonzero=True)
    inv_clean = hip_op(f, "vector_inv", clean)
    assert np.array_equal(inv_clean, ref_op(f, "vector_inv", clean))
    layouts = {
        "lanes and tile edges": [0, 63, 64, T - 1, T, 2 * T - 1, 2 * T, n - 1],  # lane 0, the last lane of a wave, first and last of a tile
        "a whole tile": list(range(T, 2 * T)),
        "the whole vector": list(range(n)),
    }
    for what, zeros in layouts.items():
        b = clean.copy()
        b[zeros] = 0
        keep = np.ones(n, bool)
        keep[zeros] = False
        inv, div = hip_op(f, "vector_inv", b), hip_op(f, "vector_div", a, b)
        assert not inv[zeros].any() and not div[zeros].any(), (f, what)  # 1 / 0 = 0 and a / 0 = 0
        assert np.array_equal(inv[keep], inv_clean[keep]), (f, what, "neighbours")
        assert np.array_equal(inv, ref_op(f, "vector_inv", b)) and np.array_equal(div, ref_op(f, "vector_div", a, b)), (f, what)
    assert M.from_words(f, inv_clean[:3]) == [M.inv(f, x) for x in M.from_words(f, clean[:3])]


# ---- 4. pointers and placement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", ["babybear", "goldilocks"])
def test_pointers_and_placement(hip, f):
    from icicle_amd.runtime import DeviceVec, Stream

    T = tile(f)
    rng = np.random.default_rng(2213)
    n = T + 37
    a, b, base = rand_ext(rng, n, f), rand_ext(rng, n, f), rand_base(rng, n, f)
    b[5] = 0
    want = {op: ref_op(f, op, a, base if op == "vector_mixed_mul" else b) for op in ("vector_mul", "vector_div", "vector_add", "vector_mixed_mul")}
    want["vector_inv"], want["vector_sum"], want["vector_product"] = ref_op(f, "vector_inv", b), ref_op(f, "vector_sum", a), ref_op(f, "vector_product", a)

    def fetch(out, rows=n):
        return out.to_host(shape=(rows, 4)) if isinstance(out, DeviceVec) else out

    # device pointers 4 bytes past a 16-byte boundary take the word path: the same bytes as the aligned path gives
    pad = np.zeros(1, np.uint32)
    va, vb, vo = (DeviceVec.from_host(np.concatenate([pad, x.reshape(-1)])) for x in (a, b, a))
    vbase = DeviceVec.from_host(np.concatenate([pad, base.reshape(-1)]))
    for op in ("vector_mul", "vector_div", "vector_add", "vector_mixed_mul", "vector_inv"):
        x = vb if op == "vector_inv" else va
        y = None if op == "vector_inv" else (vbase.ptr + 4 if op == "vector_mixed_mul" else vb.ptr + 4)
        hip_op(f, op, x.ptr + 4, y, size=n, out=vo.ptr + 4)
        got = vo.to_host()
        assert got[0] == 0 and np.array_equal(got[1:].reshape(n, 4), want[op]), (f, op, "misaligned")
        aligned = hip_op(f, op, DeviceVec.from_host(b if op == "vector_inv" else a), None if op == "vector_inv" else DeviceVec.from_host(base if op == "vector_mixed_mul" else b),
                         size=n, out=DeviceVec(a.nbytes))
        assert np.array_equal(fetch(aligned), got[1:].reshape(n, 4)), (f, op, "aligned against misaligned")
    for op in REDUCES:
        s_dev = DeviceVec(16 + 4)
        hip_op(f, op, va.ptr + 4, size=n, out=s_dev.ptr + 4)
        assert np.array_equal(s_dev.to_host()[1:].reshape(1, 4), want[op]), (f, op, "misaligned")
    # a host array view at an odd word offset
    buf = np.zeros(4 * n + 1, np.uint32)
    buf[1:] = a.reshape(-1)
    view = buf[1:].reshape(n, 4)
    assert np.array_equal(hip_op(f, "vector_mul", view, b), want["vector_mul"])
    # in place: result == vec_a, result == vec_b
    for op in ("vector_mul", "vector_div", "vector_add"):
        da, db = DeviceVec.from_host(a), DeviceVec.from_host(b)
        hip_op(f, op, da, db, size=n, out=da)
        assert np.array_equal(fetch(da), want[op]), (f, op, "out is a")
        da = DeviceVec.from_host(a)
        hip_op(f, op, da, db, size=n, out=db)
        assert np.array_equal(fetch(db), want[op]), (f, op, "out is b")
    d = DeviceVec.from_host(b)
    hip_op(f, "vector_inv", d, size=n, out=d)
    assert np.array_equal(fetch(d), want["vector_inv"])
    ha = a.copy()
    hip_op(f, "vector_mul", ha, b, out=ha)
    assert np.array_equal(ha, want["vector_mul"])
    # every mix of host and device for a, b and the result
    for a_dev in (False, True):
        for b_dev in (False, True):
            for o_dev in (False, True):
                xa, xb = (DeviceVec.from_host(a) if a_dev else a), (DeviceVec.from_host(b) if b_dev else b)
                for op in ("vector_mul", "vector_div"):
                    out = DeviceVec(a.nbytes) if o_dev else np.zeros_like(a)
                    assert np.array_equal(fetch(hip_op(f, op, xa, xb, size=n, out=out)), want[op]), (f, op, a_dev, b_dev, o_dev)
    # a stream of its own, asynchronous, then a synchronise
    st = Stream()
    try:
        cfg = hip.VecOpsConfig.default()
        cfg.stream, cfg.is_async = st.handle, True
        da, db, do, di, ds = DeviceVec.from_host(a), DeviceVec.from_host(b), DeviceVec(a.nbytes), DeviceVec(a.nbytes), DeviceVec(16)
        hip_op(f, "vector_div", da, db, size=n, out=do, cfg=cfg)
        hip_op(f, "vector_inv", db, size=n, out=di, cfg=cfg)
        hip_op(f, "vector_product", da, size=n, out=ds, cfg=cfg)
        st.synchronize()
        assert np.array_equal(fetch(do), want["vector_div"]) and np.array_equal(fetch(di), want["vector_inv"])
        assert np.array_equal(fetch(ds, 1), want["vector_product"])
    finally:
        st.destroy()


# ---- 5. sum and product -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", ALL)
def test_sum_and_product(hip, f):
    rng = np.random.default_rng(2221)
    pool = rand_ext(rng, 5000 * 1000, f, nonzero=True)  # one pool, every case a prefix of it
    for batch in (1, 3, 64, 1000):
        for columns in (False, True):
            for size in (1, 2, 255, 256, 257, 5000):
                a = pool[:size * batch]
                for op in REDUCES:
                    got = hip_op(f, op, a, size=size, batch=batch, columns=columns)
                    assert got.shape == (batch, 4)
                    assert np.array_equal(got, ref_op(f, op, a, size=size, batch=batch, columns=columns)), (f, op, batch, columns, size)
                    if size in (257, 5000):
                        assert np.array_equal(got, hip_op(f, op, a, size=size, batch=batch, columns=columns)), (f, op, "two runs")
    a = pool[:3 * 7]
    for columns in (False, True):  # against the model
        ea = M.from_words(f, a)
        for op in REDUCES:
            assert M.from_words(f, hip_op(f, op, a, size=7, batch=3, columns=columns)) == M.run(f, op, ea, None, 7, 3, columns)


@pytest.mark.parametrize("size", [3, 65])
def test_sum_and_product_over_more_entries_than_rows_of_blocks(hip, size):
    """GRID_Y_MAX + 4 entries of the babybear extension, rows layout (blocks 0 to 3 reduce a second entry; four waves and the LDS buffer at
    size 65) and columns layout (the along_k form), host input and device input with a device result: every entry against the model in
    its vectorised form (M.reduce_np), those where the trips meet against the model itself"""
    from icicle_amd.runtime import DeviceVec

    f = "babybear"
    batch = GRID_Y_MAX + 4
    assert batch > GRID_Y_MAX
    a = rand_ext(np.random.default_rng(2243 + size), size * batch, f, nonzero=True)
    d = DeviceVec.from_host(a)
    spots = (0, 3, 4, GRID_Y_MAX - 1, GRID_Y_MAX, batch - 1)
    for columns in (False, True):
        for op in REDUCES:
            want = M.reduce_np(f, op, a, size, batch, columns)
            got = hip_op(f, op, a, size=size, batch=batch, columns=columns)
            assert got.shape == (batch, 4) and np.array_equal(got, want), (op, size, columns, "host")
            o = DeviceVec(16 * batch)
            hip_op(f, op, d, size=size, batch=batch, columns=columns, out=o)
            assert np.array_equal(o.to_host(shape=(batch, 4)), want), (op, size, columns, "device")
            for k in spots:
                entry = M.from_words(f, a[k::batch][:size] if columns else a[k * size:(k + 1) * size])
                assert M.from_words(f, got[k]) == M.run(f, op, entry, None, size, 1, False), (op, size, columns, k)


# ---- 6. one size past the grid cap ---------------------------------------------------------------------------------------------------
def test_past_the_grid_cap(hip):
    from icicle_amd.runtime import DeviceVec

    f = "koalabear"
    T = tile(f)
    n = INV_MAX_GRID * 4 * T + T + 5
    rng = np.random.default_rng(2237)
    a = rand_ext(rng, n, f, nonzero=True)
    da, di = DeviceVec.from_host(a), DeviceVec(a.nbytes)
    hip_op(f, "vector_inv", da, size=n, out=di)
    hip_op(f, "vector_mul", da, di, size=n, out=da)
    prod = da.to_host(shape=(n, 4))
    assert (prod[:, 0] == 1).all() and not prod[:, 1:].any()
    idx = np.unique(np.concatenate([[0, n - 1, INV_MAX_GRID * 4 * T - 1, INV_MAX_GRID * 4 * T], rng.integers(0, n, size=1000)]))
    inv = di.to_host(shape=(n, 4))
    assert np.array_equal(inv[idx], model_rows(f, "vector_inv", a, None, idx))


# ---- 7. bit_reverse -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", ALL)
def test_bit_reverse(hip, f):
    from icicle_amd.runtime import DeviceVec

    rng = np.random.default_rng(2239)
    for logn in (1, 5, 12):
        n = 1 << logn
        a = rand_ext(rng, n, f)
        perm = np.array([int(format(j, f"0{logn}b")[::-1], 2) for j in range(n)])
        want = a[perm]  # an involution: out[rev(j)] = a[j] is out[j] = a[rev(j)]
        assert np.array_equal(hip_op(f, "bit_reverse", a), want), (f, logn)
        assert np.array_equal(want, ref_op(f, "bit_reverse", a)), (f, logn)
        d = DeviceVec.from_host(a)
        hip_op(f, "bit_reverse", d, size=n, out=d)
        assert np.array_equal(d.to_host(shape=(n, 4)), want), (f, logn, "in place on the device")
        h = a.copy()
        hip_op(f, "bit_reverse", h, out=h)
        assert np.array_equal(h, want), (f, logn, "in place on the host")


# ---- 8. mixed_mul is mul with the base vector embedded -----------------------------------------------------------------------------
@pytest.mark.parametrize("f", ALL)
def test_mixed_mul_is_mul_by_the_embedded_vector(hip, f):
    rng = np.random.default_rng(2243)
    n = 1000
    a, base = rand_ext(rng, n, f), rand_base(rng, n, f)
    base[:3] = 0
    base[3, 0] = 1
    emb = np.zeros((n, 4), np.uint32)
    emb[:, :M.BASE_WORDS[f]] = base
    assert np.array_equal(hip_op(f, "vector_mixed_mul", a, base), hip_op(f, "vector_mul", a, emb))
