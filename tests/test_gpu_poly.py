"""GPU: slice, highest_non_zero_idx, poly_eval and poly_division (icicle_amd/csrc/vecops_poly.hip) against the
reference CPU backend (oracle/_ref/libicicle_field_<F>.so), byte for byte where the reference is defined, against the Python model
(tests/poly_model.py) everywhere, and against Python integers (q * b + r == numerator). tests/test_poly_model_cpu.py pins on the CPU
where the reference is defined and that the model agrees with it there; tests/poly_ref.py states those rules. For row batches of the
division the reference is called once per entry at batch_size == 1.

T = icicle_hip_poly_division_tile(words) quotient coefficients per tile: the shapes are taken from it, not from a copy of the constant."""
import numpy as np
import pytest

from tests import poly_model as M
from tests import poly_ref as R

pytestmark = pytest.mark.gpu
INVALID_POINTER, INVALID_ARGUMENT = 3, 11
GRID_Y_MAX = 65535  # k_hnz and k_poly_eval_point: one row of blocks per entry, at most this many (the most a launch can have); a block walks on
HNZ_GRID = 1024 * 4096  # poly_plan.h: at most POLY_HNZ_MAX_CHUNKS blocks of POLY_HNZ_PER_BLOCK elements along an entry, longer chunks beyond


def cfg_of(hip, batch=1, columns=False):
    cfg = hip.VecOpsConfig.default()
    cfg.batch_size, cfg.columns_batch = batch, columns
    return cfg


def raises_code(code, fn, *a, **kw):
    import icicle_amd

    with pytest.raises(icicle_amd.IcicleError) as e:
        fn(*a, **kw)
    assert e.value.code == code, e.value


def rand_words(rng, n, f):
    """n x words uniform canonical elements without a Python loop: for the large sizes"""
    p, w = R.modulus(f), R.FIELDS[f]
    if w == 1:
        return rng.integers(0, p, size=(n, 1), dtype=np.uint32)
    x = rng.integers(0, 1 << 32, size=(n, w), dtype=np.uint32)
    x[:, w - 1] %= np.uint32(p >> (32 * (w - 1)))  # top word below p's top word: the value is below p
    return x


# ---- slice ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", R.ALL)
def test_slice(hip, f):
    from icicle_amd import vecops as V
    from icicle_amd.runtime import DeviceVec

    p, w = R.modulus(f), R.FIELDS[f]
    rng = np.random.default_rng(3301)
    n = 1029  # more than one block; (n - 4) % 5 == 0
    shapes = ((0, 1, n), (1, 2, n // 2), (n - 1, 1, 1), (3, 5, (n - 4) // 5 + 1))
    assert 3 + 5 * (shapes[3][2] - 1) == n - 1
    for batch, columns in ((1, False), (3, False), (3, True)):
        vals = R.rand_vals(rng, n * batch, p)
        a = R.words(vals, w)
        da = DeviceVec.from_host(a)
        for offset, stride, size_out in shapes:
            want = R.ref_slice(f, a, offset, stride, n, size_out, batch, columns)
            assert R.ints(want, w) == M.slice_(vals, offset, stride, n, size_out, batch, columns)
            got = V.slice(f, a, offset, stride, size_out, cfg_of(hip, batch, columns))
            assert got.shape == (size_out * batch, w) and np.array_equal(got, want), (f, batch, columns, offset, stride)
            # device operands, and one of each
            do = DeviceVec(want.nbytes)
            V.slice(f, da, offset, stride, size_out, cfg_of(hip, batch, columns), out=do, size_in=n)
            assert np.array_equal(do.to_host(shape=want.shape), want), (f, "device", batch, columns, offset, stride)
            assert np.array_equal(V.slice(f, da, offset, stride, size_out, cfg_of(hip, batch, columns), size_in=n), want)
            do2 = DeviceVec(want.nbytes)
            V.slice(f, a, offset, stride, size_out, cfg_of(hip, batch, columns), out=do2)
            assert np.array_equal(do2.to_host(shape=want.shape), want)
        # one index past the end: an error, and the output is untouched
        offset, stride, size_out = shapes[3]
        for bad in ((offset, stride, size_out + 1), (offset + 1, stride, size_out), (n, 0, 2), (0, 1, n + 1)):
            out = np.full((bad[2] * batch, w), 0xA5A5A5A5, np.uint32)
            raises_code(INVALID_ARGUMENT, V.slice, f, a, bad[0], bad[1], bad[2], cfg_of(hip, batch, columns), out=out)
            assert (out == 0xA5A5A5A5).all()
            dout = DeviceVec.from_host(out)
            raises_code(INVALID_ARGUMENT, V.slice, f, da, bad[0], bad[1], bad[2], cfg_of(hip, batch, columns), out=dout, size_in=n)
            assert (dout.to_host() == 0xA5A5A5A5).all()
    # stride 0 inside the range, an empty call, and overlapping device buffers
    assert np.array_equal(V.slice(f, a, 7, 0, 4, cfg_of(hip, 3, False)), R.ref_slice(f, a, 7, 0, n, 4, 3, False))
    assert V.slice(f, a, n + 5, 1, 0).shape == (0, w)
    raises_code(INVALID_ARGUMENT, V.slice, f, da, 0, 2, 8, out=da.ptr + 4 * w, size_in=n)
    # a view one element into its allocation (not 16-byte aligned for the narrow fields)
    do = DeviceVec(8 * 4 * w)
    V.slice(f, da.ptr + 4 * w, 1, 3, 8, out=do, size_in=n - 1)
    assert np.array_equal(do.to_host(shape=(8, w)), a[2:2 + 24:3])


# ---- highest_non_zero_idx ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", R.ALL)
def test_highest_non_zero_idx(hip, f):
    from icicle_amd import vecops as V
    from icicle_amd.runtime import DeviceVec

    p, w = R.modulus(f), R.FIELDS[f]
    rng = np.random.default_rng(3313)
    for size in (1, 63, 64, 65, 255, 256, 257, 4096, 4097, 9001):
        cases = [[0] * size, [p - 1] + [0] * (size - 1), [0] * (size - 1) + [1]]
        if size > 2:
            mid = [0] * size
            mid[size // 2] = 1 << 32 if w > 1 else 7  # multi-word fields: the low word is zero, the element is not
            mid[0] = 1
            cases.append(mid)
        for vals in cases:
            a = R.words(vals, w)
            got = V.highest_non_zero_idx(f, a)
            assert got.dtype == np.int64 and list(got) == [M.degree(vals)] == list(R.ref_hnz(f, a, size)), (f, size)
        # batch 3, a different answer per entry, on the host and on the device
        ents = [cases[-1], cases[0], cases[2]]
        for columns in (False, True):
            flat = M.pack(ents, columns)
            a = R.words(flat, w)
            want = [M.degree(e) for e in ents]
            assert list(R.ref_hnz(f, a, size, 3, columns)) == want
            assert list(V.highest_non_zero_idx(f, a, cfg_of(hip, 3, columns))) == want, (f, size, columns)
            do = DeviceVec(3 * 8)
            V.highest_non_zero_idx(f, DeviceVec.from_host(a), cfg_of(hip, 3, columns), size=size, out=do)
            assert list(do.to_host(dtype=np.int64)) == want, (f, size, columns, "device")
    # uniform values: the last element
    a = R.words(R.rand_vals(rng, 300, p, nonzero=True), w)
    assert list(V.highest_non_zero_idx(f, a, cfg_of(hip, 3), size=100)) == [99, 99, 99]
    raises_code(INVALID_ARGUMENT, V.highest_non_zero_idx, f, a, size=0)


@pytest.mark.parametrize("f", R.PER_TYPE)
def test_highest_non_zero_idx_beyond_a_whole_grid_of_blocks(hip, f):
    """one element more than the blocks of a full grid cover at their first chunk length: the chunks grow, the answer does not change"""
    from icicle_amd import vecops as V
    from icicle_amd.runtime import DeviceVec

    w = R.FIELDS[f]
    n = HNZ_GRID + 1
    a = np.zeros((n, w), np.uint32)
    d = DeviceVec.from_host(a)
    assert list(V.highest_non_zero_idx(f, d, size=n)) == [-1]
    for pos in (0, 4097, HNZ_GRID - 1, HNZ_GRID):
        a[pos, w - 1] = 1
        d = DeviceVec.from_host(a)
        assert list(V.highest_non_zero_idx(f, d, size=n)) == [pos], (f, pos)
    assert list(R.ref_hnz(f, a, n)) == [HNZ_GRID]


@pytest.mark.parametrize("size", [3, 65])
@pytest.mark.parametrize("f", ["babybear", "bn254"])
def test_highest_non_zero_idx_of_more_entries_than_rows_of_blocks(hip, f, size):
    """GRID_Y_MAX + 4 entries: blocks 0 to 3 scan a second entry each, through the same LDS slots. Every answer from -1 to size - 1
    occurs; entries 0, GRID_Y_MAX - 1, GRID_Y_MAX and the last have four different ones, -1 among them."""
    from icicle_amd import vecops as V
    from icicle_amd.runtime import DeviceVec

    w = R.FIELDS[f]
    batch = GRID_Y_MAX + 4
    assert batch > GRID_Y_MAX
    rng = np.random.default_rng(3331 + size)
    deg = np.arange(batch, dtype=np.int64) % (size + 1) - 1
    deg[[0, GRID_Y_MAX - 1, GRID_Y_MAX, batch - 1]] = [size - 1, 0, -1, 1]
    j = np.arange(size)
    below = (j[None, :] < deg[:, None]) & (rng.integers(0, 2, size=(batch, size)) == 1)  # some non-zero elements below the answer
    arr = np.zeros((batch, size, w), np.uint32)
    arr[:, :, w - 1] = (below | (j[None, :] == deg[:, None])).astype(np.uint32)  # multi-word fields: the low words are zero, the element is not
    for columns in (False, True):
        a = np.ascontiguousarray(arr.transpose(1, 0, 2) if columns else arr).reshape(-1, w)
        assert np.array_equal(R.ref_hnz(f, a, size, batch, columns), deg)
        got = V.highest_non_zero_idx(f, a, cfg_of(hip, batch, columns), size=size)
        assert got.dtype == np.int64 and np.array_equal(got, deg), (f, size, columns, "host")
        do = DeviceVec(8 * batch)
        V.highest_non_zero_idx(f, DeviceVec.from_host(a), cfg_of(hip, batch, columns), size=size, out=do)
        assert np.array_equal(do.to_host(dtype=np.int64), deg), (f, size, columns, "device")


# ---- poly_eval -----------------------------------------------------------------------------------------------------------------------
CHUNK = 16  # the forced chunk length of the split route


@pytest.mark.parametrize("f", R.ALL)
def test_poly_eval_routes_equal_the_reference(hip, f):
    from icicle_amd import vecops as V

    p, w = R.modulus(f), R.FIELDS[f]
    rng = np.random.default_rng(3319)
    for m in (1, 2, 63, 64, 65, 257):
        dvals = R.rand_vals(rng, m, p)  # 0, 1, 2, p - 1, (p + 1) / 2, then uniform
        if m == 2:
            dvals = [0, p - 1]
        domain = R.words(dvals, w)
        for n in (1, 2, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5):
            for batch, columns in ((1, False), (3, False), (3, True)):
                cvals = R.rand_vals(rng, n * batch, p)
                if n > 1:
                    for k in range(batch):  # entry 1 (entry 0 of a single polynomial) has a zero leading coefficient
                        if k == min(1, batch - 1):
                            cvals[(n - 1) * batch + k if columns else k * n + n - 1] = 0
                coeffs = R.words(cvals, w)
                want = R.ref_eval(f, coeffs, n, domain, batch, columns)
                if m <= 2 or (m == 65 and n in (1, 65, 3 * CHUNK + 5)):
                    assert R.ints(want, w) == M.poly_eval(p, cvals, n, dvals, batch, columns), (f, m, n, batch, columns)
                for chunk in (-1, CHUNK, 0):
                    got = V.poly_eval(f, coeffs, domain, cfg_of(hip, batch, columns), chunk=chunk)
                    assert got.shape == want.shape and np.array_equal(got, want), (f, m, n, batch, columns, chunk)


@pytest.mark.parametrize("f", R.PER_TYPE)
def test_poly_eval_placement_and_the_plans_own_split(hip, f):
    """5000 coefficients at one and at three points: the plan itself takes the split route (20 chunks of 256, then one chunk); every mix of
    host and device operands; a stream of its own; the argument rules"""
    from icicle_amd import vecops as V
    from icicle_amd.runtime import DeviceVec, Stream

    p, w = R.modulus(f), R.FIELDS[f]
    rng = np.random.default_rng(3323)
    n = 5000
    coeffs = rand_words(rng, n * 3, f)
    domain = R.words([p - 1, 3, (p + 1) // 2], w)
    for batch, columns, m in ((1, False, 1), (3, False, 3), (3, True, 3)):
        c, d = coeffs[:n * batch], domain[:m]
        want = R.ref_eval(f, c, n, d, batch, columns)
        if batch == 1:
            assert R.ints(want, w) == [M.horner(R.ints(c, w), p - 1, p)]
        for chunk in (0, -1, 64, 4096):
            assert np.array_equal(V.poly_eval(f, c, d, cfg_of(hip, batch, columns), chunk=chunk), want), (f, batch, columns, chunk)
        for c_dev in (False, True):
            for d_dev in (False, True):
                for o_dev in (False, True):
                    out = DeviceVec(want.nbytes) if o_dev else np.zeros_like(want)
                    r = V.poly_eval(f, DeviceVec.from_host(c) if c_dev else c, DeviceVec.from_host(d) if d_dev else d, cfg_of(hip, batch, columns), out=out,
                                    coeffs_size=n, domain_size=m)
                    got = r.to_host(shape=want.shape) if o_dev else r
                    assert np.array_equal(got, want), (f, batch, columns, c_dev, d_dev, o_dev)
    st = Stream()
    try:
        cfg = cfg_of(hip, 3, True)
        cfg.stream, cfg.is_async = st.handle, True
        dc, dd, do = DeviceVec.from_host(coeffs), DeviceVec.from_host(domain), DeviceVec(want.nbytes)
        V.poly_eval(f, dc, dd, cfg, out=do, coeffs_size=n, domain_size=3)
        st.synchronize()
        assert np.array_equal(do.to_host(shape=want.shape), want)
    finally:
        st.destroy()
    out = np.full((3, w), 0xA5A5A5A5, np.uint32)
    raises_code(INVALID_ARGUMENT, V.poly_eval, f, coeffs, domain, out=out, chunk=-2)
    raises_code(INVALID_ARGUMENT, V.poly_eval, f, coeffs, domain, out=out, coeffs_size=0)
    raises_code(INVALID_ARGUMENT, V.poly_eval, f, coeffs, domain, out=out, domain_size=0)
    raises_code(INVALID_ARGUMENT, V.poly_eval, f, dc, dd, out=dc.ptr + 4 * w, coeffs_size=n, domain_size=3)  # evals inside coeffs
    assert (out == 0xA5A5A5A5).all()


@pytest.mark.parametrize("f", ["babybear", "bn254"])
def test_poly_eval_one_point_of_a_long_polynomial(hip, f):
    """2^20 + 7 coefficients at one challenge: chunks of 320 coefficients (five Horner steps per lane, the last chunk partial), then one
    chunk of 3277 values; the point route gives the same bytes"""
    from icicle_amd import vecops as V
    from icicle_amd.runtime import DeviceVec

    p, w = R.modulus(f), R.FIELDS[f]
    rng = np.random.default_rng(3329)
    n = (1 << 20) + 7
    coeffs = rand_words(rng, n, f)
    domain = R.words([R.rand_vals(rng, 6, p)[5]], w)
    want = R.ref_eval(f, coeffs, n, domain)
    dc = DeviceVec.from_host(coeffs)
    assert np.array_equal(V.poly_eval(f, dc, domain, coeffs_size=n), want)
    assert np.array_equal(V.poly_eval(f, dc, domain, coeffs_size=n, chunk=-1), want)


@pytest.mark.parametrize("m", [1, 65])
@pytest.mark.parametrize("f", ["babybear", "bn254"])
def test_poly_eval_of_more_polynomials_than_rows_of_blocks(hip, f, m):
    """the point route over GRID_Y_MAX + 4 polynomials of 3 coefficients: blocks of rows 0 to 3 evaluate a second polynomial each, at one
    point (one wave per block) and at 65 (four waves, the last lanes idle)"""
    from icicle_amd import vecops as V

    p, w = R.modulus(f), R.FIELDS[f]
    batch, n = GRID_Y_MAX + 4, 3
    assert batch > GRID_Y_MAX
    rng = np.random.default_rng(3343 + m)
    coeffs = rand_words(rng, n * batch, f)
    domain = rand_words(rng, m, f)
    for columns in (False, True):
        want = R.ref_eval(f, coeffs, n, domain, batch, columns)
        got = V.poly_eval(f, coeffs, domain, cfg_of(hip, batch, columns), chunk=-1)
        assert got.shape == want.shape and np.array_equal(got, want), (f, m, columns)
        ci, di = R.ints(coeffs, w), R.ints(domain, w)
        for k in (0, 3, 4, GRID_Y_MAX - 1, GRID_Y_MAX, batch - 1):  # and without the reference, where the trips meet
            c = ci[k::batch][:n] if columns else ci[k * n:(k + 1) * n]
            for e in (0, m - 1):
                assert R.ints(got[e * batch + k if columns else k * m + e], w) == [M.horner(c, di[e], p)], (f, m, columns, k, e)


# ---- poly_division -------------------------------------------------------------------------------------------------------------------
def tile(f):
    from icicle_amd import vecops as V

    T = V.poly_division_tile(f)
    assert T >= 8
    return T


def check_division(hip, f, nums, dens, q_size=None, r_size=None, columns=False, extra=0):
    """nums / dens: one coefficient list per batch entry (padded here to the longest). Compares the device with the model, with the
    reference (once per entry at batch_size == 1 where it is defined; the whole batch too for columns with r_size == numerator_size) and
    q * b + r == numerator in integers. Returns (q, r) as lists per entry."""
    from icicle_amd import vecops as V

    p, w = R.modulus(f), R.FIELDS[f]
    batch = len(nums)
    ns, bs = max(len(x) for x in nums), max(len(x) for x in dens)
    nums, dens = [x + [0] * (ns - len(x)) for x in nums], [x + [0] * (bs - len(x)) for x in dens]
    need_q = max([M.degree(n) - M.degree(d) + 1 for n, d in zip(nums, dens)] + [1])
    q_size = (need_q if q_size is None else q_size) + extra
    r_size = (ns if r_size is None else r_size) + extra
    num, den = M.pack(nums, columns), M.pack(dens, columns)
    a, b = R.words(num, w), R.words(den, w)
    want_q, want_r = M.poly_division(p, num, ns, den, bs, q_size, r_size, batch, columns)
    q, r = V.poly_division(f, a, b, cfg_of(hip, batch, columns), q_size=q_size, r_size=r_size)
    assert q.shape == (q_size * batch, w) and r.shape == (r_size * batch, w)
    assert (R.ints(q, w), R.ints(r, w)) == (want_q, want_r), (f, batch, columns, ns, bs, q_size, r_size)
    qs, rs = [M.entry(want_q, k, q_size, batch, columns) for k in range(batch)], [M.entry(want_r, k, r_size, batch, columns) for k in range(batch)]
    for k in range(batch):
        if R.ref_division_defined(nums[k], dens[k]):
            rq, rr = R.ref_division(f, R.words(nums[k], w), ns, R.words(dens[k], w), bs, q_size, r_size)
            assert (R.ints(rq, w), R.ints(rr, w)) == (qs[k], rs[k]), (f, "reference, entry", k)
        back = M.poly_mul(p, qs[k], dens[k]) + [0] * (ns + r_size)
        assert [(x + y) % p for x, y in zip(back, rs[k] + [0] * len(back))][:ns] == nums[k] and not any(back[ns:]), (f, "q b + r", k)
        assert M.degree(rs[k]) < max(M.degree(dens[k]), M.degree(nums[k]) + 1)
    if batch > 1 and columns and r_size == ns and all(R.ref_division_defined(n, d) for n, d in zip(nums, dens)):
        rq, rr = R.ref_division(f, a, ns, b, bs, q_size, r_size, batch, True)
        assert np.array_equal(rq, q) and np.array_equal(rr, r), (f, "reference, columns batch")
    return qs, rs


@pytest.mark.parametrize("f", R.PER_TYPE)
def test_poly_division_around_the_tile(hip, f):
    p, T = R.modulus(f), tile(f)
    rng = np.random.default_rng(3331)
    for nq in (1, T - 1, T, T + 1, 2 * T + 3):
        for db in (0, 1, T - 1, T, T + 1):
            num, den = R.rand_vals(rng, db + nq, p, nonzero=True), R.rand_vals(rng, db + 1, p, nonzero=True)  # a non-monic denominator
            if db == 0:
                num[0] = 0  # keeps the reference defined; a non-zero constant term is in test_poly_division_directed
            check_division(hip, f, [num], [den])


@pytest.mark.parametrize("f", R.ALL)
def test_poly_division_directed(hip, f):
    from icicle_amd import vecops as V
    from icicle_amd.runtime import DeviceVec

    p, w, T = R.modulus(f), R.FIELDS[f], tile(f)
    rng = np.random.default_rng(3337)
    den = R.rand_vals(rng, 12, p, nonzero=True)
    # a numerator shorter than the denominator, by one and by more (the reference is not defined for the latter), and a zero numerator
    for num in (R.rand_vals(rng, 11, p, nonzero=True), R.rand_vals(rng, 4, p, nonzero=True), [0] * 9):
        qs, rs = check_division(hip, f, [num], [den], extra=2)
        assert not any(qs[0]) and rs[0][:len(num)] == num
    # a constant denominator under a numerator with a non-zero constant term (not defined in the reference either)
    check_division(hip, f, [R.rand_vals(rng, T + 9, p, nonzero=True)], [[p - 2]])
    # buffers longer than the degrees, and q_size / r_size larger than needed
    num = R.rand_vals(rng, T + 50, p, nonzero=True)
    check_division(hip, f, [num + [0] * 7], [den + [0] * 5], extra=6)
    # an exact product whose quotient has runs of zeros, one of them across the boundary of the top tile (quotient index nq - 1 - T)
    nq = T + 40
    q = R.rand_vals(rng, nq, p, nonzero=True)
    for lo, hi in ((nq - 1 - T - 3, nq - 1 - T + 4), (5, 9), (nq - 9, nq - 2), (0, 2)):
        q[lo:hi] = [0] * (hi - lo)
    qs, rs = check_division(hip, f, [M.poly_mul(p, q, den)], [den])
    assert qs[0] == q and not any(rs[0])
    # batch 3 with a different degree per entry, rows and columns, the outputs larger than needed and not
    nums = [R.rand_vals(rng, 2 * T + 20, p, nonzero=True), R.rand_vals(rng, 30, p, nonzero=True), R.rand_vals(rng, T + 3, p, nonzero=True)]
    dens = [R.rand_vals(rng, 40, p, nonzero=True), R.rand_vals(rng, 7, p, nonzero=True), R.rand_vals(rng, T + 1, p, nonzero=True)]
    for columns in (False, True):
        for extra in (0, 5):
            check_division(hip, f, nums, dens, columns=columns, extra=extra)
    # device operands, device results
    ns, bs = len(nums[0]), len(dens[0])
    a, b = R.words(nums[0], w), R.words(dens[0], w)
    want_q, want_r = V.poly_division(f, a, b)
    assert want_q.shape == (ns - bs + 1, w) and want_r.shape == (ns, w)
    for a_dev, b_dev, o_dev in ((True, True, True), (True, False, False), (False, True, True)):
        qo, ro = (DeviceVec(want_q.nbytes), DeviceVec(want_r.nbytes)) if o_dev else (None, None)
        q, r = V.poly_division(f, DeviceVec.from_host(a) if a_dev else a, DeviceVec.from_host(b) if b_dev else b, q_out=qo, r_out=ro, num_size=ns, den_size=bs,
                               q_size=ns - bs + 1, r_size=ns)
        if o_dev:
            q, r = q.to_host(shape=want_q.shape), r.to_host(shape=want_r.shape)
        assert np.array_equal(q, want_q) and np.array_equal(r, want_r), (f, a_dev, b_dev, o_dev)
    # the argument rules: a zero denominator in entry 1 of 3, a q_size and an r_size one too small; nothing is written
    flat_n, flat_d = R.words(M.pack([x + [0] * (ns - len(x)) for x in nums], False), w), M.pack([x + [0] * (T + 1 - len(x)) for x in dens], False)
    zero_d = list(flat_d)
    zero_d[T + 1:2 * (T + 1)] = [0] * (T + 1)
    need_q = max(M.degree(n) - M.degree(d) + 1 for n, d in zip(nums, dens))
    for dvals, q_size, r_size in ((zero_d, need_q, ns), (flat_d, need_q - 1, ns), (flat_d, need_q, ns - 1)):
        qo, ro = np.full((q_size * 3, w), 0xA5A5A5A5, np.uint32), np.full((r_size * 3, w), 0xA5A5A5A5, np.uint32)
        raises_code(INVALID_ARGUMENT, V.poly_division, f, flat_n, R.words(dvals, w), cfg_of(hip, 3), q_size=q_size, r_size=r_size, q_out=qo, r_out=ro)
        assert (qo == 0xA5A5A5A5).all() and (ro == 0xA5A5A5A5).all()
    dn = DeviceVec.from_host(a)
    raises_code(INVALID_ARGUMENT, V.poly_division, f, dn, b, q_out=DeviceVec(want_q.nbytes), r_out=dn.ptr + 4 * w, num_size=ns - 1, q_size=ns - bs + 1, r_size=ns - 1)
