"""GPU: interleaved transforms (columns_batch batches, the quartic extension field) of 2^25 .. 2^27 points, BabyBear.

Lane-native tiles (ntt_fast.hpp LN) take their launch geometry from the length of each pass (ntt_plan.h fast_pass_geometry), and
passes of 512 rows -- tiles of 16 word-columns, slices of 16 transforms -- exist only from 2^25 up: 8,9,8 at 2^25, 9,9,8 at 2^26,
9,9,9 at 2^27. The cases are chosen for the branch each reaches:
  * 16 / 32 / 64 columns: column groups (cg = 8 / 4 / 2) in pass 0 and the last pass, outer-index groups (ag) in the middle one;
  * 48 columns (and 12 extension columns, the same 48 words): the padded work buffer (rows of 64 words) together with groups --
    the group strides were built from the caller's 48-word stride on the work buffer's side until the plan check found it;
  * 33 and 100 columns: padded work buffer with a ragged last slice, no groups;
  * extension rows (ltot = 4), 1 and 3 of them: several row groups;
  * kNR (bit-reversed store, cst_out = 0), kRN (consumed natively, groups in every pass), kRR (reordering pre-pass), cosets.
Every case is compared exactly with (a) the row-major batched transform of the same columns gathered into rows -- ALL columns,
8 at a time --, (b) a plain direct DFT in numpy at sampled (lane, k), and once (c) the reference CPU backend; every kNN case
also runs the inverse round trip. Inputs are a hash of the word index, so any column can be regenerated on the device without
a copy of the input (the 2^27 x 48 case runs in place: 24 GiB plus the 32 GiB padded work buffer).
"""
import numpy as np
import pytest

from oracle import pyref

pytestmark = pytest.mark.gpu

F = pyref.BABYBEAR
FNAME = "babybear"
kNN, kNR, kRN, kRR = 0, 1, 2, 3
COSET = 31
CHUNK = 1 << 22  # rows per generator step (bounded int64 temporaries)


def _hash(idx, seed):
    """field elements (int32 tensor of values < p) from int64 word indices < 2^33; no product leaves int64"""
    import torch

    h = (idx * 0x2545F491 + seed) & 0xFFFFFFFF
    h = h ^ (h >> 16)
    h = (h * 0x45D9F3B) & 0xFFFFFFFF
    h = h ^ (h >> 16)
    return (h % F.p).to(torch.int32)


class Layout:
    """the buffer of one case as word columns q = 0 .. W-1, each a transform of n points: columns_batch (n, W), W = batch * lanes;
    row-major extension rows (R, n, 4), q = 4 r + coordinate"""

    def __init__(self, logn, batch, ext, columns):
        self.logn, self.n, self.batch, self.ext, self.columns = logn, 1 << logn, batch, ext, columns
        self.W = batch * (4 if ext else 1)
        self.shape = (self.n, self.W) if columns else (batch, self.n, 4)

    def col(self, t, q):
        return t[:, q] if self.columns else t[q // 4, :, q % 4]

    def base_stride(self, q):  # flat word index of element j of column q = base + j * stride
        return (q, self.W) if self.columns else ((q // 4) * self.n * 4 + q % 4, 4)

    def fill(self, t, seed):
        import torch

        flat = t.view(-1)
        for i0 in range(0, flat.numel(), CHUNK * 8):
            i1 = min(flat.numel(), i0 + CHUNK * 8)
            flat[i0:i1] = _hash(torch.arange(i0, i1, device=t.device, dtype=torch.int64), seed)

    def gen_cols(self, qs, seed, dev):
        """the input's columns qs as contiguous rows (len(qs), n), regenerated"""
        import torch

        out = torch.empty((len(qs), self.n), dtype=torch.int32, device=dev)
        for i, q in enumerate(qs):
            b, s = self.base_stride(q)
            for j0 in range(0, self.n, CHUNK):
                j = torch.arange(j0, min(self.n, j0 + CHUNK), device=dev, dtype=torch.int64)
                out[i, j0 : j0 + len(j)] = _hash(b + j * s, seed)
        return out

    def cfg(self, hip, ordering, coset):
        c = hip.NTTConfigU32.default()
        c.batch_size, c.columns_batch, c.is_async, c.ordering, c.coset_gen = self.batch, self.columns, True, ordering, coset
        return c


def _ntt(hip, lay, src, dst, direction, ordering, coset):
    from icicle_amd import ntt as N

    N.ntt(FNAME, src.data_ptr(), direction, lay.cfg(hip, ordering, coset), out=dst.data_ptr(), size=lay.n, extension=lay.ext)


def _rowmajor(hip, rows, direction, ordering, coset):
    """the oracle of (a): the row-major batched base-field transform (byte-compared with the reference at 2^25 and 2^27 and with
    the four-step identity at 2^25 .. 2^27, test_gpu_ntt_fullsize.py); an extension coordinate is a base-field transform of its own
    (twiddles and the coset generator are base-field elements)"""
    import torch
    from icicle_amd import ntt as N

    out = torch.empty_like(rows)
    c = hip.NTTConfigU32.default()
    c.batch_size, c.is_async, c.ordering, c.coset_gen = rows.shape[0], True, ordering, coset
    N.ntt(FNAME, rows.data_ptr(), direction, c, out=out.data_ptr(), size=rows.shape[1])
    return out


def _check_vs_rowmajor(hip, lay, y, seed, direction, ordering, coset, what):
    import torch

    for q0 in range(0, lay.W, 8):
        qs = list(range(q0, min(lay.W, q0 + 8)))
        exp = _rowmajor(hip, lay.gen_cols(qs, seed, y.device), direction, ordering, coset)
        got = torch.stack([lay.col(y, q) for q in qs])
        torch.cuda.synchronize()
        if not torch.equal(got, exp):
            bad = [q for i, q in enumerate(qs) if not torch.equal(got[i], exp[i])]
            raise AssertionError(f"{what}: columns {bad} differ from the row-major transform of the same columns")
        del exp, got


def _bitrev_idx(logn, dev):
    import torch

    i = torch.arange(1 << logn, device=dev, dtype=torch.int64)
    r = torch.zeros_like(i)
    for b in range(logn):
        r |= ((i >> b) & 1) << (logn - 1 - b)
    return r


def _powers(r, n):
    """r^0 .. r^(n-1) mod p, uint64, built by doubling"""
    p = np.uint64(F.p)
    t = np.empty(n, dtype=np.uint64)
    t[0] = 1
    m, rm = 1, r % F.p
    while m < n:
        np.multiply(t[:m], np.uint64(rm), out=t[m : 2 * m])
        np.remainder(t[m : 2 * m], p, out=t[m : 2 * m])
        m, rm = 2 * m, rm * rm % F.p
    return t


def _dft_samples(x_cols, logn, ks, direction, coset):
    """direct DFT of logical inputs x_cols (list of uint64 arrays) at outputs ks: X_k = sum_j x_j g^j w^(jk) (forward),
    x_k = n^-1 g^-k sum_j X_j w^(-jk) (inverse); reduced per term, one power table per k"""
    n, p = 1 << logn, F.p
    w = pyref.omega(F, logn)
    res = {}
    for k in ks:
        if direction == 0:
            t = _powers(coset * pow(w, k, p) % p, n)
            scale = 1
        else:
            t = _powers(pow(w, (n - k) % n, p), n)
            scale = pow(n, p - 2, p) * pow(pow(coset, k, p), p - 2, p) % p
        for i, x in enumerate(x_cols):
            s = int(np.remainder(x * t, np.uint64(p)).sum(dtype=np.uint64)) % p
            res[(i, k)] = s * scale % p
        del t
    return res


def _check_dft(lay, y, seed, direction, ordering, coset, lanes, ks, what):
    import torch

    dev = y.device
    cols = lay.gen_cols(lanes, seed, dev)
    if ordering in (kRN, kRR):  # memory index bitrev(j) holds logical x_j
        cols = cols[:, _bitrev_idx(lay.logn, dev)]
    x_cols = [cols[i].cpu().numpy().astype(np.uint64) for i in range(len(lanes))]
    del cols
    exp = _dft_samples(x_cols, lay.logn, ks, direction, coset)
    for i, q in enumerate(lanes):
        for k in ks:
            kk = pyref.bitrev(k, lay.logn) if ordering in (kNR, kRR) else k
            got = int(lay.col(y, q)[kk].item())
            assert got == exp[(i, k)], f"{what}: lane {q}, X[{k}] = {got}, direct DFT {exp[(i, k)]}"


def _samples(lay, seed):
    """(lanes, ks): lanes from the first and the last slice (and column group), k = 0, n - 1 and seeded ones in both halves;
    2^27: two k per case (a direct DFT of 2^27 terms costs 1-2 s)"""
    n, W = lay.n, lay.W
    rng = np.random.default_rng(seed)
    lanes = sorted({0, W - 1, int(rng.integers(0, W))})
    lo, hi = int(rng.integers(1, n // 2)), int(rng.integers(n // 2, n - 1))
    ks = [n - 1, hi] if lay.logn >= 27 else [0, n - 1, lo, hi]
    if lay.logn >= 27:
        lanes = [0, W - 1]
    return lanes, ks


@pytest.fixture(scope="module")
def domain27(hip):
    """BabyBear's whole domain, 2^27 (the module owns it, as test_gpu_ntt_fullsize.py does at its sizes)"""
    from icicle_amd import ntt as N

    N.init_domain(FNAME, N.get_root_of_unity(FNAME, 1 << 27))
    yield
    N.release_domain(FNAME)


# (logn, batch, extension, columns_batch)
KNN_CASES = (
    [(lg, b, False, True) for lg in (25, 26) for b in (16, 32, 64)]  # cg 8 / 4 / 2, no padding
    + [(lg, 48, False, True) for lg in (25, 26, 27)]  # padding + groups
    + [(lg, 12, True, True) for lg in (25, 26, 27)]  # the same through the extension entry point
    + [(25, 33, False, True), (25, 100, False, True)]  # padding, ragged last slice, no groups
    + [(lg, b, True, False) for lg in (25, 27) for b in (1, 3)]  # extension rows: ltot = 4, row groups
)


def _id(c):
    lg, b, ext, cols = c
    return f"2^{lg}-{'ext' if ext else 'base'}-{'cols' if cols else 'rows'}{b}"


@pytest.mark.parametrize("case", KNN_CASES, ids=[_id(c) for c in KNN_CASES])
def test_interleaved_knn_big(hip, domain27, case):
    """forward kNN against the row-major transform of every column and a direct DFT at sampled outputs; the inverse round trip"""
    import torch
    from icicle_amd import ntt as N

    logn, batch, ext, columns = case
    lay = Layout(logn, batch, ext, columns)
    seed = 7919 * logn + 31 * lay.W + (1 if ext else 0) + (0 if columns else 2)
    dev = torch.device("cuda", 0)
    in_place = lay.n * lay.W * 4 > (16 << 30)  # 2^27 x 48: 24 GiB per buffer plus the 32 GiB work buffer
    what = f"{_id(case)} forward kNN"
    x = torch.empty(lay.shape, dtype=torch.int32, device=dev)
    lay.fill(x, seed)
    y = x if in_place else torch.empty_like(x)
    try:
        _ntt(hip, lay, x, y, N.FORWARD, kNN, 1)
        torch.cuda.synchronize()
        _check_vs_rowmajor(hip, lay, y, seed, N.FORWARD, kNN, 1, what)
        lanes, ks = _samples(lay, seed)
        _check_dft(lay, y, seed, N.FORWARD, kNN, 1, lanes, ks, what)
        _ntt(hip, lay, y, y, N.INVERSE, kNN, 1)  # in place
        torch.cuda.synchronize()
        if in_place:
            for q0 in range(0, lay.W, 8):
                qs = list(range(q0, min(lay.W, q0 + 8)))
                assert torch.equal(torch.stack([lay.col(y, q) for q in qs]), lay.gen_cols(qs, seed, dev)), f"{_id(case)}: inverse(forward(x)) != x, columns {qs}"
        else:
            assert torch.equal(y, x), f"{_id(case)}: inverse(forward(x)) != x"
    finally:
        del x, y
        torch.cuda.empty_cache()


# 2^25, 48 and 32 columns: (ordering, direction, coset)
ORDER_CASES = [(b, o, d, c) for b in (48, 32) for (o, d, c) in ((kNR, 0, 1), (kRN, 0, 1), (kRR, 0, 1), (kNN, 0, COSET), (kNN, 1, COSET))]
_ONAME = {kNN: "kNN", kNR: "kNR", kRN: "kRN", kRR: "kRR"}


def _oid(c):
    b, o, d, cs = c
    return f"2^25-cols{b}-{_ONAME[o]}-{'inv' if d else 'fwd'}{'-coset' if cs != 1 else ''}"


@pytest.mark.parametrize("case", ORDER_CASES, ids=[_oid(c) for c in ORDER_CASES])
def test_interleaved_orderings_and_cosets_2_25(hip, domain27, case):
    """bit-reversed store (kNR), bit-reversed input consumed natively (kRN) and through the reordering pre-pass (kRR), coset
    factors in pass 0 (forward) or the last pass (inverse), on 48 (padded work buffer) and 32 columns; kNR is also run back with
    the kRN inverse"""
    import torch
    from icicle_amd import ntt as N

    batch, ordering, direction, coset = case
    lay = Layout(25, batch, False, True)
    seed = 104729 + 97 * batch + 13 * ordering + 5 * direction + (coset != 1)
    dev = torch.device("cuda", 0)
    what = _oid(case)
    x = torch.empty(lay.shape, dtype=torch.int32, device=dev)
    lay.fill(x, seed)
    y = torch.empty_like(x)
    try:
        _ntt(hip, lay, x, y, direction, ordering, coset)
        torch.cuda.synchronize()
        _check_vs_rowmajor(hip, lay, y, seed, direction, ordering, coset, what)
        lanes, ks = _samples(lay, seed)
        _check_dft(lay, y, seed, direction, ordering, coset, lanes, ks[1::2], what)  # k = n - 1 and a seeded one
        if ordering == kNR:  # the polynomial-product pattern: kNR forward, kRN inverse
            _ntt(hip, lay, y, y, N.INVERSE, kRN, 1)
            torch.cuda.synchronize()
            assert torch.equal(y, x), f"{what}: kRN inverse of the kNR forward output != x"
    finally:
        del x, y
        torch.cuda.empty_cache()


# (c) the reference CPU backend, once: 8 of the 48 columns at 2^25 (both slices, several column groups), as a row-major batch
REF_LAY = (25, 48, False, True)
REF_COLS = [0, 5, 16, 31, 32, 40, 46, 47]
REF_SEED = 2025


def _job_ref48(pool, hip, dev):
    lay = Layout(*REF_LAY)
    rows = lay.gen_cols(REF_COLS, REF_SEED, dev)
    pool.submit_ntt("lanes48_fwd_25", FNAME, rows.cpu().numpy().view(np.uint32).reshape(-1), 25, 0, batch=len(REF_COLS), lane="ntt_c")


@pytest.mark.refjob("lanes48_fwd_25", order=40)
def test_interleaved_48_columns_2_25_vs_oracle(hip, domain27, refpool):
    """2^25 x 48 columns forward kNN (padded work buffer plus column / outer-index groups): 8 columns byte-compared with the
    reference CPU backend's row-major transform of the same columns (1 GiB)"""
    import torch
    from icicle_amd import ntt as N

    lay = Layout(*REF_LAY)
    dev = torch.device("cuda", 0)
    x = torch.empty(lay.shape, dtype=torch.int32, device=dev)
    lay.fill(x, REF_SEED)
    y = torch.empty_like(x)
    _ntt(hip, lay, x, y, N.FORWARD, kNN, 1)
    torch.cuda.synchronize()
    del x
    got = torch.stack([lay.col(y, q) for q in REF_COLS]).cpu().numpy().view(np.uint32).reshape(-1)
    del y
    torch.cuda.empty_cache()
    assert np.array_equal(got, refpool.result("lanes48_fwd_25")), "2^25 x 48 columns forward: differs from the reference CPU backend"
    refpool.drop("lanes48_fwd_25")


REF_JOBS = {"lanes48_fwd_25": (25, _job_ref48)}
