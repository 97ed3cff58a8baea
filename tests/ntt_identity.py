"""A full-output check of ONE transform of the 256-bit / Goldilocks NTT (icicle_amd/csrc/ntt_big.hip) that runs on the device and
shares no code with that kernel.

For a forward transform X[k] = sum_j x_j (g w^k)^j with coset generator g (1 without a coset), and any r with r^n != 1:

    sum_k r^k X[k]  =  (1 - r^n) * sum_j x_j g^j / (1 - r w^j)

(sum_k (r w^j)^k is a geometric series). The left side is the polynomial with coefficients X at the point r: one wrong output element
changes it unless r is a root of a fixed non-zero polynomial of degree < n, probability <= n / p. An inverse transform y = INTT(X) is
checked with the roles swapped, check(x=y, X=X): X is the forward (coset) transform of y.

Both sides are computed with the project's own device calls on device addresses (icicle_amd/vecops.py), each kept inside the size at which
the suite compares it with the reference or with Python integers:
  * poly_eval at one point: 2^20 + 7 coefficients (tests/test_gpu_poly.py test_poly_eval_one_point_of_a_long_polynomial) -> rows of
    ROW = 2^20 coefficients with batch_size = n / 2^20; the partial values P_c(r) are combined on the host, sum_c r^(c ROW) P_c(r).
  * vector_sum: 2^20 elements, and 4 rows of 2^18 (tests/test_gpu_vecops_inv.py test_reductions_beyond_one_block_of_partials) -> the same
    rows of 2^20, added on the host.
  * vector_inv: a * inv(a) = 1 at 2^16 elements (test_gpu_vecops_inv.py test_round_trip_at_size; against the reference only up to
    2 T + 3 elements, T = vector_inv_tile) -> slices of INV_SLICE = 2^16 elements.
  * scalar_mul_vec, scalar_sub_vec, vector_mul: against the reference up to 2^14 x 2 elements (tests/test_gpu_vecops.py) -> slices of at most
    SLICE = 2^20 elements, by pointer arithmetic. In place only where that test is: vector_mul with out = b, vector_inv with out = a.
A defect in one of these primitives makes the identity fail; it cannot make a wrong transform pass.

The identity alone would accept X[k] + p, so every output word is also compared with the modulus (canonical()).

Vectors are torch int32 tensors of shape [n, words] on the device (little-endian u32 words reinterpreted), nothing of size n crosses to
the host."""
import random

import numpy as np

ROW = 1 << 20        # poly_eval / vector_sum: elements per batch entry
SLICE = 1 << 20      # element-wise calls
INV_SLICE = 1 << 16  # vector_inv
SIGN = -(1 << 31)    # x ^ SIGN orders int32 words like the unsigned words they hold

WORDS = {"bn254": 8, "bls12_381": 8, "bls12_377": 8, "stark252": 8, "goldilocks": 2}


def to_words(v: int, w: int) -> np.ndarray:
    return np.array([[(v >> (32 * i)) & 0xFFFFFFFF for i in range(w)]], dtype=np.uint32)


def from_words(row) -> int:
    return sum((int(x) & 0xFFFFFFFF) << (32 * i) for i, x in enumerate(np.asarray(row).reshape(-1)))


def challenge(p: int, n: int, seed: int) -> int:
    """a seeded r in [2, p) with r^n != 1 -- then 1 - r w^j != 0 for every j, w^j being an n-th root of unity"""
    r = random.Random(seed).randrange(2, p)
    assert pow(r, n, p) != 1, "r lies in the transform's domain: take another seed"
    return r


def split_logn(logn: int, smax: int = 8):
    """pass lengths, as ntt_plan.h split_logn gives them to ntt_big.hip: the digits of an output index in the failure message"""
    big = max(smax, (logn + 2) // 3)
    P = max(1, (logn + big - 1) // big)
    return [logn // P + (1 if i < logn % P else 0) for i in range(P)]


# ---- the host's share: combining at most n / ROW partial values in Python integers -------------------------------------------------------
def combine_lhs(parts, r: int, row: int, p: int) -> int:
    """sum_c r^(c row) P_c(r) from the values P_c(r) of the rows"""
    step, acc, f = pow(r, row, p), 0, 1
    for v in parts:
        acc = (acc + f * v) % p
        f = f * step % p
    return acc


def combine_rhs(parts, r: int, n: int, p: int) -> int:
    """(1 - r^n) * the sum of the rows' sums"""
    return (1 - pow(r, n, p)) * (sum(parts) % p) % p


def python_sides(p: int, w_n: int, x, X, r: int, g: int = 1, row: int = None):
    """both sides in Python integers, through the same row split and combine functions as the device path: (left, right)"""
    n = len(x)
    row = min(row or n, n)
    assert n % row == 0
    lhs_parts = [sum(X[c + k] * pow(r, k, p) for k in range(row)) % p for c in range(0, n, row)]
    terms = [x[j] * pow(g, j, p) * pow((1 - r * pow(w_n, j, p)) % p, -1, p) % p for j in range(n)]
    rhs_parts = [sum(terms[c:c + row]) % p for c in range(0, n, row)]
    return combine_lhs(lhs_parts, r, row, p), combine_rhs(rhs_parts, r, n, p)


# ---- device helpers ----------------------------------------------------------------------------------------------------------------------
def _cfg(batch=1):
    from icicle_amd import VecOpsConfig

    cfg = VecOpsConfig.default()
    cfg.batch_size = batch
    return cfg


def _slices(n: int, limit: int):
    for off in range(0, n, limit):
        yield off, min(limit, n - off)


def random_elements(field: str, p: int, n: int, gen, dev):
    """n canonical elements as [n, words] int32 on the device: random words, the top word reduced below the modulus' top word"""
    import torch

    w = WORDS[field]
    x = torch.randint(0, 256, (n, 4 * w), dtype=torch.uint8, generator=gen, device=dev).view(torch.int32)
    top = torch.randint(0, p >> (32 * (w - 1)), (n,), dtype=torch.int64, generator=gen, device=dev)
    x[:, w - 1] = ((top + (1 << 31)) % (1 << 32) - (1 << 31)).to(torch.int32)
    return x


def element_tensor(v: int, w: int, dev):
    """one element as a [words] int32 tensor on the device"""
    import torch

    return torch.from_numpy(to_words(v, w).view(np.int32).reshape(-1).copy()).to(dev)


def progression(field: str, p: int, n: int, first: int, base: int, dev):
    """v_j = first * base^j, j < n (n a power of two), by doubling: v[m:2m] = base^m * v[0:m] with scalar_mul_vec"""
    import torch
    from icicle_amd import vecops as V

    w = WORDS[field]
    eb = 4 * w
    v = torch.empty((n, w), dtype=torch.int32, device=dev)
    v[0] = element_tensor(first % p, w, dev)
    m = 1
    while m < n:
        s = to_words(pow(base, m, p), w)
        for off, cnt in _slices(m, SLICE):
            V.scalar_mul_vec(field, s, v.data_ptr() + off * eb, _cfg(), out=v.data_ptr() + (m + off) * eb, size=cnt)
        m *= 2
    return v


def canonical(X, p: int) -> bool:
    """every element of X ([n, words] int32) is below p: lexicographic word comparison, top word first"""
    import torch

    n, w = X.shape
    for lo in range(0, n, 1 << 24):
        part = X[lo:lo + (1 << 24)]
        lt = torch.zeros(part.shape[0], dtype=torch.bool, device=X.device)
        eq = torch.ones(part.shape[0], dtype=torch.bool, device=X.device)
        for i in reversed(range(w)):
            pw = ((p >> (32 * i)) & 0xFFFFFFFF) - (1 << 31)  # the modulus' word, mapped like col below
            col = part[:, i] ^ SIGN
            lt |= eq & (col < pw)
            eq &= col == pw
        if not bool(lt.all()):
            return False
    return True


class Checker:
    """1 / (1 - r w^j) for one (field, logn, seed), built once and shared by the checks of a case; release() frees it."""

    def __init__(self, field: str, F, logn: int, seed: int, dev):
        import torch
        from icicle_amd import ntt as N, vecops as V
        from oracle import pyref

        self.field, self.p, self.logn, self.n, self.dev = field, F.p, logn, 1 << logn, dev
        self.w = WORDS[field]
        self.omega = N.get_root_of_unity_from_domain(field, logn)
        assert self.omega == pyref.omega(F, logn)
        self.r = challenge(self.p, self.n, seed)
        eb, n = 4 * self.w, self.n
        u = progression(field, self.p, n, self.r, self.omega, dev)  # u_j = r w^j
        d = torch.empty_like(u)
        one = to_words(1, self.w)
        for off, cnt in _slices(n, SLICE):
            V.scalar_sub_vec(field, one, u.data_ptr() + off * eb, _cfg(), out=d.data_ptr() + off * eb, size=cnt)
        del u
        for off, cnt in _slices(n, INV_SLICE):
            V.vector_inv(field, d.data_ptr() + off * eb, _cfg(), out=d.data_ptr() + off * eb, size=cnt)
        self.d = d

    def release(self):
        self.d = None

    def _rows(self):
        row = min(ROW, self.n)
        return self.n // row, row

    def sides(self, x, X, g: int = 1):
        """(left, right) of the identity for x, X: [n, words] int32 on the device, contiguous"""
        import torch
        from icicle_amd import vecops as V

        f, p, n, w = self.field, self.p, self.n, self.w
        eb = 4 * w
        assert x.shape == X.shape == (n, w) and x.is_contiguous() and X.is_contiguous()
        rows, row = self._rows()
        t = torch.empty_like(x)
        for off, cnt in _slices(n, SLICE):
            V.vector_mul(f, x.data_ptr() + off * eb, self.d.data_ptr() + off * eb, _cfg(), out=t.data_ptr() + off * eb, size=cnt)
        if g != 1:
            c = progression(f, p, n, 1, g, self.dev)  # c_j = g^j
            for off, cnt in _slices(n, SLICE):
                V.vector_mul(f, c.data_ptr() + off * eb, t.data_ptr() + off * eb, _cfg(), out=t.data_ptr() + off * eb, size=cnt)
            del c
        sums = V.vector_sum(f, t.data_ptr(), _cfg(rows), size=row)
        del t
        rhs = combine_rhs([from_words(s) for s in sums], self.r, n, p)
        vals = V.poly_eval(f, X.data_ptr(), to_words(self.r, w), _cfg(rows), coeffs_size=row)
        lhs = combine_lhs([from_words(v) for v in vals], self.r, row, p)
        return lhs, rhs

    def evaluate(self, x, points):
        """P_x(z) for every z of points, by the same rows of poly_eval: the definition of single outputs, for the failure message"""
        from icicle_amd import vecops as V

        rows, row = self._rows()
        dom = np.concatenate([to_words(z, self.w) for z in points])
        vals = V.poly_eval(self.field, x.data_ptr(), dom, _cfg(rows), coeffs_size=row).reshape(rows, len(points), self.w)
        return [combine_lhs([from_words(vals[c, e]) for c in range(rows)], z, row, self.p) for e, z in enumerate(points)]

    def triage(self, x, X, g: int = 1) -> str:
        """outputs whose digits (k0, k1, k2) of k = k0 + n0 k1 + n0 n1 k2 are 0, 1 or the largest, evaluated directly: the first wrong one"""
        parts = split_logn(self.logn)
        digs = [sorted({0, 1, (1 << s) - 1} & set(range(1 << s))) for s in parts]
        digs += [[0]] * (3 - len(parts))
        shifts = [0, parts[0], parts[0] + (parts[1] if len(parts) > 1 else 0)]
        cand = sorted({(k0 << shifts[0]) + (k1 << shifts[1]) + (k2 << shifts[2]) for k0 in digs[0] for k1 in digs[1] for k2 in digs[2]})
        want = self.evaluate(x, [g * pow(self.omega, k, self.p) % self.p for k in cand])
        got = [from_words(X[k].cpu().numpy()) for k in cand]
        for k, a, b in zip(cand, got, want):
            if a != b:
                ds = tuple((k >> shifts[i]) & ((1 << parts[i]) - 1) if i < len(parts) else 0 for i in range(3))
                return f"first wrong sampled output: k = {k}, digits (k0, k1, k2) = {ds} of passes {parts}: got {a:#x}, want {b:#x}"
        return f"the {len(cand)} sampled outputs (digits 0, 1, max of passes {parts}) are right"

    def accepts(self, x, X, g: int = 1) -> bool:
        lhs, rhs = self.sides(x, X, g)
        return lhs == rhs and canonical(X, self.p)

    def check(self, x, X, g: int = 1, what=""):
        """assert that X is the forward (coset g) transform of x, on every output element, and that X is canonical"""
        assert canonical(X, self.p), f"{self.field} 2^{self.logn} {what}: an output element is not below the modulus"
        lhs, rhs = self.sides(x, X, g)
        if lhs != rhs:
            raise AssertionError(f"{self.field} 2^{self.logn} {what}: sum_k r^k X[k] = {lhs:#x}, (1 - r^n) sum_j x_j g^j / (1 - r w^j) = {rhs:#x}; " + self.triage(x, X, g))
