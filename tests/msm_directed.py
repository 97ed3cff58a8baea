"""Directed MSM inputs and their oracle, shared by the MSM test modules (host-side only: nothing here needs a GPU or the product library).

1. The input builders of the bucket-reduction tests (in_*): each takes (r, bases_fn, neg_fn) -- the scalar modulus, bases_fn(n, period=1024)
   giving n base rows, neg_fn(rows) giving the rows of the negated points -- and returns (scalars as Python integers, base rows).
2. in_overflow: chosen buckets of window 0 with chosen sizes, for the overflow-segment path (k_plan_overflow, the overflow threads of
   k_accumulate, k_fold_overflow).
3. A model of the signed window recoding (msm_impl.hpp DigitIter, WinWidths, negate_scalar_if_top_bit) that turns scalars into bucket counts.
4. The seven groups (GROUPS, Group) with what the launch decisions read of them (point sizes -> ReduceWindowLanes, QUAD_OK), and the closed-form
   oracle: the bases are (k0 + i) G, a negated row counts as -(k0 + i), a zero row as nothing, so an MSM is ((sum s_i k_i) mod r) G -- one
   scalar multiplication on Python integers, which shares no code with the kernels or with the reference backend."""
import collections

import numpy as np

from oracle import pyref
from tests.util import rand_scalars, to_words


def _plan_widths(bits, nwin):
    """(offset, width) of the windows of a forced mixed plan: the top x windows one bit wider (msm_plan.h make_plan)"""
    clo, x = bits // nwin, bits - (bits // nwin) * nwin
    out, off = [], 0
    for w in range(nwin):
        width = clo if w < nwin - x else clo + 1
        out.append((off, width))
        off += width
    assert off == bits
    return out


def uniform_widths(bits, c):
    """(offset, width) of the windows of a uniform plan: ceil((bits + 1) / c) windows of c bits (msm_plan.h make_plan)"""
    return [(c * w, c) for w in range((bits + 1 + c - 1) // c)]


def mixed_windows(bits, c):
    """the window count W of a forced mixed plan ("hip_msm_windows") whose windows are c - 1 and c bits wide: the largest W with
    bits // W == c - 1 that leaves at least one wide window (make_plan skips a W whose widths come out equal)"""
    W = bits // (c - 1)
    if bits - (c - 1) * W == 0:
        W -= 1
    assert bits // W == c - 1 and bits % W != 0
    return W


# ---- the directed bucket patterns of the reduction tests ----
def in_all_scalars_equal(r, bases_fn, neg_fn, n=(1 << 10) + 1):
    """one full bucket per window, every other bucket the identity: line and tri0 stay the identity until that row"""
    rng = np.random.default_rng(9102)
    s = rand_scalars(rng, 1, r)[0]
    return [s] * n, bases_fn(n)


def in_equal_bases_under_scalars_k_and_k_plus_one(r, bases_fn, neg_fn):
    """every bucket holds a multiple of ONE point and neighbouring buckets are full: column sums and running sums that are equal
    or negatives of each other meet in the lane scans (an addition that is a doubling, one that gives the identity)"""
    rng = np.random.default_rng(9103)
    n = 1 << 10
    bases = np.ascontiguousarray(np.tile(bases_fn(1), (n, 1)))
    vals = rand_scalars(rng, n, r)
    for i in range(0, n, 2):
        vals[i + 1] = (vals[i] + 1) % r
    vals[0:64] = [5, 6] * 32  # the same number of points in buckets 5 and 6 of window 0: equal bucket sums side by side
    return vals, bases


def in_cancelling_pairs(r, bases_fn, neg_fn, n=1 << 12):
    """cancelled buckets (the identity) between full ones"""
    rng = np.random.default_rng(9104)
    half = bases_fn(n // 2)
    bases = np.empty((n, half.shape[1]), dtype=np.uint32)
    bases[0::2] = half
    bases[1::2] = neg_fn(half)
    vals = rand_scalars(rng, n, r)
    for i in range(0, n // 2, 2):  # the first half of the pairs share a scalar: their buckets cancel where nothing else lands
        vals[i + 1] = vals[i]
    return vals, bases


def in_scalars_one_and_r_minus_one(r, bases_fn, neg_fn):
    """only bucket 1 of window 0 is populated, with both signs: every other chunk sums identities"""
    n = (1 << 11) + 7
    return [r - 1 if i % 3 else 1 for i in range(n)], bases_fn(n, period=300)


def in_top_bucket_only(r, bases_fn, wins):
    """every second window's digit is 2^(width - 1), the largest a signed digit takes; wins: (bit offset, width) of every window"""
    bits = r.bit_length()
    n = 1 << 10
    s_even = sum(1 << (off + width - 1) for k, (off, width) in enumerate(wins) if k % 2 == 0 and off + width < bits)
    s_odd = sum(1 << (off + width - 1) for k, (off, width) in enumerate(wins) if k % 2 == 1 and off + width < bits)
    assert 0 < s_even < r and 0 < s_odd < r
    return [s_even if i % 2 == 0 else s_odd for i in range(n)], bases_fn(n)


def in_identity_bases(r, bases_fn, neg_fn):
    rng = np.random.default_rng(9107)
    n = 1 << 12
    bases = bases_fn(n)
    bases[0:3] = 0
    bases[100:2000:2] = 0
    bases[3000:3500] = 0
    bases[-1] = 0
    return rand_scalars(rng, n, r), bases


def in_random(r, bases_fn, neg_fn, n=1000, seed=9120):
    return rand_scalars(np.random.default_rng(seed), n, r), bases_fn(n)


PATTERNS = [in_all_scalars_equal, in_equal_bases_under_scalars_k_and_k_plus_one, in_cancelling_pairs, in_scalars_one_and_r_minus_one, in_identity_bases]
PATTERN_IDS = [f.__name__[3:] for f in PATTERNS] + ["top_bucket_only"]  # (in_top_bucket_only takes the window plan: the tests call it themselves)


# ---- the signed recoding, as the device does it ----
def recode(s, widths, r=None, negate=False, bitsize=0):
    """signed digits of one scalar, lowest window first. widths: bits of every window. msm_impl.hpp load_scalar (only `bitsize` bits of the
    scalar are read), negate_scalar_if_top_bit (negate: a scalar with bit r.bit_length() - 1 set becomes r - s and every digit changes sign),
    DigitIter::next (v = low bits + carry; v > 2^(w - 1) gives the digit v - 2^w and a carry). The carry out of the last window is dropped."""
    if bitsize:
        s &= (1 << bitsize) - 1
    flip = 1
    if negate and (s >> (r.bit_length() - 1)) & 1:
        s, flip = r - s, -1
    out, carry = [], 0
    for w in widths:
        v = (s & ((1 << w) - 1)) + carry
        s >>= w
        if v > (1 << (w - 1)):
            carry, d = 1, v - (1 << w)
        else:
            carry, d = 0, v
        out.append(flip * d)
    return out


def bucket_counts(vals, widths, wpf=None, **kw):
    """Counter {(target window, bucket): list entries}: digit d != 0 of window w lands in bucket |d| - 1 of target window w % wpf (with a
    base table of precompute_factor pf the windows j * wpf + wp share the buckets of wp; without one wpf = the window count). Zero bases
    count too: k_accumulate skips them when it meets them, the lists hold them."""
    wpf = wpf or len(widths)
    cnt = collections.Counter()
    for s in vals:
        for w, d in enumerate(recode(s, widths, **kw)):
            if d:
                cnt[(w % wpf, abs(d) - 1)] += 1
    return cnt


# ---- overflow segments ----
def in_overflow(r, bases_fn, neg_fn, seg, sizes, c=13, nrand=1000, seed=9130):
    """`sizes`: {v: m} -- m terms with the scalar v, 1 <= v <= 2^(c - 1): all of them land in bucket v - 1 of window 0 and in no other
    window. A bucket of more than `seg` entries is split: the bucket's own thread takes the first seg, overflow threads the rest, seg each.
    The terms of one value are consecutive. A bucket of 3 seg entries and more starts with 2 seg entries of P, -P pairs (two whole segments
    that sum to the identity when the sort keeps the order of equal keys), then seg / 2 + 1 copies of one point (every madd after the first
    is a doubling), three zero rows, and distinct points for the rest; a smaller one holds distinct points. nrand full-width scalars, none
    of whose digits (windows of c bits) has a chosen value, fill the other windows and come first."""
    rng = np.random.default_rng(seed)
    assert all(1 <= v <= 1 << (c - 1) for v in sizes)
    widths = [c] * ((r.bit_length() + 1 + c - 1) // c)
    rand = [s for s in rand_scalars(rng, nrand + nrand // 4, r) if not any(abs(d) in sizes for d in recode(s, widths))][:nrand]
    assert len(rand) == nrand
    n = nrand + sum(sizes.values())
    vals = list(rand)
    bases = bases_fn(n)
    at = nrand
    for v, m in sizes.items():
        vals += [v] * m
        if m >= 3 * seg:
            bases[at + 1:at + 2 * seg:2] = neg_fn(bases[at:at + 2 * seg:2])
            run = at + 2 * seg
            bases[run:run + seg // 2 + 1] = bases[run].copy()
            bases[run + seg // 2 + 1:run + seg // 2 + 4] = 0
        at += m
    assert len(vals) == n == at
    return vals, bases


# the launches of the overflow tests, in segments: {value: bucket size}(seg). mx = the largest number of overflow segments of one bucket =
# ceil(size / seg) - 1; k_fold_overflow (msm_impl.hpp, "const uint32_t G = mx <= 2 ? 1u : (mx <= 32 ? 4u : (mx <= 256 ? 16u : 64u))") folds a
# bucket's partial sums with G lanes. The values lie in different partitions of the two-level sort and include the first and the last bucket.
def fold_width(mx):
    return 1 if mx <= 2 else 4 if mx <= 32 else 16 if mx <= 256 else 64


OVERFLOW_LAUNCHES = {  # name: (sizes(seg), mx, G)
    1: (lambda seg: {1: seg, 2: seg + 1, 65: 2 * seg, 2049: 2 * seg + 1, 4096: 3 * seg}, 2, 1),
    2: (lambda seg: {1: seg + 1, 700: 4 * seg + 1, 4096: 33 * seg}, 32, 4),
    3: (lambda seg: {3000: seg + 1, 1: 34 * seg}, 33, 16),
    4: (lambda seg: {4096: 3 * seg + 1, 130: 257 * seg}, 256, 16),
    5: (lambda seg: {2: seg + 1, 4095: 5 * seg + 1, 1025: 258 * seg}, 257, 64),
}


# ---- the groups ----
GROUPS = [("bn254", False), ("bls12_381", False), ("bls12_377", False), ("grumpkin", False), ("bn254", True), ("bls12_381", True), ("bls12_377", True)]


def gid(cname, g2):
    return f"{cname}{'_g2' if g2 else ''}"


K0 = 987654321  # the bases are (K0 + i) G
PERIOD = 1024   # distinct bases of an input; the builders tile them


class Group:
    """One of the seven groups the MSM kernels are instantiated for."""

    def __init__(self, cname, g2):
        self.cname, self.g2, self.id = cname, g2, gid(cname, g2)
        self.C = pyref.G2_CURVES[cname] if g2 else pyref.CURVES[cname]
        base = self.C.base if g2 else self.C
        self.r, self.q, self.bits = base.r, base.q, base.r.bit_length()
        self.L = base.limbs_q        # 32-bit words of a coordinate component in the C ABI
        self.ext = 2 if g2 else 1
        # what the launch decisions read of the group: field_consts.h NL (29-bit limbs: 9 up to 261 bits, 14 for the 377- and 381-bit fields),
        # sizeof(EC::Proj) = 3 coordinates, sizeof(EC::XYZZ) = 4; msm_impl.hpp ReduceWindowLanes (the window kernel's block: its LDS holds a
        # point per thread) and MsmLaunch::QUAD_OK (the four-lane reduction: G1, and the G2 whose XYZZ point is at most 288 bytes)
        self.limbs = 9 if self.q.bit_length() <= 261 else 14
        self.proj_bytes, self.xyzz_bytes = 3 * self.ext * self.limbs * 4, 4 * self.ext * self.limbs * 4
        self.rwl = 256 if self.proj_bytes * 256 <= 60 * 1024 else 128
        self.quad_ok = self.ext == 1 or self.xyzz_bytes <= 288
        self._table = None

    # -- oracle side (Python integers) --
    def mul_g(self, k):
        if self.g2:
            return pyref.g2_mul(self.C, k, (self.C.gx, self.C.gy))
        return pyref.ec_mul(self.C, k, (self.C.gx, self.C.gy))

    def gen(self, n, k0):
        return pyref.g2_gen_points(self.C, n, k0) if self.g2 else pyref.gen_points(self.C, n, k0)

    def rows(self, pts):
        """affine points -> rows of the C ABI (x | y; G2: x0 | x1 | y0 | y1)"""
        if self.g2:
            return np.concatenate([to_words([p[0][0] for p in pts], self.L), to_words([p[0][1] for p in pts], self.L),
                                   to_words([p[1][0] for p in pts], self.L), to_words([p[1][1] for p in pts], self.L)], axis=1)
        return np.concatenate([to_words([p[0] for p in pts], self.L), to_words([p[1] for p in pts], self.L)], axis=1)

    def _ints(self, row):
        L = self.L
        return [sum(int(x) << (32 * k) for k, x in enumerate(row[i * L:(i + 1) * L])) for i in range(len(row) // L)]

    def affine(self, proj_row):
        """a projective result row -> the affine point as Python integers (the identity: (0, 0) / ((0, 0), (0, 0)))"""
        v = self._ints(proj_row)
        if self.g2:
            return pyref.g2_proj_to_affine(self.C, (v[0], v[1]), (v[2], v[3]), (v[4], v[5]))
        return pyref.proj_to_affine(self.C, *v)

    def neg_rows(self, arr):
        L, q, half = self.L, self.q, self.ext * self.L
        out = arr.copy()
        for i, row in enumerate(arr):
            out[i, half:] = to_words([(q - y) % q for y in self._ints(row[half:])], L).reshape(-1)
        return out

    # -- inputs: the distinct bases come from `points`, a function (n, k0) -> rows of (k0 + i) G --
    def bind(self, points):
        """points: generate_affine_points of the product on the GPU (checked against the Python definition by the tests' section 0)"""
        base = points(PERIOD, K0)
        self._table = {}
        for sign, rows in ((1, base), (-1, self.neg_rows(base))):
            for i, row in enumerate(rows):
                self._table[row.tobytes()] = sign * (K0 + i)
        self._table[np.zeros_like(base[0]).tobytes()] = 0
        self._base = base
        return self

    def bases_fn(self, n, period=PERIOD):
        pts = self._base[:min(n, period)]
        return np.ascontiguousarray(np.tile(pts, ((n + period - 1) // period, 1))[:n])

    def fns(self):
        return self.r, self.bases_fn, self.neg_rows

    def multipliers(self, bases):
        """k_i of every row: K0 + j for the j-th distinct base, -(K0 + j) for its negation, 0 for a zero row"""
        return [self._table[row.tobytes()] for row in bases]

    def expected(self, vals, bases, bitsize=0):
        """((sum s_i k_i) mod r) G, affine"""
        mask = (1 << bitsize) - 1 if bitsize else -1
        return self.mul_g(sum((s & mask) * k for s, k in zip(vals, self.multipliers(bases))) % self.r)


class ModelGroup(Group):
    """the same group without a device: base rows that only tell distinct, negated and zero rows apart (for the bucket-count model)"""

    def __init__(self, cname, g2):
        super().__init__(cname, g2)
        self._base = np.zeros((PERIOD, 2), dtype=np.uint32)
        self._base[:, 0] = np.arange(1, PERIOD + 1)

    def neg_rows(self, arr):
        out = arr.copy()
        out[:, 1] ^= (arr[:, 0] != 0).astype(np.uint32)
        return out


# ---- the shapes of tests/test_gpu_msm_groups_directed.py; tests/test_msm_groups_directed_cpu.py pins the route of each from msm_plan.h ----
OVERFLOW_C = 13                       # section 1: 4096 buckets per window, two-level sort, seg = 64 up to 2^15 terms
NEVER_ONE_LANE = [("bls12_381", False), ("bls12_377", False), ("bn254", True), ("bls12_381", True), ("bls12_377", True)]  # section 2
ONE_LANE_CS = (8, 13, 16)             # one chunk per window (direct store) / 4 chunks / 64 (BLS G2) chunks per window
BATCH_CS = (13, 16)                   # (a batch of two at c = 8 has 64 windows of 128 buckets: k_reduce_small's)
SMALL_GROUPS = [("bn254", False), ("bls12_381", False), ("bn254", True), ("bls12_381", True)]  # section 3
# (config.c, batch, bitsize): batch * wpf >= 64 windows of 16 / 64 / 128 / 512 buckets -> 4 / 8 / 16 / 32 lanes per window. With 254- and 255-bit
# scalars c = 8 and 10 give an even number of windows per MSM, so every wave is full; a bitsize of 247 / 240 bits gives 31 / 25 windows and a batch of
# three leaves the last wave partly empty there as well
SMALL_SHAPES = [(5, 2, 0), (7, 2, 0), (8, 2, 0), (10, 4, 0), (8, 3, 247), (10, 3, 240)]
SMALL_LW_LOG = {5: 2, 7: 3, 8: 4, 10: 5}
FULL_WINDOW_GROUP = ("bls12_381", True)  # section 4: ReduceWindowLanes = 128 and a window of 2^17 / 2^18 buckets: all 128 chunks in use
FULL_WINDOW_CS = (18, 19)
