"""Directed operands for the field arithmetic (bigfield.hpp, fq2.hpp, goldfield.hpp, smallfield.hpp): the values at which
limb arithmetic goes wrong and which uniformly random operands never draw. Plain Python, no GPU; shared by the host tests
(tests/test_host_math.py), the device tests (tests/test_gpu_device_math.py) and the vector-op tests.

29-bit-radix fields, `directed_values(p, NL, NL32)` -- every group once as a plain value and once placed in the MONTGOMERY
domain (v = pattern * R^-1 mod p, so that from_canonical(v) hands mul() exactly the pattern's limbs), R = 2^(29*NL):
  * 0, 1, 2, 3, p-1, p-2, p-3, (p-1)/2, (p+1)/2, R, R^2, -R, R^-1 (mod p)          identities, negation, conversion constants
  * 2^(29k)+d, p-2^(29k)+d, d in {-1,0,1}, every limb boundary k                    carries / borrows across one limb (add, sub<K>)
  * the same at the 32-bit word boundaries                                          unpack / pack (two- and three-limb words)
  * largest value below p whose k low limbs are all ones                            carry runs through 0x1fffffff limbs
  * alternating all-ones / zero limbs (both phases)                                 carry stops / borrow runs through zero limbs
  * p with its k low limbs cleared, p mod 2^(29k)                                   cond_sub<K> ties: equal top limbs, the borrow
                                                                                    from below decides
`directed_pairs` = all ordered pairs of that list, pairs by relation ((a,a), (a,p-a), (a,a+1), (a,a-1)) and a fixed count
of seeded random pairs. `lazy_limbs` gives the raw lazy representatives a0 + j*p that the raw-mode tests feed the ops
without any conversion (exact multiples K*p and their neighbours included: the ties of cond_sub<K>, is_zero, eq).

Goldilocks (`gold_values`, `gold_pairs`; goldfield.hpp keeps elements canonical in one u64), branch by branch:
  * add:  a+b wraps 2^64 ("s < a.v")        pairs with a+b >= 2^64: (p-1, p-1), (2^63, 2^63), (p-2^32, 2^32+1) ...
          a+b in [p, 2^64) ("s >= P")       pairs with a+b = p, p+1, 2^64-1: (a, p-a), (a, p+1-a), (a, 2^64-1-a)
          neither                           a+b = p-1 and small values
  * sub:  a < b (borrow, "d -= EPS") / a >= b                  (0, 1), (a, a+1), (a, a), (p-1, 0)
  * neg:  a == 0 / a != 0
  * reduce128 (mul): "lo < hh"              (x*2^32) * (y*2^32) with x*y = -1 mod 2^32 and x*y >= 2^32: lo = 0 < hh, hl = 2^32-1
          "r < t1" (t0 + t1 wraps)          same family and (p-1)*(p-1), (p-2)*(p-1)
          final "r >= P"                    2 * (2^63 - 2^31 + 1) = p + 1 and neighbours: hi = 0, lo in [p, 2^64)
  * unpack "v >= P": only a non-canonical word pair reaches it (`GOLD_NONCANONICAL`, used where the interface allows it)
`gold_branches(a, b)` is an integer model of those branches; tests/test_host_math.py asserts that the pair list takes every one.

BabyBear / KoalaBear (`small_values`): 0, 1, 2, p-1, p-2, (p-1)/2, (p+1)/2, 2^k and 2^k-1 around the word's top bits, R mod p,
R^2 mod p, p-R mod p, each also in the Montgomery domain (R = 2^32); all pairs."""
import random

RB = 29
RANDOM_PAIRS = 2000  # fixed, seeded


def _patterns(p, NL, NL32):
    R = 1 << (RB * NL)
    Rinv = pow(R, -1, p)
    out = [0, 1, 2, 3, p - 1, p - 2, p - 3, (p - 1) // 2, (p + 1) // 2, R % p, R * R % p, (-R) % p, Rinv]
    for width, count in ((RB, NL), (32, NL32)):
        for k in range(1, count):
            for d in (-1, 0, 1):
                out += [(1 << (width * k)) + d, p - (1 << (width * k)) + d]
    for k in range(1, NL):
        ones = (1 << (RB * k)) - 1
        v = ((p >> (RB * k)) << (RB * k)) | ones
        if v >= p:
            v -= 1 << (RB * k)
        out += [v, (p >> (RB * k)) << (RB * k), p & ones]
    below_top = (1 << (p.bit_length() - 1)) - 1
    for phase in (0, 1):
        v = sum(((1 << RB) - 1) << (RB * i) for i in range(NL) if i % 2 == phase)
        out.append(v & below_top)
    return [v for v in out if 0 <= v < p]


def directed_values(p, NL, NL32):
    """deterministic list of distinct canonical values, plain patterns first, then the same patterns in the Montgomery domain"""
    pats = _patterns(p, NL, NL32)
    Rinv = pow(1 << (RB * NL), -1, p)
    seen, out = set(), []
    for v in pats + [v * Rinv % p for v in pats]:
        if v not in seen:
            seen.add(v)
            out.append(v)
    return out


def relation_pairs(vals, p):
    out = []
    for a in vals:
        out += [(a, a), (a, (p - a) % p), (a, (a + 1) % p), (a, (a - 1) % p)]
    return out


def random_pairs(p, count=RANDOM_PAIRS, seed=0):
    rnd = random.Random(0xD1EC7ED ^ seed)
    return [(rnd.randrange(p), rnd.randrange(p)) for _ in range(count)]


def directed_pairs(p, NL, NL32, seed=0):
    """(directed pairs, random pairs): every ordered pair of directed_values plus the pairs by relation; then the seeded random ones"""
    vals = directed_values(p, NL, NL32)
    return [(a, b) for a in vals for b in vals] + relation_pairs(vals, p), random_pairs(p, RANDOM_PAIRS, seed)


def to_limbs(v, NL):
    """normalised limb vector: limbs 0..NL-2 below 2^29, the rest in the top limb (must fit 32 bits)"""
    l = [(v >> (RB * i)) & ((1 << RB) - 1) for i in range(NL - 1)] + [v >> (RB * (NL - 1))]
    assert 0 <= l[-1] < (1 << 32)
    return l


def from_limbs(l):
    return sum(int(x) << (RB * i) for i, x in enumerate(l))


def max_bound(p, NL):
    """FieldOps::max_bound(): min(R/p lower bound, 64) in units of p"""
    return min(1 << (RB * NL - p.bit_length()), 64)


def lazy_values(a0, K, p, NL):
    """the representatives a0 + j*p, j = 0..K-1 (all below K*p), capped by max_bound() and by value < 2^(29*NL)"""
    K = min(K, max_bound(p, NL))
    return [a0 + j * p for j in range(K) if a0 + j * p < (1 << (RB * NL))]


LAZY_K = (1, 2, 4, 8, 16, 32, 64)


def raw_seeds(p, NL, NL32):
    """canonical a0 for the raw lazy representatives: the tie makers (0, 1, p-1: a0 + j*p is K*p and its neighbours), limb-boundary
    values, the cond_sub tie patterns, and Montgomery-domain ones"""
    R = 1 << (RB * NL)
    Rinv = pow(R, -1, p)
    out = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, R % p, Rinv, (1 << RB) - 1, 1 << RB, p - (1 << RB),
           (1 << (RB * (NL - 1))) - 1, 1 << (RB * (NL - 1)), p - (1 << (RB * (NL - 1))), p & ((1 << (RB * (NL - 1))) - 1),
           (p >> (RB * (NL - 1))) << (RB * (NL - 1)), (p >> RB) << RB, p & ((1 << RB) - 1)]
    v = ((p >> (RB * (NL - 1))) << (RB * (NL - 1))) | ((1 << (RB * (NL - 1))) - 1)
    out.append(v if v < p else v - (1 << (RB * (NL - 1))))
    for phase in (0, 1):
        out.append(sum(((1 << RB) - 1) << (RB * i) for i in range(NL) if i % 2 == phase) & ((1 << (p.bit_length() - 1)) - 1))
    rnd = random.Random(p & 0xFFFF)
    out += [rnd.randrange(p) for _ in range(6)]
    seen, res = set(), []
    for x in out:
        x %= p
        if x not in seen:
            seen.add(x)
            res.append(x)
    return res


# ---- goldilocks --------------------------------------------------------------------------------------------------------------
GOLD_P = 0xFFFFFFFF00000001
GOLD_EPS = 0xFFFFFFFF
GOLD_NONCANONICAL = [GOLD_P, GOLD_P + 1, (1 << 64) - 1, (1 << 64) - 2]  # word pairs in [p, 2^64): unpack's "v >= P"


def gold_values():
    p = GOLD_P
    out = [0, 1, 2, p - 1, p - 2, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, 1 << 63, p - (1 << 32), (p - 1) // 2, (p + 1) // 2,
           (1 << 63) - (1 << 31) + 1, (1 << 63) - (1 << 31), (1 << 63) - (1 << 31) + 2, (1 << 31), (1 << 33) - 1, (1 << 48) + 1,
           (1 << 63) - 1, (1 << 63) + 1, p - (1 << 32) - 1, p - (1 << 32) + 1, 0xFFFFFFFE00000001, 0xFFFFFFFE00000000, 0xFFFFFFFEFFFFFFFF]
    # (x * 2^32) * (y * 2^32) = x*y * 2^64: lo = 0, hi = x*y with low word 2^32 - 1 and a non-zero high word
    for x in (0xFFFFFFFB, 0xFFFFFFFD, 0x10001, 0xDEADBEEF, 0x7FFFFFFF, 5):
        y = (-pow(x, -1, 1 << 32)) % (1 << 32)
        out += [x << 32, y << 32]
    seen, res = set(), []
    for v in out:
        if 0 <= v < p and v not in seen:
            seen.add(v)
            res.append(v)
    return res


def gold_pairs(seed=0):
    p = GOLD_P
    vals = gold_values()
    pairs = [(a, b) for a in vals for b in vals]
    for a in vals:
        for s in (p - 1, p, p + 1, (1 << 64) - 1, 1 << 64, (1 << 64) + 1):  # a + b equal to ...
            b = s - a
            if 0 <= b < p:
                pairs.append((a, b))
    pairs += relation_pairs(vals, p)
    return pairs, random_pairs(p, RANDOM_PAIRS, 7 + seed)


def gold_branches(a, b):
    """the branches of goldfield.hpp that (a, b) takes, as a set of names (integer model of add / sub / neg / reduce128)"""
    p, M = GOLD_P, 1 << 64
    out = set()
    s = (a + b) % M
    out.add("add:wrap" if s < a else ("add:ge_p" if s >= p else "add:plain"))
    out.add("sub:borrow" if a < b else "sub:plain")
    out.add("neg:zero" if a == 0 else "neg:nonzero")
    hi, lo = (a * b) >> 64, (a * b) % M
    hh, hl = hi >> 32, hi & GOLD_EPS
    t0 = (lo - hh) % M
    if lo < hh:
        out.add("red:lo<hh")
        t0 = (t0 - GOLD_EPS) % M
        if hl == GOLD_EPS:
            out.add("red:lo<hh,hl=max")
    else:
        out.add("red:lo>=hh")
    t1 = hl * GOLD_EPS
    r = (t0 + t1) % M
    if r < t1:
        out.add("red:wrap")
        r = (r + GOLD_EPS) % M
    else:
        out.add("red:nowrap")
    out.add("red:final_ge_p" if r >= p else "red:final_lt_p")
    assert r % p == a * b % p
    return out


GOLD_ALL_BRANCHES = {"add:wrap", "add:ge_p", "add:plain", "sub:borrow", "sub:plain", "neg:zero", "neg:nonzero", "red:lo<hh", "red:lo<hh,hl=max",
                     "red:lo>=hh", "red:wrap", "red:nowrap", "red:final_ge_p", "red:final_lt_p"}


# ---- 31-bit fields -----------------------------------------------------------------------------------------------------------
def small_values(p):
    R = 1 << 32
    Rinv = pow(R, -1, p)
    pats = [0, 1, 2, 3, p - 1, p - 2, p - 3, (p - 1) // 2, (p + 1) // 2, R % p, R * R % p, (-R) % p, Rinv, (1 << 31) - p, (1 << 32) - 2 * p]
    for k in (8, 16, 24, 27, 29, 30):
        pats += [(1 << k) - 1, 1 << k, (1 << k) + 1, p - (1 << k), p - (1 << k) - 1, p - (1 << k) + 1]
    seen, res = set(), []
    for v in pats + [v * Rinv % p for v in pats]:
        v %= p
        if v not in seen:
            seen.add(v)
            res.append(v)
    return res


def small_pairs(p, seed=0):
    vals = small_values(p)
    return [(a, b) for a in vals for b in vals] + relation_pairs(vals, p), random_pairs(p, RANDOM_PAIRS, 11 + seed)
