"""The 37 distinct 16-point ECNTT inputs shared by tests/test_gpu_ecntt_routes.py (GPU) and tests/test_oracle.py (CPU; the premise that
the reference backend is representative-independent on them). 37 is prime: tiled over a batch -- transform b of a call is distinct[b % 37]
-- an index error by any power-of-two stride lands on a different transform.

A slot is (affine point or pyref.INF, lam): the projective_t words are (lam x : lam y : lam), the identity's (0 : lam : 0); lam = 1 is the
normalised form. For transforms 0..10 the discrete logarithms to the generator are known, which gives a second ground truth in Python
integers (expected_from_scalars)."""
import numpy as np

from oracle import pyref
from tests.util import cached_points, rand_scalars, to_words

N = 16
LOGN = 4
COUNT = 37
KNOWN = 11  # transforms 0 .. 10 come with their scalars
ORD = {0: "NN", 1: "NR", 2: "RN", 3: "RR"}
# the two calls every shape runs, as (direction, ordering, columns_batch, coset generator): forward kNR rows with a coset (the scale pass
# in front of the stages); inverse kRN columns_batch with a coset (the scale pass behind them, the coset folded into 1 / N)
FORWARD_CALL = (0, 1, False, 0x1234567)
INVERSE_CALL = (1, 2, True, 0x7654321)


def _lams(rng, C, n):
    return [v or 1 for v in rand_scalars(rng, n, C.q)]


def transforms(cname):
    """-> (slots, scalars): slots[t] = 16 (point, lam) pairs for t < 37, scalars[t] = the 16 discrete logarithms for t < 11"""
    C, F = pyref.CURVES[cname], pyref.NTT_FIELDS[cname]
    r = F.p  # the group order is the NTT field's modulus
    rng = np.random.default_rng(3700 + len(cname))
    G = (C.gx, C.gy)
    k, k7, k8 = (v or 5 for v in rand_scalars(rng, 3, r))
    mul = lambda s: pyref.ec_mul(C, s, G)
    slots, scalars = [], []

    def known(ks, lams=None):
        scalars.append([s % r for s in ks])
        slots.append([(mul(s), lam) for s, lam in zip(ks, lams or [1] * N)])

    known([0] * N)  # 0: all identity (0 : 1 : 0)
    known([0] * N, _lams(rng, C, N))  # 1: all identity, (0 : lam_j : 0)
    known([k] * N)  # 2: the same point in every slot
    known([k] * N, _lams(rng, C, N))  # 3: the same group element, a different representative per slot
    for at in (0, 1, 15):  # 4-6: one point, identity elsewhere
        known([k if j == at else 0 for j in range(N)])
    known([k7 if j % 2 == 0 else r - k7 for j in range(N)])  # 7: P, -P, P, -P, ...
    known([k8 if j < N // 2 else r - k8 for j in range(N)])  # 8: P in the first half, -P in the second
    known([j + 1 for j in range(N)])  # 9: (j + 1) G
    # 10: k = the inverse scalar NTT of a vector with three nonzero entries: a plain forward transform gives the identity everywhere but
    # at those three places -- sixteen nonzero multiples of G whose partial sums cancel to the identity inside the butterflies (a
    # half-size sub-transform is (X[k] +- X[k + 8]) / 2 up to a twiddle: zero wherever both are)
    sparse = [0] * N
    for at, v in zip((1, 6, 11), rand_scalars(rng, 3, r)):
        sparse[at] = v or 1
    known(pyref.ntt_naive(F, sparse, pyref.omega(F, LOGN), inverse=True))
    assert len(slots) == KNOWN
    for t in range(KNOWN, COUNT):  # 11-36: runs of distinct points, distinct k0
        pts = list(cached_points(C, N, k0=1000003 + 7919 * t))
        if t in (13, 24):  # a single identity slot
            pts[(5 * t) % N] = pyref.INF
        if t in (14, 29):  # an equal pair
            pts[(3 * t + 1) % N] = pts[t % N]
        slots.append(list(zip(pts, _lams(rng, C, N) if t % 3 == 0 else [1] * N)))
    return slots, scalars


def words(C, slots, normalised=False):
    """slots of one transform -> [16, 3 L] uint32 projective_t words"""
    L = C.limbs_q
    rows = []
    for p, lam in slots:
        lam = 1 if normalised else lam
        xyz = (0, lam, 0) if p == pyref.INF else (p[0] * lam % C.q, p[1] * lam % C.q, lam)
        rows.append(to_words(list(xyz), L).reshape(-1))
    return np.ascontiguousarray(np.stack(rows).astype(np.uint32))


def affine_words(C, pts):
    """affine python points -> [n, 2 L] uint32 in the encoding to_affine gives (the identity is (0, 0))"""
    L = C.limbs_q
    return np.concatenate([to_words([p[0] for p in pts], L), to_words([p[1] for p in pts], L)], axis=1)


def expected_from_scalars(cname, ks, inverse, ordering, coset_gen):
    """NTT(k)_i G for one transform with known scalars, under the call's direction, ordering ("NR", ...) and coset: [16, 2 L] affine words"""
    C, F = pyref.CURVES[cname], pyref.NTT_FIELDS[cname]
    out = pyref.ntt_naive(F, ks, pyref.omega(F, LOGN), inverse=inverse, coset_gen=coset_gen, ordering=ordering)
    return affine_words(C, [pyref.ec_mul(C, s, (C.gx, C.gy)) for s in out])


def tile(per_transform, batch, columns):
    """[37, 16, W] per-transform rows -> the [16 * batch, W] layout of a call whose transform b is distinct[b % 37]: rows, or
    element j of transform b at j * batch + b (columns_batch)"""
    idx = np.arange(batch) % COUNT
    t = per_transform[idx]  # [batch, 16, W]
    if columns:
        t = t.transpose(1, 0, 2)
    return np.ascontiguousarray(t.reshape(N * batch, -1))
