"""CPU: the identity of tests/ntt_identity.py in Python integers, against the O(n^2) definition pyref.ntt_naive:
sum_k r^k X[k] = (1 - r^n) sum_j x_j g^j / (1 - r w^j) holds for a plain and for a coset transform, and for the inverse with the roles
swapped; a single output changed by 1 breaks it; the row split and host combine of the device path change nothing."""
import random

import pytest

from oracle import pyref
from tests import ntt_identity as I

LOGN = 6


@pytest.mark.parametrize("fname", ["goldilocks", "bn254"])
def test_identity_holds_and_detects_one_changed_output(fname):
    F = pyref.NTT_FIELDS[fname]
    p, n = F.p, 1 << LOGN
    w_n = pyref.omega(F, LOGN)
    rng = random.Random(4242)
    x = [rng.randrange(p) for _ in range(n)]
    x[3], x[7], x[11] = 0, 1, p - 1
    r = I.challenge(p, n, seed=91)
    assert pow(r, n, p) != 1
    g = rng.randrange(2, p)
    assert pow(g, n, p) != 1  # not a power of w: a real coset
    for gen in (1, g):
        X = pyref.ntt_naive(F, x, w_n, coset_gen=gen)
        for row in (None, 16, 1):  # one row, four rows, a row per element
            lhs, rhs = I.python_sides(p, w_n, x, X, r, gen, row)
            assert lhs == rhs, (fname, gen, row)
        for k in (0, n - 1, rng.randrange(n)):  # one output off by one: both signs
            for delta in (1, p - 1):
                bad = list(X)
                bad[k] = (bad[k] + delta) % p
                lhs, rhs = I.python_sides(p, w_n, x, bad, r, gen, 16)
                assert lhs != rhs, (fname, gen, k)
        # the coset form must be told the generator: the plain form rejects a coset transform
        if gen != 1:
            lhs, rhs = I.python_sides(p, w_n, x, X, r, 1)
            assert lhs != rhs
        # an inverse transform, roles swapped: y = INTT(X) is accepted as check(x=y, X=X)
        y = pyref.ntt_naive(F, X, w_n, inverse=True, coset_gen=gen)
        assert y == x
        lhs, rhs = I.python_sides(p, w_n, y, X, r, gen, 16)
        assert lhs == rhs


@pytest.mark.parametrize("fname", ["goldilocks", "bn254", "stark252"])
def test_canonical_is_an_unsigned_word_comparison_top_word_first(fname):
    """the identity accepts X[k] + p, so the outputs are also compared with the modulus: p - 1 passes, p and everything above fails,
    whichever word decides, with words above 2^31 (negative as int32) ordered as unsigned"""
    import torch

    F = pyref.NTT_FIELDS[fname]
    p, w = F.p, I.WORDS[fname]
    dev = torch.device("cpu")
    top = 1 << (32 * w)
    good = [0, 1, p - 1, p - 2, p >> 1, p - (1 << 32), p - (1 << (32 * (w - 1))), 0x80000000, 0xFFFFFFFF, p & ~0xFFFFFFFF]
    bad = [v for v in (p, p + 1, top - 1, p + 0x80000000, p + (1 << 32), p + (1 << (32 * (w - 1))), (p & ~0xFFFFFFFF) + (1 << 32)) if v < top]
    assert all(0 <= v < p for v in good) and all(p <= v < top for v in bad) and len(bad) >= 3
    base = torch.stack([I.element_tensor(v, w, dev) for v in good])
    assert I.canonical(base, p)
    for i, v in enumerate(good):  # each alone, too
        assert I.canonical(base[i:i + 1], p), hex(v)
    for v in bad:
        for pos in (0, len(good) // 2, len(good) - 1):
            x = base.clone()
            x[pos] = I.element_tensor(v, w, dev)
            assert not I.canonical(x, p), (hex(v), pos)


def test_random_elements_are_canonical_and_fill_the_words():
    import torch

    for fname in ("goldilocks", "bn254"):
        p, w = pyref.NTT_FIELDS[fname].p, I.WORDS[fname]
        x = I.random_elements(fname, p, 4096, torch.Generator().manual_seed(5), torch.device("cpu"))
        assert x.shape == (4096, w) and x.dtype == torch.int32 and I.canonical(x, p)
        assert bool((x[:, :w - 1] < 0).any()) and bool((x[:, :w - 1] > 0).any())  # all 32 bits of a word are used
        y = I.random_elements(fname, p, 4096, torch.Generator().manual_seed(5), torch.device("cpu"))
        assert torch.equal(x, y)


def test_split_and_words():
    assert I.split_logn(8) == [8] and I.split_logn(16) == [8, 8] and I.split_logn(17) == [6, 6, 5] and I.split_logn(24) == [8, 8, 8]
    assert I.split_logn(25) == [9, 8, 8] and I.split_logn(27) == [9, 9, 9] and I.split_logn(28) == [10, 9, 9]
    p = pyref.BN254_FR.p
    assert I.from_words(I.to_words(p - 1, 8)) == p - 1
    assert I.from_words(I.to_words(p - 1, 8).view("int32")) == p - 1  # the int32 view of the device tensors
