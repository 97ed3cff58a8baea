"""CPU: the Python model of slice / highest_non_zero_idx / poly_eval / poly_division (tests/poly_model.py) against the reference CPU
backend (oracle/_ref/libicicle_field_<F>.so, backend/cpu/src/field/cpu_vec_ops.cpp:566-780), byte for byte, wherever the reference is
defined -- and where it is not, pinned in a child process, because an assertion of the reference ends the process that called it.

What this pins about cpu_poly_divide (tests/poly_ref.py states the rules the other tests then rely on):
  * batch_size == 1, and columns_batch with r_size == numerator_size, agree with the model on zero-filled outputs;
  * a numerator with deg_n < deg_b - 1 (a zero numerator among them) trips the q_size assertion, whatever q_size is;
  * a constant denominator with a numerator whose constant term is not zero trips the size != 0 assertion of the remainder's rescan;
  * row batches: entry 0 agrees, later entries need not (the remainder is rescanned at r_out + idx * deg_r) -- not called here."""
import subprocess
import sys

import numpy as np
import pytest

from tests import poly_model as M
from tests import poly_ref as R

pytestmark = pytest.mark.skipif(not all(R.ref_available(f) for f in R.ALL), reason="oracle/_ref not built")


@pytest.mark.parametrize("f", R.ALL)
def test_slice_equals_the_reference(f):
    p, w = R.modulus(f), R.FIELDS[f]
    rng = np.random.default_rng(2203)
    n = 24
    for batch, columns in ((1, False), (3, False), (3, True)):
        vals = R.rand_vals(rng, n * batch, p)
        a = R.words(vals, w)
        for offset, stride, size_out in ((0, 1, n), (1, 2, n // 2), (n - 1, 1, 1), (3, 5, 5), (4, 0, 6)):
            if size_out > 1 and stride:
                assert offset + (size_out - 1) * stride <= n - 1
            want = M.slice_(vals, offset, stride, n, size_out, batch, columns)
            assert R.ints(R.ref_slice(f, a, offset, stride, n, size_out, batch, columns), w) == want, (f, batch, columns, offset, stride)
    assert (3 + 4 * 5) == n - 1  # (3, 5, 5) ends exactly on the last index
    with pytest.raises(ValueError):
        M.slice_(list(range(n)), 3, 5, n, 6)
    with pytest.raises(ValueError):
        M.slice_(list(range(n)), n, 0, n, 2)
    assert M.slice_(list(range(n)), n, 7, n, 0) == []


@pytest.mark.parametrize("f", R.ALL)
def test_highest_non_zero_idx_equals_the_reference(f):
    p, w = R.modulus(f), R.FIELDS[f]
    n = 9
    cases = [[0] * n, [5] + [0] * (n - 1), [0] * (n - 1) + [p - 1], [0, 3, 0, 7, 0, 0, 0, 0, 0]]
    if w > 1:
        cases.append([0, 0, 1 << 32, 0, 0, 0, 0, 0, 0])  # the low word is zero, the element is not
    for vals in cases:
        assert list(R.ref_hnz(f, R.words(vals, w), n)) == M.highest_non_zero_idx(vals, n) == [M.degree(vals)], (f, vals)
    ents = [cases[0], cases[2], cases[3]]
    for columns in (False, True):
        flat = M.pack(ents, columns)
        assert list(R.ref_hnz(f, R.words(flat, w), n, 3, columns)) == M.highest_non_zero_idx(flat, n, 3, columns) == [-1, n - 1, 3], (f, columns)


@pytest.mark.parametrize("f", R.ALL)
def test_poly_eval_equals_the_reference(f):
    p, w = R.modulus(f), R.FIELDS[f]
    rng = np.random.default_rng(2213)
    domain = [0, 1, p - 1] + R.rand_vals(rng, 6, p)
    for n in (1, 2, 17):
        for batch, columns in ((1, False), (3, False), (3, True)):
            coeffs = R.rand_vals(rng, n * batch, p)
            if n > 2:
                coeffs[-1] = 0  # a zero leading coefficient somewhere
            want = M.poly_eval(p, coeffs, n, domain, batch, columns)
            assert R.ints(R.ref_eval(f, R.words(coeffs, w), n, R.words(domain, w), batch, columns), w) == want, (f, n, batch, columns)


def _division_cases(rng, p):
    """(numerator, denominator) of single entries inside the reference's domain of definition"""
    out = []
    for dn, db in ((0, 1), (1, 1), (5, 1), (7, 3), (12, 12), (12, 11), (3, 4), (9, 0), (20, 7)):
        num, den = R.rand_vals(rng, dn + 1, p, nonzero=True), R.rand_vals(rng, db + 1, p, nonzero=True)
        if db == 0:
            num[0] = 0  # a constant denominator: only with a zero constant term in the numerator
        out.append((num, den))
    num, den = out[-1]
    out.append((num + [0, 0, 0], den + [0, 0]))  # buffers longer than the degrees
    q = [0, 0, 4, 0, 0, 0, p - 1, 1]
    out.append((M.poly_mul(p, q, den), den))  # an exact product whose quotient has runs of zeros
    return out


@pytest.mark.parametrize("f", R.ALL)
def test_poly_division_equals_the_reference_where_it_is_defined(f):
    p, w = R.modulus(f), R.FIELDS[f]
    rng = np.random.default_rng(2221)
    cases = _division_cases(rng, p)
    for num, den in cases:
        assert R.ref_division_defined(num, den)
        for extra in (0, 3):
            q_size, r_size = max(1, len(num) - M.degree(den)) + extra, len(num) + extra
            want_q, want_r = M.poly_division(p, num, len(num), den, len(den), q_size, r_size)
            got_q, got_r = R.ref_division(f, R.words(num, w), len(num), R.words(den, w), len(den), q_size, r_size)
            assert (R.ints(got_q, w), R.ints(got_r, w)) == (want_q, want_r), (f, len(num), len(den), extra)
            # and the identity itself, in integers
            back = M.poly_mul(p, want_q, den)
            back = [(x + y) % p for x, y in zip(back + [0] * len(num), want_r + [0] * len(num))][:len(num)]
            assert back == num and M.degree(want_r) < M.degree(den)
    # columns_batch with r_size == numerator_size: three entries of different degrees in buffers of one size
    ns, bs = 24, 13
    trio = [cases[3], cases[8], cases[5]]
    nums = [n + [0] * (ns - len(n)) for n, _ in trio]
    dens = [d + [0] * (bs - len(d)) for _, d in trio]
    num, den = M.pack(nums, True), M.pack(dens, True)
    q_size = 21
    want_q, want_r = M.poly_division(p, num, ns, den, bs, q_size, ns, 3, True)
    got_q, got_r = R.ref_division(f, R.words(num, w), ns, R.words(den, w), bs, q_size, ns, 3, True)
    assert (R.ints(got_q, w), R.ints(got_r, w)) == (want_q, want_r), f


def test_model_rules_of_the_division():
    p = R.modulus("babybear")
    assert M.poly_division(p, [4, 0, 0], 3, [5, 1, 7], 3, 2, 3) == ([0, 0], [4, 0, 0])  # shorter than the denominator: r = numerator
    assert M.poly_division(p, [0, 0, 0], 3, [5, 1], 2, 1, 1) == ([0], [0])              # a zero numerator gives zeros
    for args in (([1, 2, 3], 3, [0, 0], 2, 3, 3), ([1, 2, 3], 3, [5, 1], 2, 1, 3), ([1, 2, 3], 3, [5, 1], 2, 2, 2)):
        with pytest.raises(ValueError):  # a zero denominator, a q_size and an r_size too small
            M.poly_division(p, *args)
    with pytest.raises(ValueError):  # a zero denominator in entry 1 of 3
        M.poly_division(p, [1, 2, 3] * 3, 3, [5, 1, 0, 0, 5, 1], 2, 3, 3, 3, False)


_CHILD = """
import sys
import numpy as np
from tests import poly_ref as R
num, den = {num}, {den}
print("calling", flush=True)
R.ref_division("babybear", R.words(num, 1), len(num), R.words(den, 1), len(den), 5, len(num), guard=False)
print("returned", flush=True)
"""


@pytest.mark.parametrize("num,den,what", [([0, 0, 0], [5, 1], "q_size >="), ([4, 0, 0], [5, 1, 7], "q_size >="), ([1, 2, 3], [5], "size != 0"), ([7], [5], "size != 0")])
def test_where_the_reference_is_not_defined(num, den, what):
    """the reference asserts: its exception leaves through the C interface and ends the child"""
    assert not R.ref_division_defined(num, den)
    run = subprocess.run([sys.executable, "-c", _CHILD.format(num=num, den=den)], cwd=R.os.path.dirname(R.os.path.dirname(R.os.path.abspath(__file__))),
                         capture_output=True, text=True)
    assert "calling" in run.stdout and "returned" not in run.stdout and run.returncode != 0, (run.returncode, run.stdout, run.stderr[-500:])
    assert "Assertion failed" in run.stderr and what in run.stderr, run.stderr[-800:]
