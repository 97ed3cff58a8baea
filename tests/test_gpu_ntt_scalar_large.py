"""GPU: the 256-bit and Goldilocks NTT (icicle_amd/csrc/ntt_big.hip k_big_ntt_pass) above 2^17, on EVERY output element.

The reference CPU backend needs minutes for a 256-bit domain of 2^25, so nothing here is compared with it above 2^17. Instead
tests/ntt_identity.py checks a whole transform on the device: sum_k r^k X[k] = (1 - r^n) sum_j x_j g^j / (1 - r w^j) at a seeded r,
both sides computed with vector operations that share no code with the NTT kernel, each kept inside the size at which the suite compares
it with the reference (see that module). Inputs are generated on the device (seeded torch.Generator); nothing of size n crosses to the
host above 2^17. Every case initialises the domain at exactly its size and releases it, with its tensors, when it ends.

What the sizes reach (ntt_plan.h split_logn(logn, 8)): 20, 21 and 24: 7,7,6 / 7,7,7 / 8,8,8 (128- and 256-row tiles inside a three-pass
plan); 25: 9,8,8, the first 512-row pass -- for a 256-bit field an LDS tile of exactly 72 KiB with 512 threads; 26 and 27: 9,9,8 and
9,9,9, a second non-last nine-stage pass and the natural-order scatter with n0 = 512; goldilocks 28: 10,9,9, the 1024-row pass, where the
radix-16 loop splits 4 + 4 + 2 stages (4 + 4 + 1 at nine) and a thread's geometric store progression makes 16 trips.

(a) the checker itself: at 2^17, where tests/test_gpu_ntt_scalar.py and test_gpu_goldilocks.py byte-compare this kernel with the reference,
    the transform equals the reference, the checker accepts it, and rejects it with 1 added to one word of one output (first element, an
    element of the last tile, a seeded one); the rejection again at 2^25, through the sliced path.
(b) forward kNN on every output, then the inverse round trip. (c) kNR / kRN against bit_reverse, in place, and cosets. (d) batch rows
and columns_batch against the single transform. (e) inputs with closed-form transforms that push the lazy bounds: all p - 1, p - 1 at the
even indices, a single p - 1 at index 1, both directions, compared in full.

LEFT OUT ON PURPOSE: a 256-bit transform at 2^28 -- the only place where a 256-bit field runs a TEN-stage pass. It needs 8 GiB per
buffer, with the twiddle table, the work buffer, the output and the checker's vectors on top. The ten-stage lazy bound of the 256-bit
fields ("<= 23.2 p after ten stages", header of ntt_big.hip) therefore still rests on that comment's arithmetic alone; nine stages
(21.2 p) are run here at 2^25 .. 2^27, ten stages only with goldilocks' exact arithmetic. bn254 at 2^27 holds 4 GiB per vector: the
checker's vectors are freed as soon as each is consumed.

Time: the whole module takes about 5 s; see MEASURED below, with the suite's time before and after."""
import contextlib
import ctypes
import random

import numpy as np
import pytest

from oracle import pyref, ref
from tests import ntt_identity as I

pytestmark = pytest.mark.gpu
# MEASURED on an MI355X (one run each): this module alone 31 tests in 4.5 s of pytest (6.5 s wall). The slowest: the 2^17 anchor with
# the reference's CPU transform 0.63 s (+ 1.35 s of session setup), bn254 2^27 forward 0.42 s, goldilocks 2^28 forward 0.22 s, bn254 2^26
# 0.21 s, the bn254 2^27 closed forms 0.17 s, orderings and cosets at bn254 2^25 0.16 s; every other test under 0.15 s. The doubling loop
# and the sliced element-wise calls (2048 vector_inv calls at 2^27) cost less than the random input. No case was dropped.
# The whole GPU suite with this module: 1668 passed, 11 skipped in 714.9 s (718 s wall). Without it (the parent's GPU tests; the library
# differs from the parent's only in where big_ntt_run's launch geometry is computed): 1637 passed, 11 skipped in 855.7 s (859 s wall) --
# on another machine of the pool, whose host was slower that hour (session setup 81.7 s against 36.7 s, the reference-CPU legs 10 - 25 %
# longer): the 140 s between the two runs are the machines, this module's share is its 5 s.

GOLD = "goldilocks"


class Case:
    """one test's domain and tensors; everything it holds is dropped when the case ends"""

    def __init__(self, hip, field, logn):
        import torch
        from icicle_amd import ntt as N, vecops as V

        self.hip, self.N, self.V, self.torch = hip, N, V, torch
        self.field, self.logn, self.n = field, logn, 1 << logn
        self.F = pyref.NTT_FIELDS[field]
        self.p, self.w = self.F.p, I.WORDS[field]
        self.dev = torch.device("cuda", 0)
        self.t = {}  # the case's tensors, by name

    def gen(self, seed):
        return self.torch.Generator(device=self.dev).manual_seed(seed)

    def random(self, count, seed):
        return I.random_elements(self.field, self.p, count, self.gen(seed), self.dev)

    def cfg(self, ordering=0, coset=1, batch=1, columns=False):
        c = self.hip.NTTConfigU64.default() if self.field == GOLD else self.hip.NTTConfigU256.default()
        c.ordering, c.batch_size, c.columns_batch = ordering, batch, columns
        c.set_coset_gen(coset)
        return c

    def ntt(self, src, direction, dst=None, extension=False, **kw):
        """a transform of device tensors; dst None: a new tensor"""
        if dst is None:
            dst = self.torch.empty_like(src)
        self.N.ntt(self.field, src.data_ptr(), direction, self.cfg(**kw), out=dst.data_ptr(), size=self.n, extension=extension)
        return dst

    def bit_reverse(self, src):
        dst = self.torch.empty_like(src)
        self.V.bit_reverse(self.field, src.data_ptr(), self.hip.VecOpsConfig.default(), out=dst.data_ptr(), size=self.n)
        return dst

    def checker(self, seed):
        return I.Checker(self.field, self.F, self.logn, seed, self.dev)

    def coset_gen(self, seed):
        g = random.Random(seed).randrange(2, self.p)
        assert pow(g, self.n, self.p) != 1  # not a power of w
        return g


@contextlib.contextmanager
def case(hip, field, logn):
    c = Case(hip, field, logn)
    root = c.N.get_root_of_unity(field, 1 << logn)
    assert root == pyref.omega(c.F, logn)
    c.N.init_domain(field, root)
    try:
        yield c
    finally:
        c.N.release_domain(field)
        c.t.clear()
        c.torch.cuda.empty_cache()


# ---- (a) the checker is itself checked ---------------------------------------------------------------------------------------------------
def _mutations(c, X, ck, x, g=1):
    """1 added to one word of one output element: the identity alone (not the canonical test) must notice"""
    rng = random.Random(1700 + c.logn)
    for pos, word in ((0, 0), (c.n - 3, c.w - 1), (rng.randrange(c.n), rng.randrange(c.w))):
        X[pos, word] += 1
        lhs, rhs = ck.sides(x, X, g)
        assert lhs != rhs, (c.field, c.logn, pos, word)
        assert not ck.accepts(x, X, g)
        if pos == 0:  # the failure message's direct evaluation of sampled outputs names this one (digits 0, 0, 0)
            assert "k = 0, digits (k0, k1, k2) = (0, 0, 0)" in ck.triage(x, X, g)
        X[pos, word] -= 1
    assert ck.accepts(x, X, g)
    assert "are right" in ck.triage(x, X, g)


@pytest.mark.parametrize("field", ["bn254", GOLD])
def test_checker_agrees_with_the_reference_at_2_17_and_rejects_one_changed_word(hip, field):
    logn = 17
    rf = ref.RefGoldField() if field == GOLD else ref.RefScalarNttField(field)
    with case(hip, field, logn) as c:
        t = c.t
        t["x"] = c.random(c.n, 1701)
        t["X"] = c.ntt(t["x"], c.N.FORWARD)
        rf.init_domain(rf.get_root_of_unity(c.n))
        try:
            want = rf.ntt(np.ascontiguousarray(t["x"].cpu().numpy().view(np.uint32).reshape(-1)), c.n, 0)
        finally:
            rf.release_domain()
        assert np.array_equal(t["X"].cpu().numpy().view(np.uint32).reshape(-1), want)
        ck = c.checker(1702)
        try:
            ck.check(t["x"], t["X"], what="kNN forward")
            _mutations(c, t["X"], ck, t["x"])
            # an element of value p (the identity cannot see X[k] + p) is refused by the word comparison, on the device as on the CPU
            # (tests/test_ntt_identity_cpu.py has the directed cases)
            t["X"][c.n // 2] = I.element_tensor(c.p, c.w, c.dev)
            assert not I.canonical(t["X"], c.p) and not ck.accepts(t["x"], t["X"])
        finally:
            ck.release()


@pytest.mark.parametrize("field", ["bn254", GOLD])
def test_checker_rejects_one_changed_word_at_2_25(hip, field):
    """the sliced path: 32 rows of 2^20 for poly_eval and vector_sum, 512 slices of vector_inv"""
    with case(hip, field, 25) as c:
        t = c.t
        t["x"] = c.random(c.n, 1711)
        t["X"] = c.ntt(t["x"], c.N.FORWARD)
        ck = c.checker(1712)
        try:
            ck.check(t["x"], t["X"], what="kNN forward")
            _mutations(c, t["X"], ck, t["x"])
        finally:
            ck.release()


# ---- (b) forward kNN on every output, then the inverse round trip ------------------------------------------------------------------------
FORWARD_CASES = [("bn254", 20), ("bn254", 24), ("bn254", 25), ("bn254", 26), ("bn254", 27), ("bls12_381", 21), ("bls12_377", 21), ("stark252", 21),
                 (GOLD, 20), (GOLD, 24), (GOLD, 25), (GOLD, 26), (GOLD, 27), (GOLD, 28)]


@pytest.mark.parametrize("field,logn", FORWARD_CASES)
def test_forward_on_every_output_then_round_trip(hip, field, logn):
    with case(hip, field, logn) as c:
        t = c.t
        t["x"] = c.random(c.n, 1800 + logn)
        t["X"] = c.ntt(t["x"], c.N.FORWARD)
        ck = c.checker(1900 + logn)
        try:
            ck.check(t["x"], t["X"], what="kNN forward")
        finally:
            ck.release()
        t["back"] = c.ntt(t["X"], c.N.INVERSE)
        assert c.torch.equal(t["back"], t["x"]), (field, logn, "inverse of forward")


def test_goldilocks_extension_per_component_at_2_25(hip):
    """the quadratic extension transforms its two components with the base field's twiddles (lanes = 2 in the kernel): each component
    of the output, as a strided copy, is the base-field transform of that component of the input"""
    with case(hip, GOLD, 25) as c:
        t = c.t
        t["x"] = c.random(2 * c.n, 1725).reshape(c.n, 2, c.w)  # [element, component, word]
        t["X"] = c.ntt(t["x"], c.N.FORWARD, extension=True)
        ck = c.checker(1726)
        try:
            for comp in (0, 1):
                t["xc"], t["Xc"] = t["x"][:, comp, :].contiguous(), t["X"][:, comp, :].contiguous()
                ck.check(t["xc"], t["Xc"], what=f"extension component {comp}")
        finally:
            ck.release()
        t["back"] = c.ntt(t["X"], c.N.INVERSE, extension=True)
        assert c.torch.equal(t["back"], t["x"])


# ---- (c) orderings and cosets ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn", [20, 25])
@pytest.mark.parametrize("field", ["bn254", GOLD])
def test_orderings_and_cosets(hip, field, logn):
    with case(hip, field, logn) as c:
        t, N, eq = c.t, c.N, c.torch.equal
        t["x"] = c.random(c.n, 2000 + logn)
        t["X"] = c.ntt(t["x"], N.FORWARD)
        ck = c.checker(2100 + logn)
        try:
            ck.check(t["x"], t["X"], what="kNN forward")
            # kNR output = bit_reverse of the checked kNN output
            t["Xr"] = c.bit_reverse(t["X"])
            t["y"] = c.ntt(t["x"], N.FORWARD, ordering=N.kNR)
            assert eq(t["y"], t["Xr"]), "kNR forward"
            # kRN of the bit-reversed input = kNN of the input, both directions
            t["xr"] = c.bit_reverse(t["x"])
            c.ntt(t["xr"], N.FORWARD, dst=t["y"], ordering=N.kRN)
            assert eq(t["y"], t["X"]), "kRN forward"
            c.ntt(t["Xr"], N.INVERSE, dst=t["y"], ordering=N.kRN)
            assert eq(t["y"], t["x"]), "kRN inverse"
            del t["xr"]
            # kNR forward, then kRN inverse, in place
            t["y"].copy_(t["x"])
            c.ntt(t["y"], N.FORWARD, dst=t["y"], ordering=N.kNR)
            assert eq(t["y"], t["Xr"]), "kNR forward in place"
            c.ntt(t["y"], N.INVERSE, dst=t["y"], ordering=N.kRN)
            assert eq(t["y"], t["x"]), "kNR forward + kRN inverse in place"
            del t["Xr"]
            # a coset: the coset form of the identity, and the inverse returns x
            g = c.coset_gen(2200 + logn)
            c.ntt(t["x"], N.FORWARD, dst=t["X"], coset=g)
            ck.check(t["x"], t["X"], g, what="coset forward")
            c.ntt(t["X"], N.INVERSE, dst=t["y"], coset=g)
            assert eq(t["y"], t["x"]), "coset inverse"
        finally:
            ck.release()


# ---- (d) layouts -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn", [20, 25])
@pytest.mark.parametrize("field", ["bn254", GOLD])
def test_batch_rows_and_columns_equal_the_single_transform(hip, field, logn):
    """(the single kNN transform at these sizes is checked on every output above)"""
    with case(hip, field, logn) as c:
        t, N, eq = c.t, c.N, c.torch.equal
        t["x"] = c.random(2 * c.n, 2300 + logn).reshape(2, c.n, c.w)
        t["Y"] = c.ntt(t["x"], N.FORWARD, batch=2)
        for row in (0, 1):
            t["one"] = c.ntt(t["x"][row], N.FORWARD)
            assert eq(t["Y"][row], t["one"]), (field, logn, "row", row)
        t["xc"] = t["x"].reshape(c.n, 2, c.w)  # the same words read as two interleaved columns, element stride 2
        c.ntt(t["xc"], N.FORWARD, dst=t["Y"], batch=2, columns=True)
        Yc = t["Y"].reshape(c.n, 2, c.w)
        for col in (0, 1):
            t["col"] = t["xc"][:, col, :].contiguous()
            c.ntt(t["col"], N.FORWARD, dst=t["one"])
            assert eq(Yc[:, col, :], t["one"]), (field, logn, "column", col)


# ---- (e) inputs that push the lazy bounds ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field,logn", [("bn254", 8), ("bn254", 25), ("bn254", 27), (GOLD, 28)])
def test_structured_inputs_against_their_closed_forms(hip, field, logn):
    """all p - 1: X[0] = n (p - 1), else 0. p - 1 at even indices: X[0] = X[n / 2] = (n / 2)(p - 1), else 0. A single p - 1 at index 1:
    X[k] = -w^k. Inverse: the same with w^-1 and a factor 1 / n. Random inputs keep the lazy butterflies near the middle of their range;
    these put every operand of the first stages at p - 1 (2^8 is the one-pass anchor of tests/test_gpu_ntt_scalar.py)."""
    with case(hip, field, logn) as c:
        t, N, torch = c.t, c.N, c.torch
        p, n, w = c.p, c.n, c.w
        top = I.element_tensor(p - 1, w, c.dev)
        ninv = pow(n, -1, p)
        omega = N.get_root_of_unity_from_domain(field, logn)
        assert omega == pyref.omega(c.F, logn)
        t["x"] = torch.empty((n, w), dtype=torch.int32, device=c.dev)
        t["X"] = torch.empty_like(t["x"])
        t["want"] = torch.empty_like(t["x"])

        def sparse(values):
            t["want"].zero_()
            for k, v in values.items():
                t["want"][k] = I.element_tensor(v % p, w, c.dev)

        for direction, scale in ((N.FORWARD, 1), (N.INVERSE, ninv)):
            t["x"][:] = top
            c.ntt(t["x"], direction, dst=t["X"])
            sparse({0: n * (p - 1) * scale})
            assert torch.equal(t["X"], t["want"]), (field, logn, direction, "all p - 1")
            t["x"][1::2] = 0
            c.ntt(t["x"], direction, dst=t["X"])
            sparse({0: (n // 2) * (p - 1) * scale, n // 2: (n // 2) * (p - 1) * scale})
            assert torch.equal(t["X"], t["want"]), (field, logn, direction, "p - 1 at even indices")
            t["x"].zero_()
            t["x"][1] = top
            c.ntt(t["x"], direction, dst=t["X"])
            del t["want"]
            base = omega if direction == N.FORWARD else pow(omega, -1, p)
            t["want"] = I.progression(field, p, n, -scale, base, c.dev)  # -w^k (forward), -w^-k / n (inverse): the doubling vector
            assert torch.equal(t["X"], t["want"]), (field, logn, direction, "a single p - 1 at index 1")
