"""GPU: FRI over the wide fields -- Goldilocks, its quadratic extension, stark252 and the scalar fields of BN254, BLS12-381 and
BLS12-377: the fold kernel alone against Python integers (the sizes at which every launch shape runs, both domain sizes, directed
operands in the first lanes, host / device / unaligned operands), the refusals, the prover against every proof of the reference
(tests/golden/fri_vectors_wide.json) slot by slot and against the model (tests/fri_model_wide.py) at sizes whose trees cross the
single-launch top of the Merkle build, the verifier on the reference's proofs and on wrong ones, and the Python round trip."""
import contextlib
import ctypes
import random

import numpy as np
import pytest

from tests import blake_model as bm
from tests import fri_model_wide as fw

pytestmark = pytest.mark.gpu

CASES = fw.load_fixtures()
CASE_IDS = [c["name"] for c in CASES]
KIND_IDS = [fw.prefix(f, e) for f, e in fw.KINDS]
INVALID_POINTER, INVALID_ARGUMENT = 3, 11


@contextlib.contextmanager
def domain(field, logn):
    """the field's NTT domain of 2^logn points for the body (an earlier module's domain would silently win over init_domain)"""
    from icicle_amd import ntt

    ntt.release_domain(field)
    ntt.init_domain(field, ntt.get_root_of_unity(field, 1 << logn))
    try:
        yield
    finally:
        ntt.release_domain(field)


def hasher(name, chunk=0):
    from icicle_amd.hash import Hasher

    return getattr(Hasher, name)(chunk)


def to_array(F, elems):
    return np.frombuffer(F.raw(elems), dtype=np.uint32).reshape(-1, F.words).copy()


# ---- the fold alone ---------------------------------------------------------------------------------------------------------------------
# h = 1 (the wrapping twiddle alone), h = 2, the first full vector lane of Goldilocks scalars (h = 4), under a block, several blocks
FOLD_SIZES = [2, 4, 8, 1 << 6, 1 << 12]


def fold_inputs(F, n, rng):
    """n random elements with directed (lo, hi) pairs in the first lanes: 0, 1, p - 1, (p +- 1)/2, lo == hi, lo == -hi"""
    p, c = F.p, F.coeffs
    e = [tuple(rng.randrange(p) for _ in range(c)) for _ in range(n)]
    h = n // 2
    x = tuple(rng.randrange(p) for _ in range(c))
    el = lambda v: (v,) * c
    pairs = [(el(0), el(p - 1)), (el(p - 1), el(p - 1)), (el(p - 1), el(0)), (el(0), el(0)), (el((p + 1) // 2), el((p - 1) // 2)), (el(1), el(p - 1)),
             (x, x), (x, F.sub(el(0), x)), (el((p - 1) // 2), el((p + 1) // 2)), (el(1), el(1))]
    if c == 2:
        pairs += [((p - 1, 0), (0, p - 1)), ((0, 1), (p - 1, 0))]  # one coefficient zero
    for i, (lo, hi) in enumerate(pairs[:h]):
        e[i], e[i + h] = lo, hi
    return e


def alphas_for(F, rng):
    p, c = F.p, F.coeffs
    a = [(0,) * c, (1,) + (0,) * (c - 1), (p - 1,) * c, tuple(rng.randrange(p) for _ in range(c))]
    if c == 2:
        a += [(rng.randrange(p), 0), (0, p - 1)]
    return a


@pytest.mark.parametrize("field,ext", fw.KINDS, ids=KIND_IDS)
def test_fold_against_python_integers(hip, field, ext):
    from icicle_amd import fri
    from icicle_amd._lib import lib, check
    from icicle_amd.runtime import DeviceVec

    F = fw.Field(field, ext)
    rng = random.Random(13)
    cases = [(n, fold_inputs(F, n, rng)) for n in FOLD_SIZES]
    alphas = alphas_for(F, rng)
    want = {(n, a): to_array(F, F.fold(e, a)) for n, e in cases for a in alphas}
    fold = getattr(lib, f"{fw.prefix(field, ext)}_hip_fri_fold")
    for n, e in cases:
        x = to_array(F, e)
        logn = n.bit_length() - 1
        for log_domain in (logn, logn + 4):  # the domain equal to n (twiddle stride 1) and 2^4 times larger (stride 16), at every size
            with domain(field, log_domain):
                for a in alphas:
                    got = fri.fri_fold(field, x, to_array(F, [a]), extension=ext)
                    assert np.array_equal(got, want[n, a]), (log_domain, n, a, "host")
                # device operands: 16-byte aligned, one element further (8 bytes off a 16-byte boundary for Goldilocks scalars), and
                # one word further (the word-by-word path of every kind)
                a = alphas[3]
                for shift in (0, F.bytes, 4):
                    d_in, d_out, d_alpha = DeviceVec(x.nbytes + 32), DeviceVec(x.nbytes // 2 + 32), DeviceVec.from_host(to_array(F, [a]))
                    check(lib.icicle_copy_to_device(d_in.ptr + shift, x.ctypes.data, x.nbytes))
                    check(lib.icicle_memset(d_out.ptr, 0xEE, d_out.nbytes))
                    check(fold(d_in.ptr + shift, n, d_alpha.ptr, d_out.ptr + shift, True, None))
                    hip.runtime.device_synchronize()
                    raw = d_out.to_host(np.uint32)
                    s, m = shift // 4, x.size // 2
                    assert np.array_equal(raw[s:s + m], want[n, a].reshape(-1)), (log_domain, n, "device", shift)
                    assert np.all(raw[:s] == 0xEEEEEEEE) and np.all(raw[s + m:] == 0xEEEEEEEE), "the fold wrote outside its output"


@pytest.mark.parametrize("field,ext", fw.KINDS, ids=KIND_IDS)
def test_refusals(hip, field, ext):
    """With a domain of 2^5 points a well-formed prove and fold of 32 elements succeed, so each refusal below is the argument's"""
    from icicle_amd import FriConfig, FriProof, FriTranscriptConfig, ntt
    from icicle_amd._lib import lib

    F, prefix = fw.Field(field, ext), fw.prefix(field, ext)
    prove, fold = getattr(lib, prefix + "_fri_merkle_tree_prove"), getattr(lib, prefix + "_hip_fri_fold")
    th, leaves, compress = hasher("keccak256"), hasher("blake2s", F.bytes), hasher("blake2s", 64)
    ffi, keep = FriTranscriptConfig.new_default_labels(th, 1)._ffi(ext, field)
    rng = random.Random(3)
    data = to_array(F, [tuple(rng.randrange(F.p) for _ in range(F.coeffs)) for _ in range(64)])
    proof = FriProof(field, ext)
    c = FriConfig.default()
    c.nof_queries, c.pow_bits = 4, 4

    def run(n=32, lh=leaves, d=data.ctypes.data, t=ffi, pr=proof):
        return prove(ctypes.byref(c), ctypes.byref(t) if t is not None else None, d, n, lh.handle if lh else None, compress.handle, 0, pr.handle if pr else None)

    out, alpha = np.zeros_like(data), to_array(F, [(1,) * F.coeffs])
    fold_of = lambda n, i=data.ctypes.data, a=alpha.ctypes.data, o=out.ctypes.data: fold(i, n, a, o, False, None)
    ntt.release_domain(field)
    assert run() == INVALID_ARGUMENT and fold_of(32) == INVALID_ARGUMENT  # no domain on this device
    with domain(field, 5):
        assert run() == 0 and proof.nof_queries == 8 and proof.nof_rounds == 5
        for n_bad in (0, 3, 24, 48, 64):  # no power of two; 64: beyond the domain
            assert run(n=n_bad) == INVALID_ARGUMENT, n_bad
        for bad_leaves in (hasher("blake2s", F.bytes + 4), hasher("blake2s", F.bytes // 2), hasher("blake2s", 2 * F.bytes), hasher("blake2s", 0)):
            assert run(lh=bad_leaves) == INVALID_ARGUMENT  # a leaf is one element of 8, 16 or 32 bytes
        assert run(d=None) == INVALID_POINTER and run(t=None) == INVALID_POINTER and run(lh=None) == INVALID_POINTER and run(pr=None) == INVALID_POINTER
        assert proof.nof_queries == 8 and proof.nof_rounds == 5, "a refused call changed the proof"
        assert fold_of(32) == 0
        for n_bad in (0, 1, 3, 24, 64):
            assert fold_of(n_bad) == INVALID_ARGUMENT, n_bad
        assert fold_of(32, i=None) == INVALID_POINTER and fold_of(32, a=None) == INVALID_POINTER and fold_of(32, o=None) == INVALID_POINTER
    with domain(field, 4):  # smaller than n
        assert run() == INVALID_ARGUMENT and fold_of(32) == INVALID_ARGUMENT
        # the device is still usable, and the answer is still right
        assert fold_of(16) == 0
        assert np.array_equal(out[:8], to_array(F, F.fold(F.elements(data[:16].tobytes()), (1,) * F.coeffs)))
    del keep


# ---- prove ------------------------------------------------------------------------------------------------------------------------------
def transcript_of(F, proto, th):
    from icicle_amd import FriTranscriptConfig

    _, labels, public, seed = proto[:4]
    return FriTranscriptConfig(th, *labels, public, np.frombuffer(F.to_bytes(seed), dtype=np.uint32))


def config_of(sd, pow_bits, nq):
    from icicle_amd import FriConfig

    c = FriConfig.default()
    c.stopping_degree, c.pow_bits, c.nof_queries = sd, pow_bits, nq
    return c


def hashers_of(F, transcript_hash, leaves_hash, compress_hash):
    return hasher(transcript_hash), hasher(leaves_hash, F.bytes), hasher(compress_hash, 2 * bm.OUT_SIZE[compress_hash])


def read_proof(F, proof):
    """the device's proof in the model's form"""
    return {"final_poly": F.elements(proof.final_poly.tobytes()), "nonce": proof.pow_nonce,
            "slots": [[(mp.leaf_idx, mp.leaf, mp.root, mp.path) for mp in row] for row in proof.slots()]}


def assert_same_proof(got, want, what):
    assert got["final_poly"] == want["final_poly"], what
    assert got["nonce"] == want["nonce"], what
    assert len(got["slots"]) == len(want["slots"]), what
    for q, (g, w) in enumerate(zip(got["slots"], want["slots"])):
        assert len(g) == len(w), (what, q)
        for r, (a, b) in enumerate(zip(g, w)):
            assert a == b, (what, "slot", q, "round", r)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_prove_equals_the_reference(hip, case):
    import icicle_amd
    from icicle_amd.runtime import DeviceVec

    F, proto, want = fw.case_field(case), fw.case_protocol(case), fw.case_proof(case)
    x = to_array(F, fw.case_elements(case))
    th, lh, ch = hashers_of(F, case["transcript_hash"], case["leaves_hash"], case["compress_hash"])
    cfg = lambda: config_of(case["stopping_degree"], case["pow_bits"], case["nof_queries"])
    with domain(case["field"], case["log_domain"]):
        for from_device, min_layer in ((False, 0), (True, 0), (False, 2), (True, 2)):
            data = DeviceVec.from_host(x) if from_device else x
            proof = icicle_amd.fri_merkle_tree_prove(case["field"], cfg(), transcript_of(F, proto, th), data, lh, ch, min_layer, extension=F.ext)
            if from_device:
                assert np.array_equal(data.to_host(np.uint32), x.reshape(-1)), "prove changed its input"
            assert proof.nof_queries == 2 * case["nof_queries"] and proof.nof_rounds == len(want["slots"][0]) and proof.final_poly_size == case["stopping_degree"] + 1
            assert_same_proof(read_proof(F, proof), want, (from_device, min_layer))
            assert icicle_amd.fri_merkle_tree_verify(case["field"], cfg(), transcript_of(F, proto, th), proof, lh, ch, extension=F.ext)


BIG = [  # one per element size -- field, extension, log n, tree hashers, transcript hasher, stopping degree
    ("goldilocks", False, 12, ("blake2s", "blake2s"), "sha3_512", 3),
    ("goldilocks", True, 12, ("keccak256", "keccak256"), "keccak256", 0),
    ("stark252", False, 10, ("sha3_256", "sha3_256"), "blake2s", 1),
]


@pytest.mark.parametrize("field,ext,logn,trees,th_name,sd", BIG, ids=[f"{fw.prefix(b[0], b[1])}_2^{b[2]}_{b[3][1]}" for b in BIG])
def test_prove_equals_the_model_beyond_the_single_launch_top(hip, field, ext, logn, trees, th_name, sd):
    import icicle_amd

    F = fw.Field(field, ext)
    rng = random.Random(logn)
    elems = [tuple(rng.randrange(F.p) for _ in range(F.coeffs)) for _ in range(1 << logn)]
    proto = (th_name, (b"ds", b"round", b"commit", b"nonce"), b"big", (3,) + (0,) * (F.coeffs - 1), trees[0], trees[1], sd, 8, 20)
    want = fw.prove(F, elems, *proto)
    th, lh, ch = hashers_of(F, th_name, *trees)
    with domain(field, logn):
        proof = icicle_amd.fri_merkle_tree_prove(field, config_of(sd, 8, 20), transcript_of(F, proto, th), to_array(F, elems), lh, ch, 0, extension=ext)
        assert_same_proof(read_proof(F, proof), want, "model")
        assert icicle_amd.fri_merkle_tree_verify(field, config_of(sd, 8, 20), transcript_of(F, proto, th), proof, lh, ch, extension=ext)


# ---- verify -------------------------------------------------------------------------------------------------------------------------------
def rebuild(case, pr):
    """a device proof from the model's form, through create_with_arguments"""
    from icicle_amd import FriProof
    from icicle_amd.merkle import MerkleProof

    rows = [[MerkleProof.with_data(False, idx, leaf, root, path) for idx, leaf, root, path in row] for row in pr["slots"]]
    fp = np.frombuffer(b"".join(pr["final_poly"]), dtype=np.uint32)
    return FriProof.create_with_arguments(case["field"], rows, fp, pr["nonce"], extension=case["extension"])


def flip_first_bit(b: bytes) -> bytes:
    return bytes([b[0] ^ 1]) + b[1:]


def not_below_p(F, raw: bytes) -> bytes:
    """the element with its first coefficient at or above p: the same residue where x + p fits the coefficient's bytes, else all ones"""
    x = int.from_bytes(raw[:F.coeff_bytes], "little")
    v = x + F.p if x + F.p < 1 << (8 * F.coeff_bytes) else (1 << (8 * F.coeff_bytes)) - 1
    return v.to_bytes(F.coeff_bytes, "little") + raw[F.coeff_bytes:]


def wrong_proofs(case):
    """(what, proof with the final polynomial as a list of the elements' bytes)"""
    F = fw.case_field(case)

    def base():
        pr = fw.case_proof(case)
        pr["final_poly"] = [F.to_bytes(e) for e in pr["final_poly"]]
        return pr

    pr = base()
    k = pr["slots"][0][-1][0] % len(pr["final_poly"])  # the coefficient the first query reads: q % final_size
    pr["final_poly"][k] = flip_first_bit(pr["final_poly"][k])
    yield "final polynomial bit", pr
    for what, pos in (("leaf bit", 1), ("root bit", 2)):
        pr = base()
        row = list(pr["slots"][2][1])
        row[pos] = flip_first_bit(row[pos])
        pr["slots"][2][1] = tuple(row)
        yield what, pr
    if case["pow_bits"]:  # without a proof of work the nonce is not part of the transcript
        pr = base()
        pr["nonce"] ^= 1
        yield "nonce bit", pr
    for k in range(len(base()["final_poly"])):
        pr = base()
        pr["final_poly"][k] = not_below_p(F, pr["final_poly"][k])
        yield f"final polynomial element {k} at or above p", pr
    pr = base()
    idx, leaf, root, path = pr["slots"][0][0]
    pr["slots"][0][0] = (idx, not_below_p(F, leaf), root, path)
    yield "leaf at or above p", pr


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_verify_accepts_the_reference_and_rejects_wrong_proofs(hip, case):
    import icicle_amd

    F, proto = fw.case_field(case), fw.case_protocol(case)
    th, lh, ch = hashers_of(F, case["transcript_hash"], case["leaves_hash"], case["compress_hash"])

    def verify(pr):
        cfg = config_of(case["stopping_degree"], case["pow_bits"], case["nof_queries"])
        return icicle_amd.fri_merkle_tree_verify(case["field"], cfg, transcript_of(F, proto, th), rebuild(case, pr), lh, ch, extension=F.ext)  # raises unless SUCCESS

    good = fw.case_proof(case)
    good["final_poly"] = [F.to_bytes(e) for e in good["final_poly"]]
    assert verify(good) is True  # verification needs no NTT domain: w_n comes from the field's own root of unity
    for what, pr in wrong_proofs(case):
        assert verify(pr) is False, what


# ---- the Python round trip ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field,ext", fw.KINDS, ids=KIND_IDS)
def test_python_round_trip(hip, field, ext):
    """verify(prove(x)) through icicle_amd/fri.py with the default labels and an integer seed, from the host and from the device"""
    import icicle_amd
    from icicle_amd.runtime import DeviceVec

    F = fw.Field(field, ext)
    rng = random.Random(21)
    x = to_array(F, [tuple(rng.randrange(F.p) for _ in range(F.coeffs)) for _ in range(1 << 9)])
    th, lh, ch = hashers_of(F, "keccak256", "keccak256", "keccak256")
    tc = icicle_amd.FriTranscriptConfig.new_default_labels(th, F.p - 1)
    assert tc.seed_words(ext, field) == list(np.frombuffer(F.to_bytes((F.p - 1,) + (0,) * (F.coeffs - 1)), dtype=np.uint32))
    with domain(field, 10):
        for data in (x, DeviceVec.from_host(x)):
            proof = icicle_amd.fri_merkle_tree_prove(field, config_of(1, 10, 30), tc, data, lh, ch, 0, extension=ext)
            assert (proof.nof_queries, proof.nof_rounds, proof.final_poly_size) == (60, 8, 2) and proof.final_poly.shape == (2, F.words)
            assert icicle_amd.fri_merkle_tree_verify(field, config_of(1, 10, 30), tc, proof, lh, ch, extension=ext)
            assert not icicle_amd.fri_merkle_tree_verify(field, config_of(1, 10, 30), icicle_amd.FriTranscriptConfig.new_default_labels(th, F.p - 2), proof, lh, ch, extension=ext)
