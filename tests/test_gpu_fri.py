"""GPU: FRI over BabyBear and KoalaBear, scalar and quartic extension -- the fold kernel alone against Python integers (sizes at
which every launch shape runs, both domain sizes, operands at the ends of the range, host / device / unaligned operands), the
prover against every proof of the reference (tests/golden/fri_vectors.json) slot by slot and against the model (tests/fri_model.py)
at sizes whose trees cross the single-launch top of the Merkle build, the verifier on its own proofs, the reference's proofs and
seven kinds of wrong proof, and the reference's Rust tests replayed (wrappers/rust/icicle-core/src/fri/tests.rs)."""
import contextlib
import random

import numpy as np
import pytest

from tests import fri_model as fm

pytestmark = pytest.mark.gpu

CASES = fm.load_fixtures()
FIELD_KINDS = [(f, e) for f in ("babybear", "koalabear") for e in (False, True)]
KIND_IDS = [f"{f}{'_ext' if e else ''}" for f, e in FIELD_KINDS]


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
    a = np.array(elems, dtype=np.uint32)
    return a if F.ext else a.reshape(-1)


# ---- the fold alone ---------------------------------------------------------------------------------------------------------------------
FOLD_SIZES = [2, 4, 8, 16, 64, 1 << 10, 1 << 13]  # h = 1, 2, one vector of scalars, under a block, several blocks


def fold_inputs(F, n, rng):
    """n elements: random ones, with 0 and p - 1 at both halves' ends, where i = 0 (w^0) and i = h - 1 meet them"""
    e = [tuple(rng.randrange(F.p) for _ in range(F.words)) for _ in range(n)]
    h = n // 2
    zero, top = (0,) * F.words, (F.p - 1,) * F.words
    e[0], e[h] = zero, top
    if n >= 4:
        e[h - 1], e[n - 1] = top, top
    if n >= 8:
        e[1], e[h + 1] = top, zero
        e[2], e[h + 2] = zero, zero
    return e


def alphas_for(F, rng):
    p = F.p
    return [(0,) * F.words, (1,) + (0,) * (F.words - 1), (p - 1,) * F.words, tuple(rng.randrange(p) for _ in range(F.words))]


@pytest.mark.parametrize("field,ext", FIELD_KINDS, ids=KIND_IDS)
def test_fold_against_python_integers(hip, field, ext):
    from icicle_amd import fri
    from icicle_amd._lib import lib, check
    from icicle_amd.runtime import DeviceVec

    F = fm.Field(field, ext)
    rng = random.Random(11)
    cases = [(n, fold_inputs(F, n, rng)) for n in FOLD_SIZES]
    alphas = alphas_for(F, rng)
    want = {(n, a): to_array(F, F.fold(e, a)) for n, e in cases for a in alphas}
    fold = getattr(lib, f"{field}{'_extension' if ext else ''}_hip_fri_fold")
    for n, e in cases:
        x = to_array(F, e)
        logn = n.bit_length() - 1
        for log_domain in (logn, logn + 4):  # the domain equal to n (twiddle stride 1) and 2^4 times larger (stride 16), at every size
            with domain(field, log_domain):
                for a in alphas:
                    got = fri.fri_fold(field, x, np.array(a, dtype=np.uint32), extension=ext)
                    assert np.array_equal(got, want[n, a]), (log_domain, n, a, "host")
                # device operands: aligned, and 4 bytes off a 16-byte boundary (the word-by-word path at every size)
                a = alphas[3]
                for shift in (0, 1):
                    d_in, d_out, d_alpha = DeviceVec(x.nbytes + 16), DeviceVec(x.nbytes // 2 + 16), DeviceVec.from_host(np.array(a, dtype=np.uint32))
                    check(lib.icicle_copy_to_device(d_in.ptr + 4 * shift, x.ctypes.data, x.nbytes))
                    check(lib.icicle_memset(d_out.ptr, 0xEE, d_out.nbytes))
                    check(fold(d_in.ptr + 4 * shift, n, d_alpha.ptr, d_out.ptr + 4 * shift, True, None))
                    hip.runtime.device_synchronize()
                    raw = d_out.to_host(np.uint32)
                    m = x.size // 2
                    assert np.array_equal(raw[shift:shift + m], want[n, a].reshape(-1)), (log_domain, n, "device", shift)
                    assert np.all(raw[:shift] == 0xEEEEEEEE) and np.all(raw[shift + m:] == 0xEEEEEEEE), "the fold wrote outside its output"


def test_fold_refuses_a_domain_that_is_too_small(hip):
    import icicle_amd
    from icicle_amd import fri

    x = np.zeros(64, dtype=np.uint32)
    with domain("babybear", 5):
        with pytest.raises(icicle_amd.IcicleError) as e:
            fri.fri_fold("babybear", x, np.array([1], dtype=np.uint32))
        assert e.value.code == 11
        assert fri.fri_fold("babybear", x[:32], np.array([1], dtype=np.uint32)).shape == (16,)


@pytest.mark.parametrize("field,ext", FIELD_KINDS, ids=KIND_IDS)
def test_argument_errors_under_a_domain(hip, field, ext):
    """With a domain of 2^5 points a well-formed prove and fold of 32 elements succeed, so each refusal below is the argument's"""
    import ctypes

    from icicle_amd import FriConfig, FriProof, FriTranscriptConfig
    from icicle_amd._lib import lib

    F = fm.Field(field, ext)
    prefix = f"{field}_extension" if ext else field
    prove, fold = getattr(lib, prefix + "_fri_merkle_tree_prove"), getattr(lib, prefix + "_hip_fri_fold")
    th, leaves, compress = hasher("keccak256"), hasher("blake2s", F.bytes), hasher("blake2s", 64)
    ffi, keep = FriTranscriptConfig.new_default_labels(th, 1)._ffi(ext)
    data = np.arange(64 * F.words, dtype=np.uint32)
    proof = FriProof(field, ext)

    def run(n=32, lh=leaves, ch=compress, **kw):
        c = FriConfig.default()
        c.nof_queries, c.pow_bits = 4, 4
        for k, v in kw.items():
            setattr(c, k, v)
        return prove(ctypes.byref(c), ctypes.byref(ffi), data.ctypes.data, n, lh.handle, ch.handle, 0, proof.handle)

    out, alpha = np.zeros_like(data), np.ones(4, dtype=np.uint32)
    with domain(field, 5):
        assert run() == 0 and proof.nof_queries == 8 and proof.nof_rounds == 5
        assert run(nof_queries=16) == 0 and run(stopping_degree=15) == 0 and run(pow_bits=0) == 0  # the last values accepted
        for bad in (dict(folding_factor=4), dict(folding_factor=0), dict(nof_queries=0), dict(nof_queries=17), dict(stopping_degree=2), dict(stopping_degree=31),
                    dict(stopping_degree=63), dict(pow_bits=61), dict(n=0), dict(n=3), dict(n=24), dict(n=64)):  # 64: beyond the domain
            assert run(**bad) == 11, bad
        for bad_compress in (hasher("blake2s", 32), hasher("blake2s", 128), hasher("keccak512", 64), hasher("blake2s", 0)):
            assert run(ch=bad_compress) == 11
        for bad_leaves in (hasher("blake2s", F.bytes + 4), hasher("blake2s", 20 - F.bytes), hasher("blake2s", 0)):
            assert run(lh=bad_leaves) == 11
        assert proof.nof_queries == 8 and proof.nof_rounds == 5, "a refused call changed the proof"
        assert fold(data.ctypes.data, 32, alpha.ctypes.data, out.ctypes.data, False, None) == 0
        for n_bad in (0, 1, 3, 24, 64):
            assert fold(data.ctypes.data, n_bad, alpha.ctypes.data, out.ctypes.data, False, None) == 11, n_bad
    with domain(field, 4):  # smaller than n
        assert run() == 11
        assert run(n=16, stopping_degree=0) == 0
    del keep


# ---- prove ------------------------------------------------------------------------------------------------------------------------------
def transcript_of(case_or_proto, th):
    from icicle_amd import FriTranscriptConfig

    _, labels, public, seed = case_or_proto[:4]
    return FriTranscriptConfig(th, *labels, public, list(seed))


def config_of(sd, pow_bits, nq, stream=None, is_async=False):
    from icicle_amd import FriConfig

    c = FriConfig.default()
    c.stopping_degree, c.pow_bits, c.nof_queries, c.stream, c.is_async = sd, pow_bits, nq, stream, is_async
    return c


def read_proof(proof):
    """the device's proof in the model's form"""
    F = fm.Field(proof.field, proof.extension)
    fp = proof.final_poly.reshape(-1, F.words)
    return {"final_poly": [tuple(int(v) for v in row) for row in fp], "nonce": proof.pow_nonce,
            "slots": [[(mp.leaf_idx, mp.leaf, mp.root, mp.path) for mp in row] for row in proof.slots()]}


def assert_same_proof(got, want, what):
    assert got["final_poly"] == want["final_poly"], what
    assert got["nonce"] == want["nonce"], what
    assert len(got["slots"]) == len(want["slots"]), what
    for q, (g, w) in enumerate(zip(got["slots"], want["slots"])):
        assert len(g) == len(w), (what, q)
        for r, (a, b) in enumerate(zip(g, w)):
            assert a == b, (what, "slot", q, "round", r)


def run_case(case, from_device, min_layer):
    import icicle_amd
    from icicle_amd.runtime import DeviceVec

    F = fm.Field(case["field"], case["extension"])
    proto = fm.case_protocol(case)
    x = np.array(case["input"], dtype=np.uint32).reshape((-1, 4) if F.ext else -1)
    th, lh, ch = hasher(case["transcript_hash"]), hasher(case["leaves_hash"], F.bytes), hasher(case["compress_hash"], 2 * fm.bm.OUT_SIZE[case["compress_hash"]])
    data = DeviceVec.from_host(x) if from_device else x
    proof = icicle_amd.fri_merkle_tree_prove(case["field"], config_of(case["stopping_degree"], case["pow_bits"], case["nof_queries"]), transcript_of(proto, th), data, lh, ch,
                                             min_layer, extension=F.ext)
    if from_device:
        assert np.array_equal(data.to_host(np.uint32), x.reshape(-1)), "prove changed its input"
    return proof, (th, lh, ch)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_prove_equals_the_reference(hip, case):
    import icicle_amd

    want = fm.case_proof(case)
    with domain(case["field"], case["log_domain"]):
        for from_device, min_layer in ((False, 0), (True, 0), (False, 3), (True, 3)):
            proof, hs = run_case(case, from_device, min_layer)
            assert proof.nof_queries == 2 * case["nof_queries"] and proof.nof_rounds == len(want["slots"][0]) and proof.final_poly_size == case["stopping_degree"] + 1
            assert_same_proof(read_proof(proof), want, (from_device, min_layer))
            cfg = config_of(case["stopping_degree"], case["pow_bits"], case["nof_queries"])
            assert icicle_amd.fri_merkle_tree_verify(case["field"], cfg, transcript_of(fm.case_protocol(case), hs[0]), proof, hs[1], hs[2], extension=case["extension"])


BIG = [  # field, extension, log n, tree hashers, transcript hasher, stopping degree; Blake3 only up to 2^8 (the model's speed)
    ("babybear", True, 12, ("keccak256", "keccak256"), "keccak256", 0),
    ("koalabear", False, 12, ("blake2s", "blake2s"), "sha3_512", 3),
    ("babybear", False, 10, ("sha3_256", "sha3_256"), "blake2s", 1),
    ("koalabear", True, 10, ("blake2s", "keccak256"), "blake3", 0),
    ("koalabear", True, 8, ("blake3", "blake3"), "keccak256", 0),
]


@pytest.mark.parametrize("field,ext,logn,trees,th_name,sd", BIG, ids=[f"{b[0]}{'_ext' if b[1] else ''}_2^{b[2]}_{b[3][1]}" for b in BIG])
def test_prove_equals_the_model_beyond_the_single_launch_top(hip, field, ext, logn, trees, th_name, sd):
    import icicle_amd

    F = fm.Field(field, ext)
    rng = random.Random(logn)
    elems = [tuple(rng.randrange(F.p) for _ in range(F.words)) for _ in range(1 << logn)]
    labels, public, seed = (b"ds", b"round", b"commit", b"nonce"), b"big", (3,) + (0,) * (F.words - 1)
    want = fm.prove(field, ext, elems, th_name, labels, public, seed, trees[0], trees[1], sd, 8, 20)
    th, lh, ch = hasher(th_name), hasher(trees[0], F.bytes), hasher(trees[1], 2 * fm.bm.OUT_SIZE[trees[1]])
    tc = icicle_amd.FriTranscriptConfig(th, *labels, public, list(seed))
    with domain(field, logn):
        proof = icicle_amd.fri_merkle_tree_prove(field, config_of(sd, 8, 20), tc, to_array(F, elems), lh, ch, 0, extension=ext)
        assert_same_proof(read_proof(proof), want, "model")
        assert icicle_amd.fri_merkle_tree_verify(field, config_of(sd, 8, 20), tc, proof, lh, ch, extension=ext)


# ---- verify -------------------------------------------------------------------------------------------------------------------------------
def rebuild(case, pr):
    """a device proof from the model's form, through create_with_arguments"""
    from icicle_amd import FriProof
    from icicle_amd.merkle import MerkleProof

    rows = [[MerkleProof.with_data(False, idx, leaf, root, path) for idx, leaf, root, path in row] for row in pr["slots"]]
    fp = np.array(pr["final_poly"], dtype=np.uint32)
    return FriProof.create_with_arguments(case["field"], rows, fp, pr["nonce"], extension=case["extension"])


def flip_first_bit(b: bytes) -> bytes:
    return bytes([b[0] ^ 1]) + b[1:]


def wrong_proofs(case):
    """(what, proof in the model's form, public state)"""
    public = bytes.fromhex(case["public_state"])
    base = lambda: fm.case_proof(case)
    pr = base()
    k = pr["slots"][0][-1][0] % len(pr["final_poly"])  # the coefficient the first query reads: q % final_size
    pr["final_poly"][k] = (pr["final_poly"][k][0] ^ 1,) + tuple(pr["final_poly"][k][1:])
    yield "final polynomial bit", pr, public
    for what, pos in (("leaf bit", 1), ("path byte bit", 3)):
        pr = base()
        row = list(pr["slots"][2][1])
        row[pos] = flip_first_bit(row[pos])
        pr["slots"][2][1] = tuple(row)
        yield what, pr, public
    pr = base()
    pr["nonce"] += 1
    yield "nonce off by one", pr, public
    pr = base()
    pr["final_poly"] = pr["final_poly"] + pr["final_poly"]
    yield "final polynomial too long", pr, public
    yield "changed public state", base(), public + b"\x01"
    # One slot opened against a tree of its own: the same leaf under the root of a layer that differs elsewhere. Its Merkle proof is
    # valid and collinearity holds, so only the comparison of the slots' roots finds it (the reference does not compare them).
    F = fm.Field(case["field"], case["extension"])
    pr = base()
    opened = {row[0][0] for row in pr["slots"]}
    other = next(i for i in range(1 << case["log_n"]) if i not in opened)
    raw = bytearray(b"".join(F.to_bytes(e) for e in fm.case_elements(case)))
    raw[other * F.bytes] ^= 1
    idx = pr["slots"][3][0][0]
    leaf, path, root = fm.bm.proof(fm.tree_shape(F, case["leaves_hash"], case["compress_hash"], 1 << case["log_n"]), bytes(raw), idx, False)
    assert leaf == pr["slots"][3][0][1] and root != pr["slots"][3][0][2]
    pr["slots"][3][0] = (idx, leaf, root, path)
    yield "a slot under another root", pr, public


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_verify_accepts_the_reference_and_rejects_wrong_proofs(hip, case):
    import icicle_amd

    F = fm.Field(case["field"], case["extension"])
    proto = fm.case_protocol(case)
    th, lh, ch = hasher(case["transcript_hash"]), hasher(case["leaves_hash"], F.bytes), hasher(case["compress_hash"], 2 * fm.bm.OUT_SIZE[case["compress_hash"]])
    cfg = lambda: config_of(case["stopping_degree"], case["pow_bits"], case["nof_queries"])

    def verify(pr, public):
        tc = icicle_amd.FriTranscriptConfig(th, *proto[1], public, list(proto[3]))
        return icicle_amd.fri_merkle_tree_verify(case["field"], cfg(), tc, rebuild(case, pr), lh, ch, extension=F.ext)  # raises unless SUCCESS

    # verification needs no NTT domain: w_n comes from the field's own root of unity
    assert verify(fm.case_proof(case), bytes.fromhex(case["public_state"])) is True
    for what, pr, public in wrong_proofs(case):
        if what == "nonce off by one" and case["pow_bits"] == 0:
            continue  # without a proof of work the nonce is not part of the transcript
        assert verify(pr, public) is False, what


# ---- the reference's Rust tests (fri/tests.rs: check_fri, check_fri_on_device) -----------------------------------------------------------
@pytest.mark.parametrize("field,ext", FIELD_KINDS, ids=KIND_IDS)
def test_rust_suite_replayed(hip, field, ext):
    """default config (pow_bits 16, 100 queries), default labels, seed one, on a stream of its own with is_async: 2^9 elements from the
    host, 2^10 from the device; Keccak-256 trees and transcript as in icicle-fields' instantiation of the tests"""
    import icicle_amd
    from icicle_amd.runtime import DeviceVec, Stream

    F = fm.Field(field, ext)
    rng = np.random.default_rng(9)
    th, lh, ch = hasher("keccak256"), hasher("keccak256", F.bytes), hasher("keccak256", 64)
    tc = icicle_amd.FriTranscriptConfig.new_default_labels(th, 1)
    stream = Stream()
    with domain(field, 10):
        for logn, on_device in ((9, False), (10, True)):
            x = rng.integers(0, F.p, size=(1 << logn, 4) if ext else 1 << logn, dtype=np.uint32)
            cfg = icicle_amd.FriConfig.default()
            assert (cfg.pow_bits, cfg.nof_queries, cfg.stopping_degree, cfg.folding_factor) == (16, 100, 0, 2)
            cfg.stream, cfg.is_async = stream.handle, True
            proof = icicle_amd.fri_merkle_tree_prove(field, cfg, tc, DeviceVec.from_host(x) if on_device else x, lh, ch, 0, extension=ext)
            stream.synchronize()
            assert (proof.nof_queries, proof.nof_rounds, proof.final_poly_size) == (200, logn, 1)
            vcfg = icicle_amd.FriConfig.default()
            vcfg.stream, vcfg.is_async = stream.handle, True
            assert icicle_amd.fri_merkle_tree_verify(field, vcfg, tc, proof, lh, ch, extension=ext)
            stream.synchronize()
    stream.destroy()
