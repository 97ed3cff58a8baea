"""GPU: sumcheck over babybear, koalabear, bn254 and bls12_381 -- the prover against every proof of the reference (tests/golden/
sumcheck_vectors.json) byte for byte with host and with device inputs, and against the model (tests/sumcheck_model.py) at every size
from L = 1 (no fold) over L = 2 (the first fold, from the caller's buffers) and L = 3 (the first fold of a folded table) to several
blocks, at L = 16 for every field and predefined program (more partial sums than the second launch has lanes), on all-zero and
all-(p - 1) inputs and for user programs; the verifier on the prover's proofs, on the model's, and on wrong ones."""
import functools
import random

import numpy as np
import pytest

from tests import sumcheck_model as sm

pytestmark = pytest.mark.gpu

CASES = sm.load_fixtures()
FIELDS = ["babybear", "koalabear", "bn254", "bls12_381"]
LABELS = (b"domain_separator_label", b"round_poly_label", b"round_challenge_label")


def hasher(name):
    from icicle_amd.hash import Hasher

    return getattr(Hasher, name)(0)


def to_array(field, values):
    w = sm.FIELDS[field][1]
    a = np.array([(int(v) >> (32 * i)) & 0xFFFFFFFF for v in values for i in range(w)], dtype=np.uint32)
    return a if w == 1 else a.reshape(-1, w)


def to_ints(field, arr):
    w = sm.FIELDS[field][1]
    a = np.asarray(arr, dtype=np.uint32).reshape(-1, w)
    return [sum(int(row[j]) << (32 * j) for j in range(w)) for row in a]


def device_program(field, program):
    from icicle_amd import ReturningValueProgram, Symbol

    if program.predefined is not None:
        return ReturningValueProgram.predefined(field, program.predefined)

    def fn(x):
        v = []
        for n in program.nodes:
            if n[0] == "in":
                v.append(x[n[1]])
            elif n[0] == "const":
                v.append(Symbol.constant(field, n[1]))
            else:
                a, b = v[n[1]], v[n[2]]
                v.append(a + b if n[0] == "add" else a - b if n[0] == "sub" else a * b)
        return v[-1]

    return ReturningValueProgram.from_function(field, fn, program.nof_inputs)


def transcript(field, hash_name, labels, seed):
    from icicle_amd import SumcheckTranscriptConfig

    return SumcheckTranscriptConfig(hasher(hash_name), *labels, seed)


def run_prover(field, polys, claimed, program, hash_name, labels, seed, on_device=False, cfg=None):
    """(round polynomials, challenge vector) as ints, and the objects"""
    from icicle_amd import Sumcheck
    from icicle_amd.runtime import DeviceVec

    arrays = [to_array(field, t) for t in polys]
    inputs = [DeviceVec.from_host(a) for a in arrays] if on_device else arrays
    sc = Sumcheck(field)
    tcfg = transcript(field, hash_name, labels, seed)
    proof = sc.prove(inputs, claimed, device_program(field, program), tcfg, cfg)
    rps = [to_ints(field, row) for row in proof.round_polys()]
    if on_device:  # the caller's polynomials are unchanged
        for v, a in zip(inputs, arrays):
            assert np.array_equal(v.to_host().reshape(a.shape), a)
    return rps, to_ints(field, sc.challenge_vector()), sc, proof, tcfg


def random_polys(field, m, n, seed):
    p = sm.FIELDS[field][0]
    rng = random.Random(seed)
    polys = [[rng.randrange(p) for _ in range(n)] for _ in range(m)]
    polys[0][0], polys[-1][-1] = 0, p - 1
    return polys


@functools.lru_cache(maxsize=None)
def model_case(field, program_id, L, fill=None):
    """inputs, claimed sum and the model's proof, computed once per (field, predefined program, size)"""
    program = sm.Program({0: 3, 1: 4}[program_id], predefined=program_id)
    p = sm.FIELDS[field][0]
    if fill is None:
        polys = random_polys(field, program.nof_inputs, 1 << L, 100 * L + program_id)
    else:
        polys = [[fill % p] * (1 << L) for _ in range(program.nof_inputs)]
    claimed = sm.claimed_sum(field, polys, program)
    return polys, claimed, program, sm.prove(field, polys, claimed, program, "keccak256", LABELS, 5)


# ---- the reference's proofs ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_prover_equals_the_reference(hip, case, on_device):
    field = case["field"]
    program = sm.Program.from_description(case["program"])
    claimed, seed = int(case["claimed_sum"], 16), int(case["seed"], 16)
    rps, challenges, sc, proof, tcfg = run_prover(field, sm.unhex(case["polys"]), claimed, program, case["transcript_hash"], sm.case_labels(case), seed, on_device)
    assert rps == sm.unhex(case["round_polys"])
    assert challenges == [int(v, 16) for v in case["challenges"]]
    assert proof.sizes() == (case["degree"] + 1, case["log_n"])
    assert sc.verify(proof, claimed, tcfg)


# ---- the model, every size -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", range(1, 15))
def test_every_size_babybear(hip, L):
    polys, claimed, program, want = model_case("babybear", 1, L)
    rps, challenges, sc, proof, tcfg = run_prover("babybear", polys, claimed, program, "keccak256", LABELS, 5, on_device=L % 2 == 0)
    assert rps == want["round_polys"] and challenges == want["challenges"]
    assert sc.verify(proof, claimed, tcfg)


@pytest.mark.parametrize("program_id", [0, 1], ids=["ab_minus_c", "eq_x_ab_minus_c"])
@pytest.mark.parametrize("field", FIELDS)
def test_two_to_the_sixteen(hip, field, program_id):
    polys, claimed, program, want = model_case(field, program_id, 16)
    rps, challenges, _, _, _ = run_prover(field, polys, claimed, program, "keccak256", LABELS, 5, on_device=True)
    assert rps == want["round_polys"] and challenges == want["challenges"]


@pytest.mark.parametrize("fill", [-1, 0], ids=["p_minus_1", "zero"])
@pytest.mark.parametrize("field", FIELDS)
def test_extreme_inputs(hip, field, fill):
    polys, claimed, program, want = model_case(field, 1, 12, fill)
    rps, challenges, sc, proof, tcfg = run_prover(field, polys, claimed, program, "keccak256", LABELS, 5)
    assert rps == want["round_polys"] and challenges == want["challenges"]
    assert sc.verify(proof, claimed, tcfg)


USER_PROGRAMS = {
    "degree6": sm.Program(6, [["in", i] for i in range(6)] + [["mul", 0, 1], ["mul", 6, 2], ["mul", 7, 3], ["mul", 8, 4], ["mul", 9, 5]]),
    # t = x0 + 5 used twice, and two more constants: (t t x1 - 7 t) + 0x77ffffff x2
    "constants": sm.Program(3, [["in", 0], ["in", 1], ["in", 2], ["const", 5], ["add", 0, 3], ["mul", 4, 4], ["mul", 5, 1], ["const", 7], ["mul", 7, 4], ["sub", 6, 8],
                                ["const", 0x77FFFFFF], ["mul", 10, 2], ["add", 9, 11]]),
    "eight_inputs": sm.Program(8, [["in", i] for i in range(8)] + [["mul", 0, 1], ["sub", 8, 2], ["mul", 9, 3], ["add", 10, 4], ["mul", 11, 5], ["sub", 12, 6],
                                                                    ["mul", 13, 7], ["mul", 14, 0]]),
}


@pytest.mark.parametrize("name", list(USER_PROGRAMS))
@pytest.mark.parametrize("field", FIELDS)
def test_user_programs(hip, field, name):
    program = USER_PROGRAMS[name]
    polys = random_polys(field, program.nof_inputs, 1 << 10, 77)
    claimed = sm.claimed_sum(field, polys, program)
    want = sm.prove(field, polys, claimed, program, "blake3", LABELS, 9)
    rps, challenges, sc, proof, tcfg = run_prover(field, polys, claimed, program, "blake3", LABELS, 9, on_device=name == "degree6")
    assert rps == want["round_polys"] and challenges == want["challenges"]
    assert sc.verify(proof, claimed, tcfg)


def test_unaligned_device_polynomials(hip):
    """device polynomials at addresses that are no multiple of 16 are copied, not read with 16-byte loads where they lie"""
    from icicle_amd import Sumcheck
    from icicle_amd.runtime import DeviceVec

    polys, claimed, program, want = model_case("babybear", 1, 6)
    block = DeviceVec.from_host(np.concatenate([np.concatenate([np.zeros(1, np.uint32), to_array("babybear", t)]) for t in polys]))
    views = [block.ptr + 4 * (65 * j + 1) for j in range(4)]
    sc = Sumcheck("babybear")
    # raw addresses: the size comes from a stand-in with the right nbytes
    class Raw(int):
        nbytes = 4 * 64
    proof = sc.prove([Raw(v) for v in views], claimed, device_program("babybear", program), transcript("babybear", "keccak256", LABELS, 5))
    assert [to_ints("babybear", r) for r in proof.round_polys()] == want["round_polys"]


def test_a_stream_of_its_own(hip):
    from icicle_amd import SumcheckConfig
    from icicle_amd.runtime import Stream

    polys, claimed, program, want = model_case("bn254", 1, 8)
    stream = Stream()
    cfg = SumcheckConfig.default()
    cfg.stream, cfg.is_async = stream.handle, True
    rps, challenges, _, _, _ = run_prover("bn254", polys, claimed, program, "keccak256", LABELS, 5, on_device=True, cfg=cfg)
    assert rps == want["round_polys"] and challenges == want["challenges"]  # the proof is host data: complete on return
    stream.synchronize()
    stream.destroy()


def test_round_times_of_the_timing_tool(hip):
    """icicle_hip_sumcheck_time_rounds: one positive time per round of the last proof, and the proof is the same"""
    import ctypes

    from icicle_amd._lib import lib

    polys, claimed, program, want = model_case("babybear", 1, 9)
    assert lib.icicle_hip_sumcheck_time_rounds(True) == 0
    try:
        rps, _, _, _, _ = run_prover("babybear", polys, claimed, program, "keccak256", LABELS, 5)
    finally:
        assert lib.icicle_hip_sumcheck_time_rounds(False) == 0
    ms, count = (ctypes.c_double * 16)(), ctypes.c_int()
    assert lib.icicle_hip_sumcheck_round_times(ms, 16, ctypes.byref(count)) == 0
    assert rps == want["round_polys"] and count.value == 9 and all(0 < ms[r] < 1000 for r in range(9))
    assert lib.icicle_hip_sumcheck_round_times(None, 16, ctypes.byref(count)) == 3


# ---- the verifier ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", FIELDS)
def test_verifier(hip, field):
    import ctypes

    from icicle_amd import Sumcheck, SumcheckProof
    from icicle_amd._lib import lib

    p, w = sm.FIELDS[field]
    polys, claimed, program, want = model_case(field, 1, 8)
    rps, _, sc, proof, tcfg = run_prover(field, polys, claimed, program, "keccak256", LABELS, 5)
    assert sc.verify(proof, claimed, tcfg)
    assert sm.verify(field, rps, claimed, "keccak256", LABELS, 5)  # the device's proof in the model
    rebuild = lambda rows: SumcheckProof.create(field, [to_array(field, r).reshape(-1) for r in rows])
    fresh = Sumcheck(field)
    assert fresh.verify(rebuild(want["round_polys"]), claimed, tcfg)  # the model's proof on the device, rebuilt with sumcheck_proof_create
    verify = getattr(lib, field + "_sumcheck_verify")
    ffi, keep = tcfg._ffi(field)
    for r in (0, 4, 6):  # round 0, a middle round, the last round that is checked
        for k in (0, 3):
            bad = [list(row) for row in rps]
            bad[r][k] = (bad[r][k] + 1) % p
            ok = ctypes.c_bool(True)
            wrong = rebuild(bad)
            c = (ctypes.c_uint32 * w)(*[(claimed >> (32 * i)) & 0xFFFFFFFF for i in range(w)])
            assert verify(fresh.handle, wrong.handle, c, ctypes.byref(ffi), ctypes.byref(ok)) == 0 and ok.value is False, (r, k)
            assert not sm.verify(field, bad, claimed, "keccak256", LABELS, 5)
    assert not fresh.verify(proof, (claimed + 1) % p, tcfg)
    assert not fresh.verify(proof, claimed, transcript(field, "keccak256", (LABELS[0] + b"!", LABELS[1], LABELS[2]), 5))
    assert not fresh.verify(proof, claimed, transcript(field, "sha3_256", LABELS, 5))
    not_canonical = [list(row) for row in rps]
    not_canonical[7][2] += p  # the last round polynomial is not checked against anything, but a word at or above p is no element
    if not_canonical[7][2] < 1 << (32 * w):
        assert not fresh.verify(rebuild(not_canonical), claimed, tcfg)
    last = [list(row) for row in rps]
    last[7][2] = (last[7][2] + 1) % p
    assert fresh.verify(rebuild(last), claimed, tcfg)  # as in the reference
    del keep
