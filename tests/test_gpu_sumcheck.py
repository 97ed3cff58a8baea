"""GPU: sumcheck over babybear, koalabear, bn254 and bls12_381 -- the prover against every proof of the reference (tests/golden/
sumcheck_vectors.json) byte for byte with host and with device inputs, and against the model (tests/sumcheck_model.py) at every size
from L = 1 (no fold) over L = 2 (the first fold, from the caller's buffers) and L = 3 (the first fold of a folded table) to several
blocks, at L = 16 for every field and predefined program (more partial sums than the second launch has lanes), on all-zero and
all-(p - 1) inputs and for user programs; the verifier on the prover's proofs, on the model's, and on wrong ones. The round launches
have a capped grid whose lanes walk on over the remaining items: that loop runs at small sizes with the cap forced down
(SumcheckConfig.ext "hip_sumcheck_max_grid") against the model, and at the library's own cap at the smallest sizes that exceed it
against the reference's proofs of tests/golden/sumcheck_vectors_large.json."""
import contextlib
import ctypes
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
    "constants": sm.CONSTANTS,  # t = x0 + 5 used twice, and two more constants: (t t x1 - 7 t) + 0x77ffffff x2
    "eight_inputs": sm.Program(8, [["in", i] for i in range(8)] + [["mul", 0, 1], ["sub", 8, 2], ["mul", 9, 3], ["add", 10, 4], ["mul", 11, 5], ["sub", 12, 6],
                                                                    ["mul", 13, 7], ["mul", 14, 0]]),
}


@functools.lru_cache(maxsize=None)
def user_case(field, name):
    """inputs, claimed sum and the model's proof of a user program at L = 10, computed once"""
    program = USER_PROGRAMS[name]
    polys = random_polys(field, program.nof_inputs, 1 << 10, 77)
    claimed = sm.claimed_sum(field, polys, program)
    return polys, claimed, program, sm.prove(field, polys, claimed, program, "blake3", LABELS, 9)


@pytest.mark.parametrize("name", list(USER_PROGRAMS))
@pytest.mark.parametrize("field", FIELDS)
def test_user_programs(hip, field, name):
    polys, claimed, program, want = user_case(field, name)
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


# ---- lanes that walk on past a capped grid -------------------------------------------------------------------------------------------------
def launch_info(predefined):
    """(lanes of a round block, most blocks of a round launch) as the library has them"""
    from icicle_amd._lib import lib

    block, grid = ctypes.c_int(), ctypes.c_int()
    assert lib.icicle_hip_sumcheck_launch_info(int(predefined), ctypes.byref(block), ctypes.byref(grid)) == 0
    return block.value, grid.value


@contextlib.contextmanager
def capped(cap, foreign_key=None):
    """a SumcheckConfig whose ext holds hip_sumcheck_max_grid = cap"""
    from icicle_amd import SumcheckConfig
    from icicle_amd._lib import lib

    cfg = SumcheckConfig.default()
    ext = lib.create_config_extension()
    lib.config_extension_set_int(ext, b"hip_sumcheck_max_grid", cap)
    if foreign_key:
        lib.config_extension_set_int(ext, foreign_key, 3)
    cfg.ext = ext
    try:
        yield cfg
    finally:
        lib.destroy_config_extension(ext)


def assert_walks(field, program, L, cap):
    """rounds 0 and 1 hand a grid of `cap` blocks more items than it has lanes (sm.round_items: the pairs, or half of them where a lane
    takes two): with the library's own block size, so that a change of it cannot turn the case into a one-trip test"""
    block, max_grid = launch_info(program.predefined is not None)
    assert 1 <= cap <= max_grid
    for r in (0, 1):
        assert sm.round_items(field, program.predefined is not None, L, r) > cap * block, (field, L, cap, r, block)


def check_capped(field, polys, claimed, program, want, hash_name, seed, cap, on_device):
    """the proof under a forced cap: the model's, the device verifier's, and byte for byte that of the same call without the key"""
    with capped(cap) as cfg:
        rps, challenges, sc, proof, tcfg = run_prover(field, polys, claimed, program, hash_name, LABELS, seed, on_device=on_device, cfg=cfg)
    assert rps == want["round_polys"] and challenges == want["challenges"]
    assert sc.verify(proof, claimed, tcfg)
    _, _, _, plain, _ = run_prover(field, polys, claimed, program, hash_name, LABELS, seed, on_device=on_device)
    assert proof.round_polys().tobytes() == plain.round_polys().tobytes()


# Predefined programs have 128 lanes per block (launch_info), so with at most 3 blocks rounds 0 and 1 both walk from L = 11 on: L = 11
# (host inputs) and L = 12 (device inputs) assert it. L = 9 and 10 keep odd grids of one to three blocks over the last full and the
# first partial trips (L = 10 walks in both rounds at cap 1, L = 9 in round 0 of the eight-word fields only).
WALKING_L = (11, 12)


@pytest.mark.parametrize("L", [9, 10, 11, 12])
@pytest.mark.parametrize("program_id", [0, 1], ids=["ab_minus_c", "eq_x_ab_minus_c"])
@pytest.mark.parametrize("cap", [1, 2, 3])
@pytest.mark.parametrize("field", FIELDS)
def test_forced_cap_predefined(hip, field, cap, program_id, L):
    """SHAPE 0 (one-word form: two pairs per load; eight-word form), SHAPE 1 with its stores in rounds 1 .. L-2 and SHAPE 2 in the last
    round, each lane taking up to 8 (one word) or 16 (eight words) trips at cap 1 and L = 12"""
    polys, claimed, program, want = model_case(field, program_id, L)
    if L in WALKING_L:
        assert_walks(field, program, L, cap)
    check_capped(field, polys, claimed, program, want, "keccak256", 5, cap, on_device=L % 2 == 0)


@pytest.mark.parametrize("name", list(USER_PROGRAMS))
@pytest.mark.parametrize("cap", [1, 2, 3])
@pytest.mark.parametrize("field", FIELDS)
def test_forced_cap_user_programs(hip, field, cap, name):
    """the interpreter (64 lanes per block) uses its LDS variable file for up to 8 pairs in round 0 at cap 1, with the constants written once"""
    polys, claimed, program, want = user_case(field, name)
    assert_walks(field, program, 10, cap)
    check_capped(field, polys, claimed, program, want, "blake3", 9, cap, on_device=True)


@pytest.mark.parametrize("fill", [-1, 0], ids=["p_minus_1", "zero"])
@pytest.mark.parametrize("field", ["babybear", "bn254"])
def test_forced_cap_extreme_inputs(hip, field, fill):
    polys, claimed, program, want = model_case(field, 1, 10, fill)
    assert_walks(field, program, 10, 1)
    check_capped(field, polys, claimed, program, want, "keccak256", 5, 1, on_device=True)


def test_max_grid_key_values(hip):
    """absent, 0 and negative: the library's cap; values above it are clamped to it; a foreign key beside it is tolerated"""
    polys, claimed, program, want = model_case("babybear", 1, 10)
    _, max_grid = launch_info(True)
    for cap, foreign in ((0, None), (-1, None), (max_grid, None), (max_grid + 1, None), (2**30, None), (2, b"hip_num_devices"), (1, b"no_such_key")):
        with capped(cap, foreign) as cfg:
            rps, challenges, _, _, _ = run_prover("babybear", polys, claimed, program, "keccak256", LABELS, 5, cfg=cfg)
        assert rps == want["round_polys"] and challenges == want["challenges"], (cap, foreign)


# ---- the library's own cap: the smallest sizes at which an unforced launch walks ----------------------------------------------------------
LARGE = sm.load_large_fixtures()


@pytest.mark.parametrize("case, walking", [(c, t[5]) for c, t in zip(LARGE, sm.LARGE_CASES)], ids=[c["name"] for c in LARGE])
def test_the_real_cap(hip, case, walking):
    """bb_eq_l21: round 0 with 2^19 items (two pairs each), round 1 with 2^19 pairs and SHAPE 1's stores; bn254_eq_l20: 2^19 pairs in
    round 0 (round 1 is exactly one full grid, and the second launch adds all of its rows of partials); bb_constants_l20: the interpreter over 2^19 pairs with 131072 lanes, and 2^18 pairs with stores. Expected values: the
    reference's (tests/golden/mint_sumcheck_vectors.py --large); the inputs come from the seed and are checked by their sha256 first."""
    from icicle_amd import Sumcheck
    from icicle_amd.runtime import DeviceVec

    field, L = case["field"], case["log_n"]
    program = sm.Program.from_description(case["program"])
    claimed, seed = int(case["claimed_sum"], 16), int(case["seed"], 16)
    block, max_grid = launch_info(program.predefined is not None)
    assert case["name"] == sm.LARGE_CASES[LARGE.index(case)][0] and 0 in walking
    for r in walking:
        assert sm.round_items(field, program.predefined is not None, L, r) > max_grid * block, r
    arrays = sm.large_inputs(field, program.nof_inputs, 1 << L, case["input_seed"])
    assert sm.sha256_of(arrays) == case["input_sha256"], "the input generator drifted: not a kernel failure"
    inputs = [DeviceVec.from_host(a) for a in arrays]
    sc = Sumcheck(field)
    tcfg = transcript(field, case["transcript_hash"], sm.case_labels(case), seed)
    proof = sc.prove(inputs, claimed, device_program(field, program), tcfg)
    assert [to_ints(field, row) for row in proof.round_polys()] == sm.unhex(case["round_polys"])
    assert to_ints(field, sc.challenge_vector()) == [int(v, 16) for v in case["challenges"]]
    assert proof.sizes() == (case["degree"] + 1, L)
    assert sc.verify(proof, claimed, tcfg)
    for v, a in zip(inputs, arrays):  # the caller's polynomials are unchanged
        assert np.array_equal(v.to_host().reshape(a.shape), a)
