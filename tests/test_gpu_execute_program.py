"""GPU: execute_program over babybear, koalabear, bn254 and bls12_381 -- every result of the reference (tests/golden/
execute_program_vectors.json) byte for byte with host and with device data, and the model (tests/execute_program_model.py) for the
predefined programs and two user programs at one element, around a wave (63, 64, 65) and over several blocks (257), at sizes that send
the grid-stride loops of the interpreter (4096 blocks of 64 lanes, four elements per lane for the one-word fields) and of the predefined kernels (2048 blocks of 256 lanes, four
elements per lane with 16-byte loads) through a second pass, on device views that are only element-aligned, in place, in batches, at
the cap on live values and over it, and against the three vector operations the fused call replaces."""
import numpy as np
import pytest

from tests import execute_program_model as em

pytestmark = pytest.mark.gpu

CASES = em.load_fixtures()
FIELDS = ["babybear", "koalabear", "bn254", "bls12_381"]
INVALID_ARGUMENT = 11
SIZES = (1, 63, 64, 65, 257)

V = em.VecProgram
IN = lambda n: [["in", i] for i in range(n)]
# x3 = (x0 + 5) x1 - 7 x2 and x4 = (x0 + 5) (x0 + 5): two outputs over a shared node, two constants
TWO_OUT = V(5, IN(5) + [["const", 5], ["add", 0, 5], ["mul", 6, 1], ["const", 7], ["mul", 8, 2], ["sub", 7, 9], ["mul", 6, 6]], [0, 1, 2, 10, 11])
# x0 = x1 / x0 + x0 (in and out), x2 = x0: the copy reads the new x0
INV_IN_OUT = V(3, IN(3) + [["inv", 0], ["mul", 3, 1], ["add", 4, 0]], [5, 1, 0])
USER_EQ = V(5, IN(5) + [["mul", 0, 1], ["sub", 5, 2], ["mul", 3, 6]], [0, 1, 2, 3, 7])  # E (A B - C) through the interpreter
PROGRAMS = {"ab": V(4, predefined=em.AB_MINUS_C), "eq": V(5, predefined=em.EQ_X_AB_MINUS_C), "two_out": TWO_OUT, "inv_in_out": INV_IN_OUT}


def to_array(field, values):
    w = em.FIELDS[field][1]
    return np.array([(int(v) >> (32 * i)) & 0xFFFFFFFF for v in values for i in range(w)], dtype=np.uint32)


def to_ints(field, arr):
    w = em.FIELDS[field][1]
    a = np.asarray(arr, dtype=np.uint32).reshape(-1, w)
    if w == 1:
        return [int(v) for v in a[:, 0]]
    return [int.from_bytes(row.tobytes(), "little") for row in a]


def random_words(field, n, seed):
    """n canonical elements as uint32 words, 0, 1 and p - 1 among them; the top word is kept below the modulus' top word"""
    p, w = em.FIELDS[field]
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 1 << 32, size=(n, w), dtype=np.uint64).astype(np.uint32)
    a[:, w - 1] %= np.uint32(p >> (32 * (w - 1)))
    for k, v in enumerate((0, 1, p - 1)):
        if n > 3 * k + seed % 3:
            a[3 * k + seed % 3] = to_array(field, [v])
    return a.reshape(-1)


def device_program(field, program):
    from icicle_amd import Program, Symbol

    if program.predefined is not None:
        return Program.predefined(field, program.predefined)

    def fn(x):
        v = []
        for n in program.nodes:
            if n[0] == "in":
                v.append(x[n[1]])
            elif n[0] == "const":
                v.append(Symbol.constant(field, n[1]))
            elif n[0] == "inv":
                v.append(v[n[1]].inverse())
            else:
                a, b = v[n[1]], v[n[2]]
                v.append(a + b if n[0] == "add" else a - b if n[0] == "sub" else a * b)
        x[:] = [v[j] for j in program.params]

    return Program.from_function(field, fn, program.nof_parameters)


def run(field, program, arrays, on_device, batch=1, handle=None):
    """the vectors after the call, as arrays; `arrays` are not changed"""
    from icicle_amd import VecOpsConfig, execute_program
    from icicle_amd.runtime import DeviceVec

    handle = handle or device_program(field, program)
    cfg = VecOpsConfig.default()
    cfg.batch_size = batch
    size = arrays[0].size // em.FIELDS[field][1] // batch
    if on_device:
        vecs = [DeviceVec.from_host(a) for a in arrays]
        execute_program(field, vecs, handle, cfg, size=size)
        return [v.to_host() for v in vecs]
    copies = [a.copy() for a in arrays]
    execute_program(field, copies, handle, cfg, size=size)
    return copies


def check_against_model(field, program, arrays, got):
    want = em.execute(field, program, [to_ints(field, a) for a in arrays])
    written = program.written()
    for j, (a, g) in enumerate(zip(arrays, got)):
        if j in written:
            assert to_ints(field, g) == want[j], j
        else:
            assert np.array_equal(g, a), f"parameter {j} is not written by the program"


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_equals_the_reference(hip, case):
    field, program = case["field"], em.VecProgram.from_description(case["program"])
    arrays = [to_array(field, row) for row in em.unhex(case["data"])]
    handle = device_program(field, program)
    for on_device in (False, True):
        got = run(field, program, arrays, on_device, batch=case["batch_size"], handle=handle)
        for j, (a, g) in enumerate(zip(arrays, got)):
            want = to_array(field, [int(v, 16) for v in case["written"][str(j)]]) if str(j) in case["written"] else a
            assert np.array_equal(g, want), (j, on_device)


@pytest.mark.parametrize("name", list(PROGRAMS))
@pytest.mark.parametrize("field", FIELDS)
def test_sizes_around_a_wave_and_a_block(hip, field, name):
    program = PROGRAMS[name]
    handle = device_program(field, program)
    for n in SIZES:
        arrays = [random_words(field, n, 10 * n + j) for j in range(program.nof_parameters)]
        if name == "inv_in_out":
            arrays[0][:em.FIELDS[field][1]] = 0  # 1 / 0
        check_against_model(field, program, arrays, run(field, program, arrays, on_device=n != 64, handle=handle))
        if n == 257:  # and from the host
            check_against_model(field, program, arrays, run(field, program, arrays, on_device=False, handle=handle))


@pytest.mark.parametrize("field", ["babybear", "bn254"])
def test_interpreter_past_a_full_grid(hip, field):
    """the 4096 blocks of 64 lanes take a second pass, three lanes a last element: 2^18 + 3 elements at one element per lane (eight
    words), 2^20 + 3 at four (one word)"""
    n = (1 << (20 if em.FIELDS[field][1] == 1 else 18)) + 3
    arrays = [random_words(field, n, 40 + j) for j in range(5)]
    check_against_model(field, TWO_OUT, arrays, run(field, TWO_OUT, arrays, on_device=True))


def numpy_eq(p, a, b, c, e):
    a, b, c, e = (v.astype(np.uint64) for v in (a, b, c, e))
    return (e * ((a * b % p + p - c) % p) % p).astype(np.uint32)  # every product is below 2^62


def test_predefined_past_a_full_grid_babybear(hip):
    """E (A B - C) at 2^21 + 7 elements, once at 16-byte aligned addresses (four elements per lane: 2^19 lanes take a second pass, the
    last three elements go to the first lanes) and once on views one element into their allocations (one element per lane)"""
    from icicle_amd import Program, VecOpsConfig, execute_program
    from icicle_amd.runtime import DeviceVec

    field, n = "babybear", (1 << 21) + 7
    p = em.FIELDS[field][0]
    arrays = [random_words(field, n, 50 + j) for j in range(4)]
    want = numpy_eq(p, *arrays)
    sample = list(range(70)) + list(range(n - 70, n)) + [int(i) for i in np.random.default_rng(1).integers(0, n, 200)]
    model = em.execute(field, PROGRAMS["eq"], [[int(a[i]) for i in sample] for a in arrays] + [[0] * len(sample)])[4]
    assert [int(want[i]) for i in sample] == model  # the vectorised reference is the model
    handle = Program.predefined(field, 1)
    vecs = [DeviceVec.from_host(np.concatenate([np.zeros(1, np.uint32), a])) for a in arrays] + [DeviceVec(4 * (n + 1))]
    execute_program(field, [v.ptr + 4 for v in vecs], handle, VecOpsConfig.default(), size=n)
    assert np.array_equal(vecs[4].to_host()[1:], want)
    for v, a in zip(vecs, arrays):
        assert np.array_equal(v.to_host()[1:], a)
    aligned = [DeviceVec.from_host(a) for a in arrays] + [DeviceVec(4 * n)]
    execute_program(field, aligned, handle, VecOpsConfig.default(), size=n)
    assert np.array_equal(aligned[4].to_host(), want)


@pytest.mark.parametrize("field", FIELDS)
def test_user_program_equals_predefined_and_the_vector_operations(hip, field):
    """E (A B - C) three ways, byte for byte; for the eight-word fields at 2^19 + 3 elements, one pass of the predefined kernel's grid
    and three elements more, with the model on a sample"""
    from icicle_amd import Program, VecOpsConfig, execute_program, vecops
    from icicle_amd.runtime import DeviceVec

    p, w = em.FIELDS[field]
    n = (1 << 19) + 3 if w == 8 else 1000
    arrays = [random_words(field, n, 60 + j) for j in range(4)]
    vecs = [DeviceVec.from_host(a) for a in arrays]
    outs = [DeviceVec(4 * w * n) for _ in range(3)]
    execute_program(field, vecs + [outs[0]], Program.predefined(field, 1), VecOpsConfig.default(), size=n)
    execute_program(field, vecs + [outs[1]], device_program(field, USER_EQ), VecOpsConfig.default(), size=n)
    vecops.vector_mul(field, vecs[0], vecs[1], VecOpsConfig.default(), out=outs[2], size=n)
    vecops.vector_sub(field, outs[2], vecs[2], VecOpsConfig.default(), out=outs[2], size=n)
    vecops.vector_mul(field, vecs[3], outs[2], VecOpsConfig.default(), out=outs[2], size=n)
    got = [o.to_host() for o in outs]
    assert np.array_equal(got[0], got[2]) and np.array_equal(got[1], got[2])
    sample = list(range(64)) + list(range(n - 64, n)) + [int(i) for i in np.random.default_rng(2).integers(0, n, 128)]
    rows = [[to_ints(field, a.reshape(-1, w)[i])[0] for i in sample] for a in arrays]
    model = em.execute(field, PROGRAMS["eq"], rows + [[0] * len(sample)])[4]
    assert [to_ints(field, got[0].reshape(-1, w)[i])[0] for i in sample] == model
    for v, a in zip(vecs, arrays):
        assert np.array_equal(v.to_host(), a)  # the inputs are as they were


@pytest.mark.parametrize("field", ["koalabear", "bls12_381"])
def test_device_views_one_element_into_an_allocation(hip, field):
    """every pointer one element past an allocation's start: 4-byte aligned for the one-word field. Both kinds of program."""
    from icicle_amd import VecOpsConfig, execute_program
    from icicle_amd.runtime import DeviceVec

    w, n = em.FIELDS[field][1], 133
    for program in (PROGRAMS["eq"], TWO_OUT):
        arrays = [random_words(field, n, 70 + j) for j in range(5)]
        guard = np.full(w, 0xDEADBEEF, dtype=np.uint32)
        vecs = [DeviceVec.from_host(np.concatenate([guard, a, guard])) for a in arrays]
        execute_program(field, [v.ptr + 4 * w for v in vecs], device_program(field, program), VecOpsConfig.default(), size=n)
        back = [v.to_host() for v in vecs]
        for b in back:
            assert np.array_equal(b[:w], guard) and np.array_equal(b[-w:], guard)  # nothing before or after the view is written
        check_against_model(field, program, arrays, [b[w:-w] for b in back])


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("field", FIELDS)
def test_in_place(hip, field, on_device):
    """the output's pointer is an input's: E (A B - C) into A (predefined, at a size with 16-byte loads and a tail), and a user program
    whose output parameter shares its vector with an input parameter"""
    from icicle_amd import VecOpsConfig, execute_program
    from icicle_amd.runtime import DeviceVec

    p, n = em.FIELDS[field][0], 71
    arrays = [random_words(field, n, 80 + j) for j in range(4)]
    ints = [to_ints(field, a) for a in arrays]
    want_eq = [e * (a * b - c) % p for a, b, c, e in zip(*ints)]
    sum_prod = V(3, IN(3) + [["mul", 0, 1], ["add", 3, 0]], [0, 1, 4])  # x2 = x0 x1 + x0, with x2's vector = x1's
    want_user = [(a * b + a) % p for a, b in zip(ints[0], ints[1])]
    if on_device:
        vecs = [DeviceVec.from_host(a) for a in arrays]
        execute_program(field, vecs + [vecs[0]], device_program(field, PROGRAMS["eq"]), VecOpsConfig.default(), size=n)
        assert to_ints(field, vecs[0].to_host()) == want_eq
        assert all(np.array_equal(vecs[j].to_host(), arrays[j]) for j in (1, 2, 3))
        vecs = [DeviceVec.from_host(a) for a in arrays[:2]]
        execute_program(field, vecs + [vecs[1]], device_program(field, sum_prod), VecOpsConfig.default(), size=n)
        assert to_ints(field, vecs[1].to_host()) == want_user and np.array_equal(vecs[0].to_host(), arrays[0])
    else:
        host = [a.copy() for a in arrays]
        execute_program(field, host + [host[0]], device_program(field, PROGRAMS["eq"]), VecOpsConfig.default(), size=n)
        assert to_ints(field, host[0]) == want_eq
        assert all(np.array_equal(host[j], arrays[j]) for j in (1, 2, 3))
        host = [a.copy() for a in arrays[:2]]
        execute_program(field, host + [host[1]], device_program(field, sum_prod), VecOpsConfig.default(), size=n)
        assert to_ints(field, host[1]) == want_user and np.array_equal(host[0], arrays[0])


@pytest.mark.parametrize("field", FIELDS)
def test_untouched_and_unwritten_parameters(hip, field):
    """a parameter the program never names is left alone, also where its words are no element of the field; one it only reads is
    bit-identical afterwards"""
    w, n = em.FIELDS[field][1], 70
    only = V(4, IN(4) + [["add", 0, 0]], [0, 1, 2, 4])  # x3 = x0 + x0: x1 and x2 are never touched
    arrays = [random_words(field, n, 90 + j) for j in range(4)]
    arrays[1][:] = 0xFFFFFFFF  # no element of the field: it must come back as it is
    for on_device in (False, True):
        check_against_model(field, only, arrays, run(field, only, arrays, on_device))


@pytest.mark.parametrize("field", FIELDS)
def test_batches(hip, field):
    """batch_size entries of `size` elements are size * batch_size elements, with and without columns_batch"""
    from icicle_amd import VecOpsConfig, execute_program

    for program in (PROGRAMS["ab"], TWO_OUT):
        arrays = [random_words(field, 3 * 23, 100 + j) for j in range(program.nof_parameters)]
        for on_device in (False, True):
            check_against_model(field, program, arrays, run(field, program, arrays, on_device, batch=3))
        cfg = VecOpsConfig.default()
        cfg.batch_size, cfg.columns_batch = 3, True
        copies = [a.copy() for a in arrays]
        execute_program(field, copies, device_program(field, program), cfg, size=23)
        check_against_model(field, program, arrays, copies)


def wide_program(k):
    """tests/test_execute_program_cpu.py wide_program: k products alive at once"""
    nodes = IN(3) + [["mul", 0 if j == 0 else 2 + j, 1] for j in range(k)]
    acc = 2 + k
    for j in range(k - 1, 0, -1):
        nodes.append(["add", acc, 2 + j])
        acc = len(nodes) - 1
    return V(3, nodes, [0, 1, acc])


@pytest.mark.parametrize("field", FIELDS)
def test_at_the_cap_and_over_it(hip, field):
    from icicle_amd import IcicleError

    cap = em.CAPS[em.FIELDS[field][1]]
    k = next(k for k in range(2, 80) if em.lower(wide_program(k), cap)[1] == cap)
    arrays = [random_words(field, 130, 110 + j) for j in range(3)]
    check_against_model(field, wide_program(k), arrays, run(field, wide_program(k), arrays, on_device=True))
    assert em.lower(wide_program(k + 1), cap) is None
    with pytest.raises(IcicleError) as err:
        run(field, wide_program(k + 1), arrays, on_device=True)
    assert err.value.code == INVALID_ARGUMENT


def test_a_stream_of_its_own_and_a_program_used_twice(hip):
    """is_async on a stream of the caller's: the result is there once the stream is drained; the second call reuses the program's
    device copy"""
    from icicle_amd import VecOpsConfig, execute_program
    from icicle_amd.runtime import DeviceVec, Stream

    field, n = "bn254", 300
    handle = device_program(field, TWO_OUT)
    stream = Stream()
    cfg = VecOpsConfig.default()
    cfg.stream, cfg.is_async = stream.handle, True
    for seed in (120, 130):
        arrays = [random_words(field, n, seed + j) for j in range(5)]
        vecs = [DeviceVec.from_host(a) for a in arrays]
        execute_program(field, vecs, handle, cfg, size=n)
        stream.synchronize()
        check_against_model(field, TWO_OUT, arrays, [v.to_host() for v in vecs])
    stream.destroy()
