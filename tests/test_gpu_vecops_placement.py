"""GPU: where the operands and the result of a vector operation live does not change its bytes. Every entry-point family -- the seven
two-operand ops, mixed_mul, div, inv, sum, product, bit_reverse, matrix_transpose, scalar_convert_montgomery, slice,
highest_non_zero_idx, poly_eval -- over one field per element kind (babybear, goldilocks, bn254, the babybear and goldilocks extensions)
is called with each operand on the host or on the device, the result on the host, on the device, and on the device in place of operand a
or b where the function allows that, synchronously and with is_async on a stream of the test's that is synchronised after the call. The
expected bytes are those of the same call with everything on the host, which the other GPU tests of these functions hold against the
reference.

Shapes: 67 elements x batch 3 in both batch layouts (more than one wave, a ragged last wave, a length that is no multiple of four,
several batch entries, one partial inversion tile); bit_reverse 64 x 3; matrix_transpose 37 x 5 x 3."""
import itertools

import numpy as np
import pytest

from oracle import pyref
from tests.util import rand_scalars, to_words

pytestmark = pytest.mark.gpu

# (field, extension, u32 words per element, u32 words per base-field element)
KINDS = [("babybear", False, 1, 1), ("goldilocks", False, 2, 2), ("bn254", False, 8, 8), ("babybear", True, 4, 1), ("goldilocks", True, 4, 2)]
KIND_IDS = [f"{f}{'_extension' if e else ''}" for f, e, _, _ in KINDS]
BASE_KINDS = [k for k in KINDS if not k[1]]
BASE_IDS = [k[0] for k in BASE_KINDS]
SIZE, BATCH = 67, 3
FILL = 0xA5A5A5A5


def elements(field, words, n, rng, zeros=()):
    """n canonical elements of `words` words ([n, words] uint32): components below the modulus, the elements at `zeros` zero"""
    if field == "babybear":
        x = rng.integers(0, pyref.NTT_FIELDS["babybear"].p, size=(n, words), dtype=np.uint32)
    elif field == "goldilocks":
        x = rng.integers(0, (1 << 64) - (1 << 32) + 1, size=(n, words // 2), dtype=np.uint64).view(np.uint32).reshape(n, words)
    else:
        x = to_words(rand_scalars(rng, n, pyref.CURVES[field].r), words)
    x = np.ascontiguousarray(x)
    x[list(zeros)] = 0
    return x


@pytest.fixture(scope="module")
def stream(hip):
    from icicle_amd.runtime import Stream

    s = Stream()
    yield s
    s.destroy()


def run_placements(call, operands, out_shape, stream, aliasable=(), out_dtype=np.uint32, layouts=(False, True), what=""):
    """call(cfg, ops, out) issues one library call. `operands`: host arrays; `aliasable`: the operands the result may replace."""
    from icicle_amd._lib import VecOpsConfig
    from icicle_amd.runtime import DeviceVec

    def config(columns, is_async):
        cfg = VecOpsConfig.default()
        cfg.batch_size, cfg.columns_batch = BATCH, columns
        if is_async:
            cfg.is_async, cfg.stream = True, stream.handle
        return cfg

    def blank():
        return np.full(out_shape, FILL, out_dtype)

    ran = 0
    for columns in layouts:
        want = blank()
        call(config(columns, False), [x.copy() for x in operands], want)
        assert not (want == FILL).all(), what
        for devs in itertools.product((False, True), repeat=len(operands)):
            for result in ["host", "device"] + [i for i in aliasable if devs[i]]:
                for is_async in (False, True):
                    ops = [DeviceVec.from_host(x) if d else x.copy() for x, d in zip(operands, devs)]
                    out = blank() if result == "host" else DeviceVec.from_host(blank()) if result == "device" else ops[result]
                    call(config(columns, is_async), ops, out)
                    if is_async:
                        stream.synchronize()
                    where = (what, "columns" if columns else "rows", devs, result, "async" if is_async else "sync")
                    got = out if result == "host" else out.to_host(out_dtype, out_shape)
                    assert np.array_equal(got, want), where
                    for x, o in zip(operands, ops):  # an operand that is not the result is left alone
                        if o is not out:
                            assert np.array_equal(o if isinstance(o, np.ndarray) else o.to_host(x.dtype, x.shape), x), where
                    ran += 1
    return ran


@pytest.mark.parametrize("field,extension,words,base_words", KINDS, ids=KIND_IDS)
def test_two_operand_ops(hip, stream, field, extension, words, base_words):
    from icicle_amd import vecops as V

    rng = np.random.default_rng(11)
    a, b, s = (elements(field, words, n, rng) for n in (SIZE * BATCH, SIZE * BATCH, BATCH))
    for op in (V.vector_add, V.vector_sub, V.vector_mul):
        ran = run_placements(lambda cfg, ops, out, op=op: op(field, ops[0], ops[1], cfg, out, SIZE, extension), [a, b], a.shape, stream, (0, 1), what=op.__name__)
        assert ran == 2 * 12 * 2
    for op in (V.scalar_add_vec, V.scalar_sub_vec, V.scalar_mul_vec):  # a: one scalar per batch entry, so the result can only replace b
        ran = run_placements(lambda cfg, ops, out, op=op: op(field, ops[0], ops[1], cfg, out, SIZE, extension), [s, b], b.shape, stream, (1,), what=op.__name__)
        assert ran == 2 * 10 * 2


@pytest.mark.parametrize("field,extension,words,base_words", KINDS, ids=KIND_IDS)
def test_div_and_inv(hip, stream, field, extension, words, base_words):
    from icicle_amd import vecops as V

    rng = np.random.default_rng(12)
    n = SIZE * BATCH
    a, b = elements(field, words, n, rng, zeros=(5,)), elements(field, words, n, rng, zeros=(0, 64, 130, n - 1))  # x / 0 = 0, 0 / x = 0
    run_placements(lambda cfg, ops, out: V.vector_div(field, ops[0], ops[1], cfg, out, SIZE, extension), [a, b], a.shape, stream, (0, 1), what="vector_div")
    run_placements(lambda cfg, ops, out: V.vector_inv(field, ops[0], cfg, out, SIZE, extension), [b], b.shape, stream, (0,), what="vector_inv")


@pytest.mark.parametrize("field,extension,words,base_words", [k for k in KINDS if k[1]], ids=[i for i, k in zip(KIND_IDS, KINDS) if k[1]])
def test_mixed_mul(hip, stream, field, extension, words, base_words):
    from icicle_amd import vecops as V

    rng = np.random.default_rng(13)
    a, b = elements(field, words, SIZE * BATCH, rng), elements(field, base_words, SIZE * BATCH, rng)
    run_placements(lambda cfg, ops, out: V.vector_mixed_mul(field, ops[0], ops[1], cfg, out, SIZE), [a, b], a.shape, stream, what="vector_mixed_mul")


@pytest.mark.parametrize("field,extension,words,base_words", KINDS, ids=KIND_IDS)
def test_sum_and_product(hip, stream, field, extension, words, base_words):
    from icicle_amd import vecops as V

    a = elements(field, words, SIZE * BATCH, np.random.default_rng(14))
    for op in (V.vector_sum, V.vector_product):
        run_placements(lambda cfg, ops, out, op=op: op(field, ops[0], cfg, out, SIZE, extension), [a], (BATCH, words), stream, what=op.__name__)


@pytest.mark.parametrize("field,extension,words,base_words", KINDS, ids=KIND_IDS)
def test_bit_reverse_transpose_and_convert(hip, stream, field, extension, words, base_words):
    from icicle_amd import vecops as V

    rng = np.random.default_rng(15)
    a = elements(field, words, 64 * BATCH, rng)
    run_placements(lambda cfg, ops, out: V.bit_reverse(field, ops[0], cfg, out, 64, extension), [a], a.shape, stream, (0,), what="bit_reverse")
    m = elements(field, words, 37 * 5 * BATCH, rng)
    run_placements(lambda cfg, ops, out: V.matrix_transpose(field, ops[0], 37, 5, cfg, out, extension), [m], m.shape, stream, (0,), layouts=(False,), what="matrix_transpose")
    c = elements(field, words, SIZE * BATCH, rng)
    for to_montgomery in (True, False):
        run_placements(lambda cfg, ops, out: V.scalar_convert_montgomery(field, ops[0], to_montgomery, cfg, out, SIZE, extension), [c], c.shape, stream, (0,),
                       what=f"scalar_convert_montgomery({to_montgomery})")


@pytest.mark.parametrize("field,extension,words,base_words", BASE_KINDS, ids=BASE_IDS)
def test_slice_degree_and_eval(hip, stream, field, extension, words, base_words):
    from icicle_amd import vecops as V

    rng = np.random.default_rng(16)
    a = elements(field, words, SIZE * BATCH, rng)
    run_placements(lambda cfg, ops, out: V.slice(field, ops[0], 1, 2, 33, cfg, out, SIZE), [a], (33 * BATCH, words), stream, what="slice")  # elements 1, 3 ... 65
    z = elements(field, words, SIZE * BATCH, rng, zeros=range(SIZE * BATCH - 7, SIZE * BATCH))  # the top of an entry, or of all of them, is zero
    run_placements(lambda cfg, ops, out: V.highest_non_zero_idx(field, ops[0], cfg, SIZE, out), [z], (BATCH,), stream, out_dtype=np.int64, what="highest_non_zero_idx")
    d = elements(field, words, SIZE, rng)
    run_placements(lambda cfg, ops, out: V.poly_eval(field, ops[0], ops[1], cfg, out, SIZE, 0, SIZE), [a, d], a.shape, stream, what="poly_eval")
