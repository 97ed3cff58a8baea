"""CPU: every vector entry point validates its arguments before it touches the device (there is none here). Each family is called
through ctypes over one field per element kind -- babybear (one word), goldilocks (two), bn254 (eight) and the babybear and goldilocks
extensions (16 bytes) -- and the return code is compared with the literal table below, which is the host frame's contract: the order of
the checks and their codes differ between the families on purpose (each follows the reference line cited beside it in the source)."""
import ctypes

import numpy as np
import pytest

SUCCESS, INVALID_POINTER, INVALID_ARGUMENT = 0, 3, 11

# (field, extension, u32 words per element, u32 words per base-field element)
KINDS = [("babybear", False, 1, 1), ("goldilocks", False, 2, 2), ("bn254", False, 8, 8), ("babybear", True, 4, 1), ("goldilocks", True, 4, 2)]
KIND_IDS = [f"{f}{'_extension' if e else ''}" for f, e, _, _ in KINDS]

TWO_OPERAND = ("vector_add", "vector_sub", "vector_mul", "scalar_add_vec", "scalar_sub_vec", "scalar_mul_vec", "vector_div")
ONE_OPERAND = ("vector_inv", "vector_sum", "vector_product")

# family -> case -> code. "size0_null": size 0 and every vector NULL.
EXPECTED = {
    # vec2_run / inv_run<DIV> / ext_mixed_mul_run: NULL config, then the empty call, then a NULL vector
    "two_operand": {"null_cfg": INVALID_POINTER, "size0": SUCCESS, "size0_null": SUCCESS, "null_a": INVALID_POINTER, "null_b": INVALID_POINTER, "null_out": INVALID_POINTER},
    # inv_run / reduce_run
    "one_operand": {"null_cfg": INVALID_POINTER, "size0": SUCCESS, "size0_null": SUCCESS, "null_a": INVALID_POINTER, "null_out": INVALID_POINTER},
    # convert_run
    "convert": {"null_cfg": INVALID_POINTER, "size0": SUCCESS, "size0_null": SUCCESS, "null_in": INVALID_POINTER, "null_out": INVALID_POINTER},
    # bitrev_run: the vectors come before the size, and no size but a power of two is accepted, 0 included
    "bit_reverse": {"null_cfg": INVALID_POINTER, "size0": INVALID_ARGUMENT, "size0_null": INVALID_POINTER, "null_in": INVALID_POINTER, "null_out": INVALID_POINTER,
                    "size6": INVALID_ARGUMENT},
    # transpose_run: a NULL vector is an argument error here
    "matrix_transpose": {"null_cfg": INVALID_POINTER, "null_in": INVALID_ARGUMENT, "null_out": INVALID_ARGUMENT, "rows0": INVALID_ARGUMENT, "cols0": INVALID_ARGUMENT,
                         "columns_batch": INVALID_ARGUMENT},
    # poly_plan.h, the cases of tests/test_poly_plan.py::test_every_argument_rule
    "slice": {"null_cfg": INVALID_POINTER, "null_cfg_size0": INVALID_POINTER, "size0": SUCCESS, "size0_null": SUCCESS, "null_in": INVALID_POINTER, "null_out": INVALID_POINTER,
              "null_in_out_of_range": INVALID_POINTER, "size_out_too_large": INVALID_ARGUMENT, "offset_too_large": INVALID_ARGUMENT, "size_in_too_small": INVALID_ARGUMENT,
              "stride0_offset_past_end": INVALID_ARGUMENT, "wrap_around": INVALID_ARGUMENT, "overlap": INVALID_ARGUMENT},
    "highest_non_zero_idx": {"null_cfg": INVALID_POINTER, "null_in": INVALID_POINTER, "null_out": INVALID_POINTER, "size0": INVALID_ARGUMENT, "size0_null": INVALID_POINTER},
    "poly_eval": {"null_cfg": INVALID_POINTER, "null_coeffs": INVALID_POINTER, "null_domain": INVALID_POINTER, "null_evals": INVALID_POINTER, "coeffs_size0": INVALID_ARGUMENT,
                  "domain_size0": INVALID_ARGUMENT, "size0_null": INVALID_POINTER, "evals_in_coeffs": INVALID_ARGUMENT, "evals_on_domain": INVALID_ARGUMENT},
    "poly_division": {"null_cfg": INVALID_POINTER, "null_num": INVALID_POINTER, "null_den": INVALID_POINTER, "null_q": INVALID_POINTER, "null_r": INVALID_POINTER,
                      "num_size0": INVALID_ARGUMENT, "den_size0": INVALID_ARGUMENT, "den_size_negative": INVALID_ARGUMENT, "size0_null": INVALID_POINTER,
                      "q_in_num": INVALID_ARGUMENT, "r_on_den": INVALID_ARGUMENT, "r_in_q": INVALID_ARGUMENT},
}

N = 8  # elements per vector
FILL = 0xA5A5A5A5


class Call:
    """the vectors of one call, host arrays that no call may write, and the codes it collected"""

    def __init__(self, words):
        from icicle_amd._lib import VecOpsConfig

        self.a, self.b = np.zeros((N, words), np.uint32), np.zeros((N, words), np.uint32)
        self.o, self.o2 = np.full((N, words), FILL, np.uint32), np.full((N, words), FILL, np.uint32)
        self.A, self.B, self.O, self.O2 = (x.ctypes.data for x in (self.a, self.b, self.o, self.o2))
        self.cfg = VecOpsConfig.default()
        self.c = ctypes.byref(self.cfg)
        self.got = {}

    def check(self, family, what):
        assert self.got == EXPECTED[family], (what, {k: (v, EXPECTED[family].get(k)) for k, v in self.got.items() if v != EXPECTED[family].get(k)})
        assert (self.o == FILL).all() and (self.o2 == FILL).all() and not self.a.any() and not self.b.any(), what


def _sym(field, extension, op):
    from icicle_amd._lib import lib

    return getattr(lib, f"{field}_extension_{op}" if extension else f"{field}_{op}")


@pytest.mark.parametrize("field,extension,words,base_words", KINDS, ids=KIND_IDS)
def test_two_operand_families(field, extension, words, base_words):
    for op in TWO_OPERAND + (("vector_mixed_mul",) if extension else ()):
        fn, k = _sym(field, extension, op), Call(words)
        k.got = {"null_cfg": fn(k.A, k.B, N, None, k.O), "size0": fn(k.A, k.B, 0, k.c, k.O), "size0_null": fn(None, None, 0, k.c, None),
                 "null_a": fn(None, k.B, N, k.c, k.O), "null_b": fn(k.A, None, N, k.c, k.O), "null_out": fn(k.A, k.B, N, k.c, None)}
        k.check("two_operand", (field, extension, op))


@pytest.mark.parametrize("field,extension,words,base_words", KINDS, ids=KIND_IDS)
def test_one_operand_families(field, extension, words, base_words):
    for op in ONE_OPERAND:
        fn, k = _sym(field, extension, op), Call(words)
        k.got = {"null_cfg": fn(k.A, N, None, k.O), "size0": fn(k.A, 0, k.c, k.O), "size0_null": fn(None, 0, k.c, None), "null_a": fn(None, N, k.c, k.O),
                 "null_out": fn(k.A, N, k.c, None)}
        k.check("one_operand", (field, extension, op))


@pytest.mark.parametrize("field,extension,words,base_words", KINDS, ids=KIND_IDS)
def test_scalar_convert_montgomery(field, extension, words, base_words):
    for pre in ("", "icicle_hip_"):
        fn, k = _sym(pre + field, extension, "scalar_convert_montgomery"), Call(words)
        k.got = {"null_cfg": fn(k.A, N, True, None, k.O), "size0": fn(k.A, 0, True, k.c, k.O), "size0_null": fn(None, 0, False, k.c, None),
                 "null_in": fn(None, N, True, k.c, k.O), "null_out": fn(k.A, N, False, k.c, None)}
        k.check("convert", (field, extension, pre))


@pytest.mark.parametrize("field,extension,words,base_words", KINDS, ids=KIND_IDS)
def test_bit_reverse(field, extension, words, base_words):
    fn, k = _sym(field, extension, "bit_reverse"), Call(words)
    k.got = {"null_cfg": fn(k.A, N, None, k.O), "size0": fn(k.A, 0, k.c, k.O), "size0_null": fn(None, 0, k.c, None), "null_in": fn(None, N, k.c, k.O),
             "null_out": fn(k.A, N, k.c, None), "size6": fn(k.A, 6, k.c, k.O)}
    k.check("bit_reverse", (field, extension))


@pytest.mark.parametrize("field,extension,words,base_words", KINDS, ids=KIND_IDS)
def test_matrix_transpose(field, extension, words, base_words):
    for pre in ("", "icicle_hip_"):
        fn, k = _sym(pre + field, extension, "matrix_transpose"), Call(words)
        k.got = {"null_cfg": fn(k.A, 2, 4, None, k.O), "null_in": fn(None, 2, 4, k.c, k.O), "null_out": fn(k.A, 2, 4, k.c, None), "rows0": fn(k.A, 0, 4, k.c, k.O),
                 "cols0": fn(k.A, 2, 0, k.c, k.O)}
        k.cfg.columns_batch = True
        k.got["columns_batch"] = fn(k.A, 2, 4, k.c, k.O)
        k.check("matrix_transpose", (field, extension, pre))


BASE_KINDS = [k for k in KINDS if not k[1]]
BASE_IDS = [k[0] for k in BASE_KINDS]


@pytest.mark.parametrize("field,extension,words,base_words", BASE_KINDS, ids=BASE_IDS)
def test_slice(field, extension, words, base_words):
    """size_in 8: offset 1, stride 2, size_out 3 reads elements 1, 3, 5"""
    fn, k = _sym(field, False, "slice"), Call(words)
    big = (1 << 64) - 1
    k.got = {"null_cfg": fn(k.A, 1, 2, N, 3, None, k.O), "null_cfg_size0": fn(k.A, 1, 2, N, 0, None, k.O), "size0": fn(k.A, 1, 2, N, 0, k.c, k.O),
             "size0_null": fn(None, 99, 2, N, 0, k.c, None), "null_in": fn(None, 1, 2, N, 3, k.c, k.O), "null_out": fn(k.A, 1, 2, N, 3, k.c, None),
             "null_in_out_of_range": fn(None, 1, 2, N, 5, k.c, k.O), "size_out_too_large": fn(k.A, 1, 2, N, 5, k.c, k.O), "offset_too_large": fn(k.A, 4, 2, N, 3, k.c, k.O),
             "size_in_too_small": fn(k.A, 1, 2, 5, 3, k.c, k.O), "stride0_offset_past_end": fn(k.A, N, 0, N, 1, k.c, k.O), "wrap_around": fn(k.A, big, big, N, big, k.c, k.O),
             "overlap": fn(k.A, 1, 2, N, 3, k.c, k.A + 4 * words)}
    k.check("slice", field)


@pytest.mark.parametrize("field,extension,words,base_words", BASE_KINDS, ids=BASE_IDS)
def test_highest_non_zero_idx(field, extension, words, base_words):
    fn, k = _sym(field, False, "highest_non_zero_idx"), Call(words)
    k.got = {"null_cfg": fn(k.A, N, None, k.O), "null_in": fn(None, N, k.c, k.O), "null_out": fn(k.A, N, k.c, None), "size0": fn(k.A, 0, k.c, k.O),
             "size0_null": fn(None, 0, k.c, k.O)}
    k.check("highest_non_zero_idx", field)


@pytest.mark.parametrize("field,extension,words,base_words", BASE_KINDS, ids=BASE_IDS)
def test_poly_eval(field, extension, words, base_words):
    fn, k = _sym(field, False, "poly_eval"), Call(words)
    k.got = {"null_cfg": fn(k.A, N, k.B, 4, None, k.O), "null_coeffs": fn(None, N, k.B, 4, k.c, k.O), "null_domain": fn(k.A, N, None, 4, k.c, k.O),
             "null_evals": fn(k.A, N, k.B, 4, k.c, None), "coeffs_size0": fn(k.A, 0, k.B, 4, k.c, k.O), "domain_size0": fn(k.A, N, k.B, 0, k.c, k.O),
             "size0_null": fn(None, 0, k.B, 0, k.c, k.O), "evals_in_coeffs": fn(k.A, 4, k.B, 4, k.c, k.A + 4 * words), "evals_on_domain": fn(k.A, 4, k.B, 4, k.c, k.B)}
    k.check("poly_eval", field)


@pytest.mark.parametrize("field,extension,words,base_words", BASE_KINDS, ids=BASE_IDS)
def test_poly_division(field, extension, words, base_words):
    fn, k = _sym(field, False, "poly_division"), Call(words)
    k.got = {"null_cfg": fn(k.A, N, k.B, 2, None, k.O, N, k.O2, N), "null_num": fn(None, N, k.B, 2, k.c, k.O, N, k.O2, N), "null_den": fn(k.A, N, None, 2, k.c, k.O, N, k.O2, N),
             "null_q": fn(k.A, N, k.B, 2, k.c, None, N, k.O2, N), "null_r": fn(k.A, N, k.B, 2, k.c, k.O, N, None, N), "num_size0": fn(k.A, 0, k.B, 2, k.c, k.O, N, k.O2, N),
             "den_size0": fn(k.A, N, k.B, 0, k.c, k.O, N, k.O2, N), "den_size_negative": fn(k.A, N, k.B, -3, k.c, k.O, N, k.O2, N),
             "size0_null": fn(None, 0, k.B, 0, k.c, k.O, N, k.O2, N), "q_in_num": fn(k.A, N, k.B, 2, k.c, k.A + 4 * words, 4, k.O2, N),
             "r_on_den": fn(k.A, N, k.B, 2, k.c, k.O, N, k.B, N), "r_in_q": fn(k.A, N, k.B, 2, k.c, k.O, N, k.O + 4 * words, 4)}
    k.check("poly_division", field)
