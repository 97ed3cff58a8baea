"""Montgomery-form conversion on device: mirror of wrappers/rust/icicle-core/src/vec_ops (convert_montgomery)
and icicle-core/src/curve (Affine/Projective to_mont / from_mont)."""
import ctypes
import numpy as np
from ._lib import lib, check, VecOpsConfig
from .runtime import DeviceVec

# u32 words per scalar (a curve name stands for its scalar field) and per base-field coordinate of a point
_WORDS = {"bn254": 8, "bls12_381": 8, "bls12_377": 8, "grumpkin": 8, "stark252": 8, "goldilocks": 2, "babybear": 1, "koalabear": 1}
_EXT_DEGREE = {"babybear": 4, "koalabear": 4, "goldilocks": 2}
_EXT_WORDS = 4  # u32 words per extension element, all three extension types
_POINT_LIMBS = {"bn254": 8, "bls12_381": 12, "bls12_377": 12, "grumpkin": 8}

def _ptr(x):
    if isinstance(x, DeviceVec):
        return x.ptr, True
    if isinstance(x, int):
        return x, True
    assert isinstance(x, np.ndarray) and x.dtype == np.uint32 and x.flags["C_CONTIGUOUS"]
    return x.ctypes.data, False


def _run(symbol, inp, count, to_montgomery, cfg, out):
    cfg = cfg or VecOpsConfig.default()
    ip, i_dev = _ptr(inp)
    cfg.is_a_on_device = i_dev
    if out is None:
        out = np.zeros_like(inp)
    op, o_dev = _ptr(out)
    cfg.is_result_on_device = o_dev
    check(getattr(lib, symbol)(ip, count, to_montgomery, ctypes.byref(cfg), op), symbol)
    return out


def scalar_convert_montgomery(field: str, inp, to_montgomery: bool, cfg=None, out=None, size=None, extension=False):
    """field in _WORDS (a curve name means its scalar field); `size` = elements per batch entry"""
    words = _WORDS[field] * (_EXT_DEGREE[field] if extension else 1)
    if size is None:
        size = inp.size // words // max(1, (cfg.batch_size if cfg else 1))
    sym = f"{field}_extension_scalar_convert_montgomery" if extension else f"{field}_scalar_convert_montgomery"
    return _run(sym, inp, size, to_montgomery, cfg, out)


def affine_convert_montgomery(curve: str, inp, to_montgomery: bool, cfg=None, out=None, n=None):
    L = _POINT_LIMBS[curve]
    return _run(f"{curve}_affine_convert_montgomery", inp, n if n is not None else inp.size // (2 * L), to_montgomery, cfg, out)


def projective_convert_montgomery(curve: str, inp, to_montgomery: bool, cfg=None, out=None, n=None):
    L = _POINT_LIMBS[curve]
    return _run(f"{curve}_projective_convert_montgomery", inp, n if n is not None else inp.size // (3 * L), to_montgomery, cfg, out)


def _sym(field: str, op: str, extension: bool) -> str:
    """the library symbol of `op` over `field` or over its extension field (babybear, koalabear: quartic; goldilocks: quadratic)"""
    if not extension:
        return f"{field}_{op}"
    if field not in _EXT_DEGREE:
        raise ValueError(f"{field} has no extension field: extension=True is for {sorted(_EXT_DEGREE)}")
    return f"{field}_extension_{op}"


def _words(field: str, extension: bool) -> int:
    return _EXT_WORDS if extension else _WORDS[field]


def _vec2(op: str, field: str, a, b, size, cfg, out, extension=False, b_words=None):
    """mirror of wrappers/rust/icicle-core/src/vec_ops: add / sub / mul / scalar-mul of field vectors"""
    sym = _sym(field, op, extension)
    cfg = cfg or VecOpsConfig.default()
    ap, cfg.is_a_on_device = _ptr(a)
    bp, cfg.is_b_on_device = _ptr(b)
    words = _words(field, extension)
    if size is None:
        size = b.size // (b_words or words) // max(1, cfg.batch_size)
    if out is None:
        out = np.zeros((size * max(1, cfg.batch_size), words), np.uint32) if b_words else np.zeros_like(b)
    op_, cfg.is_result_on_device = _ptr(out)
    check(getattr(lib, sym)(ap, bp, size, ctypes.byref(cfg), op_), sym)
    return out


def vector_add(field, a, b, cfg=None, out=None, size=None, extension=False):
    return _vec2("vector_add", field, a, b, size, cfg, out, extension)


def vector_sub(field, a, b, cfg=None, out=None, size=None, extension=False):
    return _vec2("vector_sub", field, a, b, size, cfg, out, extension)


def vector_mul(field, a, b, cfg=None, out=None, size=None, extension=False):
    return _vec2("vector_mul", field, a, b, size, cfg, out, extension)


def vector_mixed_mul(field, a_ext, b_base, cfg=None, out=None, size=None):
    """a_ext[i] * b_base[i]: an extension vector ([n, 4] words) times a base-field vector of `field`; the result is an extension vector"""
    return _vec2("vector_mixed_mul", field, a_ext, b_base, size, cfg, out, True, b_words=_WORDS[field])


def scalar_mul_vec(field, scalars, b, cfg=None, out=None, size=None, extension=False):
    """scalars: one per batch entry"""
    return _vec2("scalar_mul_vec", field, scalars, b, size, cfg, out, extension)


def scalar_add_vec(field, scalars, b, cfg=None, out=None, size=None, extension=False):
    """scalar[k] + b[i] for every element of batch entry k; scalars: one per batch entry"""
    return _vec2("scalar_add_vec", field, scalars, b, size, cfg, out, extension)


def scalar_sub_vec(field, scalars, b, cfg=None, out=None, size=None, extension=False):
    """scalar[k] - b[i] (the scalar is the minuend); scalars: one per batch entry"""
    return _vec2("scalar_sub_vec", field, scalars, b, size, cfg, out, extension)


def vector_div(field, a, b, cfg=None, out=None, size=None, extension=False):
    """a[i] / b[i], with x / 0 = 0; in place allowed (out is a or b)"""
    return _vec2("vector_div", field, a, b, size, cfg, out, extension)


def _vec1(op: str, field: str, a, size, cfg, out, reduces: bool, extension=False):
    """vector_inv (one output element per input element) and vector_sum / vector_product (one per batch entry, [batch, words])"""
    sym = _sym(field, op, extension)
    words = _words(field, extension)
    cfg = cfg or VecOpsConfig.default()
    ap, cfg.is_a_on_device = _ptr(a)
    batch = max(1, cfg.batch_size)
    if size is None:
        assert not isinstance(a, int), "a raw device address has no size: pass size"
        size = a.nbytes // (4 * words) // batch
    if out is None:
        if reduces:
            out = np.zeros((batch, words), np.uint32)
        else:
            out = np.zeros_like(a) if isinstance(a, np.ndarray) else np.zeros((size * batch, words), np.uint32)
    op_, cfg.is_result_on_device = _ptr(out)
    check(getattr(lib, sym)(ap, size, ctypes.byref(cfg), op_), sym)
    return out


def vector_inv(field, a, cfg=None, out=None, size=None, extension=False):
    """1 / a[i], with 1 / 0 = 0; in place allowed (out is a)"""
    return _vec1("vector_inv", field, a, size, cfg, out, False, extension)


def vector_sum(field, a, cfg=None, out=None, size=None, extension=False):
    """the sum of each batch entry (element j of entry k at k * size + j, or at j * batch_size + k with columns_batch): [batch, words]"""
    return _vec1("vector_sum", field, a, size, cfg, out, True, extension)


def vector_product(field, a, cfg=None, out=None, size=None, extension=False):
    """the product of each batch entry, laid out like vector_sum's: [batch, words]"""
    return _vec1("vector_product", field, a, size, cfg, out, True, extension)


def vector_inv_tile(field) -> int:
    """how many neighbouring elements of `field` share one inversion in vector_inv / vector_div"""
    return lib.icicle_hip_vector_inv_tile(_WORDS[field])


def extension_vector_inv_tile(field) -> int:
    """how many neighbouring extension elements of `field` share one base-field inversion of their norms in vector_inv / vector_div"""
    _sym(field, "vector_inv", True)
    return lib.icicle_hip_extension_vector_inv_tile(_WORDS[field])


def bit_reverse(field, inp, cfg=None, out=None, size=None, extension=False):
    sym = _sym(field, "bit_reverse", extension)
    cfg = cfg or VecOpsConfig.default()
    ip, cfg.is_a_on_device = _ptr(inp)
    if size is None:
        size = inp.size // _words(field, extension) // max(1, cfg.batch_size)
    if out is None:
        out = np.zeros_like(inp)
    op_, cfg.is_result_on_device = _ptr(out)
    check(getattr(lib, sym)(ip, size, ctypes.byref(cfg), op_), sym)
    return out


def matrix_transpose(field, inp, nof_rows: int, nof_cols: int, cfg=None, out=None, extension: bool = False):
    """batch_size row-major nof_rows x nof_cols matrices -> their transposes (icicle/include/icicle/vec_ops.h:319,
    src/matrix_ops.cpp:75-102); in place allowed, columns_batch rejected like the reference CPU backend does"""
    cfg = cfg or VecOpsConfig.default()
    ip, cfg.is_a_on_device = _ptr(inp)
    if out is None:
        out = np.zeros_like(inp)
    op_, cfg.is_result_on_device = _ptr(out)
    name = f"{field}_extension_matrix_transpose" if extension else f"{field}_matrix_transpose"
    check(getattr(lib, name)(ip, nof_rows, nof_cols, ctypes.byref(cfg), op_), name)
    return out


def execute_program(field, data, program, cfg=None, size=None):
    """data: one vector per parameter of `program` (program.Program or sumcheck.ReturningValueProgram), all NumPy uint32 arrays on the
    host or all on the device (DeviceVec, or an int: a device address, then with `size`); the parameters the program writes are written in place. `size` = elements per batch entry."""
    cfg = cfg or VecOpsConfig.default()
    ptrs = [_ptr(d) for d in data]
    assert ptrs and len({dev for _, dev in ptrs}) == 1, "parameters must be all on the host or all on the device"
    cfg.is_a_on_device = cfg.is_b_on_device = cfg.is_result_on_device = ptrs[0][1]
    if size is None:
        assert not isinstance(data[0], int), "a raw device address has no size: pass size"
        size = data[0].nbytes // (4 * _WORDS[field]) // max(1, cfg.batch_size)
    table = (ctypes.c_void_p * len(ptrs))(*[p for p, _ in ptrs])
    check(getattr(lib, f"{field}_execute_program")(table, len(ptrs), program.handle, size, ctypes.byref(cfg)), f"{field}_execute_program")
    return data


# ---- slice, highest_non_zero_idx, poly_eval, poly_division (src/vec_ops.cpp:472-677): what the reference's polynomial API is built from ----
def _elements(x, words, what):
    assert not isinstance(x, int), f"a raw device address has no size: pass {what}"
    return x.nbytes // (4 * words)


def slice(field, inp, offset, stride, size_out, cfg=None, out=None, size_in=None):
    """out[k][i] = inp[k][offset + i * stride], i < size_out, per batch entry of `size_in` elements; inp and out must not overlap"""
    sym = f"{field}_slice"
    words = _WORDS[field]
    cfg = cfg or VecOpsConfig.default()
    ip, cfg.is_a_on_device = _ptr(inp)
    batch = max(1, cfg.batch_size)
    if size_in is None:
        size_in = _elements(inp, words, "size_in") // batch
    if out is None:
        out = np.zeros((size_out * batch, words), np.uint32)
    op_, cfg.is_result_on_device = _ptr(out)
    check(getattr(lib, sym)(ip, offset, stride, size_in, size_out, ctypes.byref(cfg), op_), sym)
    return out


def highest_non_zero_idx(field, a, cfg=None, size=None, out=None):
    """per batch entry the largest index of a non-zero element, -1 for a zero vector: an int64 array of batch_size values
    (`out`: a DeviceVec or device address of batch_size int64 to keep the result on the device)"""
    sym = f"{field}_highest_non_zero_idx"
    cfg = cfg or VecOpsConfig.default()
    ap, cfg.is_a_on_device = _ptr(a)
    batch = max(1, cfg.batch_size)
    if size is None:
        size = _elements(a, _WORDS[field], "size") // batch
    if out is None:
        out = np.full(batch, -2, np.int64)
    if isinstance(out, np.ndarray):
        assert out.dtype == np.int64 and out.flags["C_CONTIGUOUS"]
        op_, cfg.is_result_on_device = out.ctypes.data, False
    else:
        op_, cfg.is_result_on_device = _ptr(out)
    check(getattr(lib, sym)(ap, size, ctypes.byref(cfg), op_), sym)
    return out


def poly_eval(field, coeffs, domain, cfg=None, out=None, coeffs_size=None, chunk=0, domain_size=None):
    """out[k][e] = P_k(domain[e]): coefficients per batch entry (constant term first), one domain shared by the entries.
    chunk: 0 = the library picks the route, > 0 = the chunk route with that chunk length, -1 = one lane per (entry, point)"""
    sym = f"{field}_poly_eval"
    words = _WORDS[field]
    cfg = cfg or VecOpsConfig.default()
    cp, cfg.is_a_on_device = _ptr(coeffs)
    dp, cfg.is_b_on_device = _ptr(domain)
    batch = max(1, cfg.batch_size)
    if coeffs_size is None:
        coeffs_size = _elements(coeffs, words, "coeffs_size") // batch
    if domain_size is None:
        domain_size = _elements(domain, words, "domain_size")
    if out is None:
        out = np.zeros((domain_size * batch, words), np.uint32)
    op_, cfg.is_result_on_device = _ptr(out)
    ext, saved = None, cfg.ext
    if chunk:
        ext = lib.clone_config_extension(saved) if saved else lib.create_config_extension()
        lib.config_extension_set_int(ext, b"hip_poly_eval_chunk", chunk)
        cfg.ext = ext
    try:
        check(getattr(lib, sym)(cp, coeffs_size, dp, domain_size, ctypes.byref(cfg), op_), sym)
    finally:
        if ext:
            cfg.ext = saved
            lib.destroy_config_extension(ext)
    return out


def poly_division(field, num, den, cfg=None, q_size=None, r_size=None, q_out=None, r_out=None, num_size=None, den_size=None):
    """(q, r) with num = q * den + r per batch entry; q has q_size and r has r_size elements per entry, zero above their degrees.
    Defaults: r_size = the numerator's size, q_size = max(1, numerator size - denominator size + 1) -- enough when the
    denominator's buffer has no trailing zeros; pass q_size otherwise. The outputs may not overlap the inputs."""
    sym = f"{field}_poly_division"
    words = _WORDS[field]
    cfg = cfg or VecOpsConfig.default()
    np_, cfg.is_a_on_device = _ptr(num)
    dp, cfg.is_b_on_device = _ptr(den)
    batch = max(1, cfg.batch_size)
    if num_size is None:
        num_size = _elements(num, words, "num_size") // batch
    if den_size is None:
        den_size = _elements(den, words, "den_size") // batch
    if r_size is None:
        r_size = num_size
    if q_size is None:
        q_size = max(1, num_size - den_size + 1)
    if q_out is None:
        q_out = np.zeros((q_size * batch, words), np.uint32)
    if r_out is None:
        r_out = np.zeros((r_size * batch, words), np.uint32)
    qp, q_dev = _ptr(q_out)
    rp, r_dev = _ptr(r_out)
    assert q_dev == r_dev, "q_out and r_out must both be on the host or both on the device"
    cfg.is_result_on_device = q_dev
    check(getattr(lib, sym)(np_, num_size, dp, den_size, ctypes.byref(cfg), qp, q_size, rp, r_size), sym)
    return q_out, r_out


def poly_division_tile(field) -> int:
    """how many quotient coefficients of `field` poly_division produces per pair of launches"""
    return lib.icicle_hip_poly_division_tile(_WORDS[field])
