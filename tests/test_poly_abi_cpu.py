"""CPU: the C ABI's surface of slice / highest_non_zero_idx / poly_eval / poly_division -- header, library and binding agree, the tile
query needs no device, and every argument error is returned before the device is touched (there is none here), in vector_inv's order:
NULL config, then the empty call, then a NULL vector, then everything else."""
import ctypes
import re

import numpy as np

from tests import poly_ref as R

SUCCESS, INVALID_POINTER, INVALID_ARGUMENT = 0, 3, 11


def test_symbols_are_declared_exported_and_bound():
    from icicle_amd import _lib
    from tests.test_abi import declared_symbols

    want = {f"{f}_{op}" for f in R.ALL for op in ("slice", "highest_non_zero_idx", "poly_eval", "poly_division")}
    want |= {"icicle_hip_poly_division_tile"}
    assert want <= set(declared_symbols()) and want <= set(_lib.API_SYMBOLS)
    for s in want:
        assert getattr(_lib.lib, s).argtypes is not None, s
    # no other field grew such a function by accident, and extension_slice is not part of this library
    assert {s for s in _lib.API_SYMBOLS if re.search(r"_(slice|highest_non_zero_idx|poly_eval|poly_division)$", s)} == want - {"icicle_hip_poly_division_tile"}


def test_tile_query_needs_no_device():
    from icicle_amd import vecops as V
    from icicle_amd._lib import lib

    tiles = [lib.icicle_hip_poly_division_tile(w) for w in range(0, 17)]
    assert tiles[1] == tiles[2] == tiles[8] > 1 and not any(t for w, t in enumerate(tiles) if w not in (1, 2, 8))
    assert all(V.poly_division_tile(f) == tiles[R.FIELDS[f]] for f in R.ALL)


def test_argument_errors_come_before_the_device():
    from icicle_amd._lib import VecOpsConfig, lib

    for f in R.ALL:
        w = R.FIELDS[f]
        a, b = np.zeros((8, w), np.uint32), np.zeros((8, w), np.uint32)
        q, r = np.full((8, w), 0xA5A5A5A5, np.uint32), np.full((8, w), 0xA5A5A5A5, np.uint32)
        cfg = VecOpsConfig.default()
        c = ctypes.byref(cfg)
        A, B, Q, Rr = a.ctypes.data, b.ctypes.data, q.ctypes.data, r.ctypes.data
        sl = getattr(lib, f"{f}_slice")
        assert sl(A, 0, 1, 8, 4, None, Q) == INVALID_POINTER and sl(A, 0, 1, 8, 0, None, Q) == INVALID_POINTER
        assert sl(None, 99, 1, 8, 0, c, None) == SUCCESS  # the empty call comes before the vectors and the bound
        assert sl(None, 0, 1, 8, 4, c, Q) == INVALID_POINTER and sl(A, 0, 1, 8, 4, c, None) == INVALID_POINTER and sl(None, 5, 1, 8, 4, c, Q) == INVALID_POINTER
        assert sl(A, 5, 1, 8, 4, c, Q) == INVALID_ARGUMENT and sl(A, 8, 0, 8, 2, c, Q) == INVALID_ARGUMENT and sl(A, 1, 7, 8, 3, c, Q) == INVALID_ARGUMENT
        assert sl(A, 0, 1, 8, 4, c, A + 4 * w) == INVALID_ARGUMENT  # overlap
        hz = getattr(lib, f"{f}_highest_non_zero_idx")
        assert hz(A, 8, None, Q) == INVALID_POINTER and hz(None, 8, c, Q) == INVALID_POINTER and hz(A, 8, c, None) == INVALID_POINTER
        assert hz(A, 0, c, Q) == INVALID_ARGUMENT and hz(None, 0, c, Q) == INVALID_POINTER
        ev = getattr(lib, f"{f}_poly_eval")
        assert ev(A, 8, B, 4, None, Q) == INVALID_POINTER
        assert ev(None, 8, B, 4, c, Q) == ev(A, 8, None, 4, c, Q) == ev(A, 8, B, 4, c, None) == INVALID_POINTER
        assert ev(A, 0, B, 4, c, Q) == INVALID_ARGUMENT and ev(A, 8, B, 0, c, Q) == INVALID_ARGUMENT and ev(None, 0, B, 0, c, Q) == INVALID_POINTER
        assert ev(A, 4, B, 4, c, A + 4 * w) == INVALID_ARGUMENT and ev(A, 4, B, 4, c, B) == INVALID_ARGUMENT  # evals inside coeffs, evals on the domain
        ext = lib.create_config_extension()
        try:
            cfg.ext = ext
            for key, want in ((-2, INVALID_ARGUMENT), (-100, INVALID_ARGUMENT)):
                lib.config_extension_set_int(ext, b"hip_poly_eval_chunk", key)
                assert ev(A, 8, B, 4, ctypes.byref(cfg), Q) == want, (f, key)
        finally:
            cfg.ext = None
            lib.destroy_config_extension(ext)
        dv = getattr(lib, f"{f}_poly_division")
        assert dv(A, 8, B, 2, None, Q, 8, Rr, 8) == INVALID_POINTER
        assert dv(None, 8, B, 2, c, Q, 8, Rr, 8) == dv(A, 8, None, 2, c, Q, 8, Rr, 8) == dv(A, 8, B, 2, c, None, 8, Rr, 8) == dv(A, 8, B, 2, c, Q, 8, None, 8) == INVALID_POINTER
        assert dv(A, 0, B, 2, c, Q, 8, Rr, 8) == INVALID_ARGUMENT and dv(A, 8, B, 0, c, Q, 8, Rr, 8) == INVALID_ARGUMENT and dv(A, 8, B, -3, c, Q, 8, Rr, 8) == INVALID_ARGUMENT
        assert dv(None, 0, B, 0, c, Q, 8, Rr, 8) == INVALID_POINTER
        assert dv(A, 8, B, 2, c, A + 4 * w, 4, Rr, 8) == INVALID_ARGUMENT and dv(A, 8, B, 2, c, Q, 8, B, 8) == INVALID_ARGUMENT and dv(A, 8, B, 2, c, Q, 8, Q + 4 * w, 4) == INVALID_ARGUMENT
        assert (q == 0xA5A5A5A5).all() and (r == 0xA5A5A5A5).all()
