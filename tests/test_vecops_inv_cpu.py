"""CPU: vector_inv / vector_div / vector_sum / vector_product are declared in include/icicle_hip.h with the reference's argument lists
(src/vec_ops.cpp:9, 40, 217, 250), exported, bound and reachable from the package, and their argument checks answer before a device
is needed: NULL config, then size == 0 (success, nothing written), then a NULL vector."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = {"babybear": 1, "koalabear": 1, "goldilocks": 2, "bn254": 8, "bls12_381": 8, "bls12_377": 8, "stark252": 8, "grumpkin": 8}  # words
FUNCTIONS = {"vector_inv": 4, "vector_div": 5, "vector_sum": 4, "vector_product": 4}  # name -> number of arguments
INVALID_POINTER = 3


def test_functions_are_declared_exported_and_bound():
    from icicle_amd import _lib
    import icicle_amd

    text = re.sub(r"\s+", " ", subprocess.check_output(["gcc", "-E", "-P", os.path.join(ROOT, "include", "icicle_hip.h")], text=True))
    for f in FIELDS:
        for name, n in FUNCTIONS.items():
            m = re.search(r"icicle_error_t %s_%s\s*\(([^)]*)\)\s*;" % (f, name), text)
            assert m and len(m.group(1).split(",")) == n, (f, name)
            assert f"{f}_{name}" in _lib.API_SYMBOLS and len(getattr(_lib.lib, f"{f}_{name}").argtypes) == n
            assert f"icicle_hip_{f}_{name}" not in text and not hasattr(_lib.lib, f"icicle_hip_{f}_{name}")  # no aliases: the plugin is out of scope
    m = re.search(r"int icicle_hip_vector_inv_tile\s*\(([^)]*)\)\s*;", text)
    assert m and len(m.group(1).split(",")) == 1
    assert "icicle_hip_vector_inv_tile" in _lib.API_SYMBOLS and len(_lib.lib.icicle_hip_vector_inv_tile.argtypes) == 1
    for name in FUNCTIONS:
        assert callable(getattr(icicle_amd, name)) and getattr(icicle_amd, name) is getattr(icicle_amd.vecops, name), name


def test_tile_covers_at_least_256_elements():
    from icicle_amd import vecops as V
    from icicle_amd._lib import lib

    for words in (1, 2, 8):
        assert lib.icicle_hip_vector_inv_tile(words) >= 256, words
    for words in (0, 3, 4, 16, -1):
        assert lib.icicle_hip_vector_inv_tile(words) == 0, words
    for f, words in FIELDS.items():
        assert V.vector_inv_tile(f) == lib.icicle_hip_vector_inv_tile(words)


@pytest.mark.parametrize("field", list(FIELDS))
def test_argument_checks_need_no_device(field):
    from icicle_amd._lib import lib, VecOpsConfig

    words = FIELDS[field]
    a = np.ones((4, words), np.uint32)
    b = np.ones((4, words), np.uint32)
    sentinel = 0xA5A5A5A5
    for name, n in FUNCTIONS.items():
        fn = getattr(lib, f"{field}_{name}")
        out = np.full((4, words), sentinel, np.uint32)
        cfg = VecOpsConfig.default()

        def call(size, cfg_ref, a_ptr=a.ctypes.data, b_ptr=b.ctypes.data, o_ptr=out.ctypes.data):
            args = (a_ptr, b_ptr) if n == 5 else (a_ptr,)
            return fn(*args, size, cfg_ref, o_ptr)

        assert call(4, None) == INVALID_POINTER, name
        assert call(0, None) == INVALID_POINTER, name  # the config is looked at first
        assert call(0, ctypes.byref(cfg)) == 0 and (out == sentinel).all(), name
        assert call(0, ctypes.byref(cfg), a_ptr=None, o_ptr=None) == 0, name  # size == 0 answers before the vectors are looked at
        assert call(4, ctypes.byref(cfg), a_ptr=None) == INVALID_POINTER, name
        assert call(4, ctypes.byref(cfg), o_ptr=None) == INVALID_POINTER, name
        if n == 5:
            assert call(4, ctypes.byref(cfg), b_ptr=None) == INVALID_POINTER, name
        assert (out == sentinel).all(), name

