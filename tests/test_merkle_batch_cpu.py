"""CPU: batched Merkle openings and verification without a GPU -- the index function the gather kernel and the host share
(icicle_amd/csrc/merkle_batch.h, compiled with g++ plainly and with -fsanitize=address,undefined as a program of its own:
tests/merkle_batch_harness.cpp) against the loop form of the proof plan, which the harness carries as reference code, for every leaf
index of small trees, the staging record's layout, the two entry points in header, library and binding, and the refusals that precede
the device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SUCCESS, INVALID_POINTER, INVALID_ARGUMENT = 0, 3, 11
NAMES = ("icicle_hip_merkle_tree_get_proofs", "icicle_hip_merkle_tree_verify_batch")


def build_harness(name, flags):
    exe = os.path.join(HERE, "_build", name)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    src = os.path.join(HERE, "merkle_batch_harness.cpp")
    hdrs = [os.path.join(ROOT, "icicle_amd", "csrc", h) for h in ("merkle_batch.h", "merkle_plan.h")]
    if not os.path.exists(exe) or max(os.path.getmtime(f) for f in [src] + hdrs) > os.path.getmtime(exe):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", *flags, src, "-o", exe])
    return exe


def run_harness(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "ok 15", lines[-5:]
    return lines


def test_index_function_matches_the_proof_plan_for_every_index():
    lines = run_harness(build_harness("merkle_batch_harness", []))
    # one line per tree, each with checks made: 1-, 2- and 6-layer trees
    assert sorted({int(l.split()[1]) for l in lines[:-1]}) == [1, 2, 3, 6]
    assert all(int(l.split()[-1]) > 0 for l in lines[:-1])


def test_index_function_under_address_and_undefined_behaviour_sanitizers():
    """the same program, instrumented: a finding makes it exit non-zero with a report on stderr"""
    run_harness(build_harness("merkle_batch_harness_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan"]))


def test_index_header_has_no_hip():
    text = open(os.path.join(ROOT, "icicle_amd", "csrc", "merkle_batch.h")).read()
    assert "hip/" not in text and "hipMemcpy" not in text and "__global__" not in text


def test_entry_points_are_declared_exported_and_bound():
    from icicle_amd import _lib
    from icicle_amd.merkle import MerkleTree

    text = re.sub(r"\s+", " ", subprocess.check_output(["gcc", "-E", "-P", os.path.join(ROOT, "include", "icicle_hip.h")], text=True))
    want = {
        NAMES[0]: ["icicle_merkle_tree_handle_t tree", "const uint8_t* leaves", "uint64_t leaves_size", "const uint64_t* leaf_indices", "uint64_t count", "_Bool is_pruned",
                   "const icicle_merkle_tree_config_t* config", "icicle_merkle_proof_handle_t* proofs"],
        NAMES[1]: ["icicle_merkle_tree_handle_t tree", "const icicle_merkle_proof_handle_t* proofs", "uint64_t count", "_Bool* valid"],
    }
    for name, params in want.items():
        m = re.search(r"icicle_error_t %s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, name
        assert [p.strip() for p in m.group(1).split(",")] == params
        assert name in _lib.API_SYMBOLS
        assert getattr(_lib.lib, name) is not None  # exported
    u64, vp = ctypes.c_uint64, ctypes.c_void_p
    assert _lib.lib.icicle_hip_merkle_tree_get_proofs.argtypes == [vp, vp, u64, ctypes.POINTER(u64), u64, ctypes.c_bool, ctypes.POINTER(_lib.MerkleTreeConfig),
                                                                  ctypes.POINTER(vp)]
    assert _lib.lib.icicle_hip_merkle_tree_verify_batch.argtypes == [vp, ctypes.POINTER(vp), u64, ctypes.POINTER(ctypes.c_bool)]
    assert callable(MerkleTree.proofs) and callable(MerkleTree.verify_batch)
    assert not re.search(r"merkle_tree_get_proofs|merkle_tree_verify_batch", open(os.path.join(ROOT, "plugin", "hip_c_api.h")).read())  # no plugin registration


@pytest.fixture()
def tree():
    from icicle_amd.hash import Hasher
    from icicle_amd.merkle import MerkleTree

    t = MerkleTree([Hasher.keccak256(4), Hasher.keccak256(64), Hasher.keccak256(64)], 4)  # 4 leaves of 4 bytes; full path 128, pruned 64
    yield t
    t.close()


def handles(proofs):
    return (ctypes.c_void_p * len(proofs))(*[p.handle if p is not None else None for p in proofs])


def is_empty(p):
    return (p.pruned, p.leaf_idx, p.leaf, p.path, p.root) == (False, 0, b"", b"", b"")


def test_get_proofs_refusals_precede_the_device(tree):
    import icicle_amd
    from icicle_amd._lib import lib
    from icicle_amd.merkle import MerkleProof

    cfg = icicle_amd.MerkleTreeConfig.default()
    leaves = (ctypes.c_uint8 * 16)()
    idx = (ctypes.c_uint64 * 2)(0, 3)
    prs = [MerkleProof(), MerkleProof()]
    call = lib.icicle_hip_merkle_tree_get_proofs
    assert call(None, leaves, 16, idx, 2, False, ctypes.byref(cfg), handles(prs)) == INVALID_POINTER
    assert call(tree.handle, leaves, 16, idx, 2, False, None, handles(prs)) == INVALID_POINTER
    assert call(tree.handle, leaves, 16, None, 2, False, ctypes.byref(cfg), handles(prs)) == INVALID_POINTER
    assert call(tree.handle, leaves, 16, idx, 2, False, ctypes.byref(cfg), None) == INVALID_POINTER
    assert call(tree.handle, leaves, 16, idx, 2, False, ctypes.byref(cfg), handles([prs[0], None])) == INVALID_POINTER
    assert call(tree.handle, None, 16, idx, 2, False, ctypes.byref(cfg), handles(prs)) == INVALID_POINTER
    # no index at all: nothing to do, with or without a device, built or not
    assert call(tree.handle, leaves, 16, idx, 0, False, ctypes.byref(cfg), handles(prs)) == SUCCESS
    assert tree.proofs(np.zeros(16, np.uint8), []) == []
    # a tree that has not been built: refused with the proofs untouched
    assert call(tree.handle, leaves, 16, idx, 2, False, ctypes.byref(cfg), handles(prs)) == INVALID_ARGUMENT
    assert all(is_empty(p) for p in prs)


def test_verify_batch_refusals_precede_the_device(tree):
    from icicle_amd._lib import lib
    from icicle_amd.merkle import MerkleProof

    root = bytes(32)
    full = [MerkleProof.with_data(False, i, b"leaf", root, bytes(128)) for i in range(3)]
    pruned = MerkleProof.with_data(True, 1, b"leaf", root, bytes(64))
    ok = (ctypes.c_bool * 4)(True, True, True, True)
    call = lib.icicle_hip_merkle_tree_verify_batch
    assert call(None, handles(full), 3, ok) == INVALID_POINTER
    assert call(tree.handle, None, 3, ok) == INVALID_POINTER
    assert call(tree.handle, handles(full), 3, None) == INVALID_POINTER
    assert call(tree.handle, handles([full[0], None, full[2]]), 3, ok) == INVALID_POINTER
    assert call(tree.handle, handles(full), 0, ok) == SUCCESS
    assert tree.verify_batch([]) == []
    assert list(ok) == [True] * 4  # none of these calls wrote a verdict
    # one pruned flag per batch
    assert call(tree.handle, handles(full + [pruned]), 4, ok) == INVALID_ARGUMENT
    assert list(ok) == [False] * 4
    # the single call's errors: the first in index order, every verdict false
    for bad in (MerkleProof.with_data(False, 1, b"", root, bytes(128)),           # an empty leaf
                MerkleProof.with_data(False, 1, b"leaf", root, bytes(127)),       # a path of the wrong size
                MerkleProof.with_data(False, -1, b"leaf", root, bytes(128))):     # leaf_idx * 4 beyond 64 bits
        ok = (ctypes.c_bool * 4)(True, True, True, True)
        assert call(tree.handle, handles([full[0], bad, full[2]]), 3, ok) == INVALID_ARGUMENT
        assert list(ok) == [False, False, False, True]  # the three of the batch
    # a root of another size is no root of this tree: invalid, no error, and no device needed to say so
    short = [MerkleProof.with_data(False, i, b"leaf", bytes(31), bytes(128)) for i in range(2)]
    ok = (ctypes.c_bool * 2)(True, True)
    assert call(tree.handle, handles(short), 2, ok) == SUCCESS
    assert list(ok) == [False, False]


def test_gather_and_scatter_kernels_are_present_and_do_not_use_scratch(tmp_path):
    """ISA lint, the method of tests/test_fri_wide_isa.py: private_segment_fixed_size == 0 in the gfx950 code objects of the library"""
    import importlib.util

    lib_path = os.path.join(ROOT, "icicle_amd", "lib", "libicicle_hip.so")
    assert os.path.exists(lib_path), "library not built"
    kernels = {"k_merkle_gather", "k_merkle_scatter"}
    spec = importlib.util.spec_from_file_location("kernel_regs", os.path.join(ROOT, "tools", "kernel_regs.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    rows = [k for co in kr.code_objects(lib_path, str(tmp_path)) for k in kr.kernels(co)]
    dm = kr.demangle([r["name"] for r in rows])
    seen, bad = set(), []
    for r in rows:
        name = re.sub(r"\(.*", "", dm[r["name"]]).replace("icicle_hip::", "").replace("void ", "")
        if name in kernels:
            seen.add(name)
            scratch = int(r.get("private_segment_fixed_size", 0))
            if scratch != 0:
                bad.append(f"{name}: {scratch} B of scratch per lane, {r.get('vgpr_count')} VGPRs")
    assert not bad, "\n".join(bad)
    assert seen == kernels, f"kernels not found in the library: {sorted(kernels - seen)}"
