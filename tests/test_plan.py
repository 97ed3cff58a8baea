"""CPU: the NTT pass decomposition (icicle_amd/csrc/ntt_plan.h) compiled for the host -- every pass covers a row exactly
once and the last pass's scatter is a permutation, for every size up to 2^27 (31-bit fields) / 2^22 (256-bit fields); the
lane-native launch geometry of interleaved transforms (ntt_plan.h fast_pass_geometry, what ntt_run launches) maps every
logical element to the same word with and without column / outer-index groups."""
import ctypes
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def _lib():
    so = os.path.join(HERE, "_build", "libplan.so")
    os.makedirs(os.path.dirname(so), exist_ok=True)
    src = os.path.join(HERE, "plan_harness.cpp")
    hdrs = [os.path.join(HERE, "..", "icicle_amd", "csrc", h) for h in ("ntt_plan.h", "msm_plan.h")]
    if not os.path.exists(so) or max([os.path.getmtime(src)] + [os.path.getmtime(h) for h in hdrs]) > os.path.getmtime(so):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", src, "-o", so])
    return ctypes.CDLL(so)


def test_ntt_plan_covers_every_slot_once():
    lib = _lib()
    assert lib.plan_check(27, 22) == 0
    assert lib.msm_groups_check() == 0  # window groups of the pipelined MSM schedule (msm_plan.h)
    assert lib.split_shape_check() == 0  # shapes of a transform split over device slots (ntt_plan.h)
    assert lib.msm_plan_check() == 0  # the window plan of msm() (msm_plan.h make_plan)
    # ECNTT: stage widths + the radix-2^r matrix-form index algebra, simulated mod a small prime against the O(n^2) definition
    assert lib.ecntt_plan_check() == 0


def test_lane_native_geometry_groups_change_no_address():
    """Interleaved transforms (columns_batch 2..160, 192, 256 columns; the extension field, columns and rows), every size 2^1..2^27,
    kNN / kNR / kRN / kRR, plain and both coset directions: for every pass, grouped launch rows (cg columns in pass 0 / the last pass,
    ag outer indices in the middle one) touch exactly the words the ungrouped pass assigns to the same logical element, never a
    padding lane of the padded work buffer, never a word outside the buffer (tests/plan_harness.cpp lane_plan_check; a non-zero
    value encodes the first failing shape). 48 columns at 2^25..2^27 -- padded work buffer plus groups -- is the case that was
    wrong: the group strides were built from the caller's element stride on the work buffer's side."""
    lib = _lib()
    assert lib.lane_plan_check(1, 27) == 0
