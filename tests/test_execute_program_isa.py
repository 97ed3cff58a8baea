"""ISA lint (CPU only), the method of tests/test_sumcheck_isa.py: the execute_program kernels of all four fields are in the gfx950 code
objects embedded in libicicle_hip.so (tools/kernel_regs.py). The kernels of the two predefined programs keep all operands in registers,
also at nine limbs per element: private_segment_fixed_size == 0. The interpreter kernels are present, and their scratch size is
reported. Template arguments of k_execute_predef: the field's parameters, the program (0 = A B - C, 1 = E (A B - C)) and the elements
per load (1, or 4 for the one-word fields)."""
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "icicle_amd", "lib", "libicicle_hip.so")

SMALL, BIG = ("babybear_params", "koalabear_params"), ("bn254_fr_params", "bls12_381_fr_params")
PREDEF = [f"k_execute_predef<{f}, {g}, {v}>" for f in SMALL for g in (0, 1) for v in (1, 4)] + [f"k_execute_predef<{f}, {g}, 1>" for f in BIG for g in (0, 1)]
INTERP = [f"k_execute_program<{f}>" for f in SMALL + BIG]


def test_kernels_are_present_and_the_predefined_ones_do_not_use_scratch(tmp_path):
    assert os.path.exists(LIB), "library not built"
    spec = importlib.util.spec_from_file_location("kernel_regs", os.path.join(ROOT, "tools", "kernel_regs.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    rows = [k for co in kr.code_objects(LIB, str(tmp_path)) for k in kr.kernels(co)]
    dm = kr.demangle([r["name"] for r in rows])
    seen, bad = set(), []
    for r in rows:
        name = re.sub(r"\(.*", "", dm[r["name"]]).replace("icicle_hip::", "").replace("void ", "")
        scratch = int(r.get("private_segment_fixed_size", 0))
        if name in PREDEF:
            seen.add(name)
            if scratch != 0:
                bad.append(f"{name}: {scratch} B of scratch per lane, {r.get('vgpr_count')} VGPRs")
        elif name in INTERP:
            seen.add(name)
            print(f"{name}: {scratch} B of scratch per lane, {r.get('vgpr_count')} VGPRs, {r.get('group_segment_fixed_size')} B of LDS")
    assert not bad, "\n".join(bad)
    assert seen == set(PREDEF + INTERP), f"kernels not found in the library: {sorted(set(PREDEF + INTERP) - seen)}"
