"""ISA lint (CPU only), the method of tests/test_fri_isa.py: every instantiation of the sumcheck round kernel for a predefined program
is in the library and keeps its operands in registers -- d + 1 <= 4 running sums, 3 or 4 inputs and their differences, also at nine
limbs per element --: private_segment_fixed_size == 0 in the gfx950 code objects embedded in libicicle_hip.so (tools/kernel_regs.py).
Template arguments: the field's parameters, the program (0 = A B - C, 1 = E (A B - C)) and the entry shape (0 = round 0, no fold;
1 = fold and write the folded pair; 2 = fold, nothing written: the last round)."""
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "icicle_amd", "lib", "libicicle_hip.so")

FIELD_PARAMS = ("babybear_params", "koalabear_params", "bn254_fr_params", "bls12_381_fr_params")
KERNELS = [f"k_sumcheck_round<{f}, {g}, {s}>" for f in FIELD_PARAMS for g in (0, 1) for s in (0, 1, 2)]


def test_round_kernels_are_present_and_do_not_use_scratch(tmp_path):
    assert os.path.exists(LIB), "library not built"
    spec = importlib.util.spec_from_file_location("kernel_regs", os.path.join(ROOT, "tools", "kernel_regs.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    rows = [k for co in kr.code_objects(LIB, str(tmp_path)) for k in kr.kernels(co)]
    dm = kr.demangle([r["name"] for r in rows])
    seen, bad = set(), []
    for r in rows:
        name = re.sub(r"\(.*", "", dm[r["name"]]).replace("icicle_hip::", "").replace("void ", "")
        if name in KERNELS:
            seen.add(name)
            scratch = int(r.get("private_segment_fixed_size", 0))
            if scratch != 0:
                bad.append(f"{name}: {scratch} B of scratch per lane, {r.get('vgpr_count')} VGPRs")
    assert not bad, "\n".join(bad)
    assert seen == set(KERNELS), f"kernels not found in the library: {sorted(set(KERNELS) - seen)}"
