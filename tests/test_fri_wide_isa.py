"""ISA lint (CPU only), the method of tests/test_fri_isa.py: every instantiation of the wide FRI fold kernel is in the library and
keeps its operands in registers -- two elements, the twiddle and alpha as limbs of the field --: private_segment_fixed_size == 0 in
the gfx950 code objects embedded in libicicle_hip.so (tools/kernel_regs.py). Template arguments: the field's parameters, the
coefficients of an element (1 scalar, 2 Goldilocks' quadratic extension), and whether a lane moves 16 bytes per access."""
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "icicle_amd", "lib", "libicicle_hip.so")

KINDS = [("goldilocks_params", 1), ("goldilocks_params", 2), ("stark252_fr_params", 1), ("bn254_fr_params", 1), ("bls12_381_fr_params", 1), ("bls12_377_fr_params", 1)]
KERNELS = [f"k_fri_fold_wide<{f}, {c}, {v}>" for f, c in KINDS for v in ("true", "false")]


def test_wide_fold_kernels_are_present_and_do_not_use_scratch(tmp_path):
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
