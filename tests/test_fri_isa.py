"""ISA lint (CPU only), the method of tests/test_pow_isa.py: every instantiation of the FRI fold kernel is in the library and keeps
its operands in registers -- two elements, the twiddle, alpha and alpha * W, at most 4 + 4 + 9 words of constants --:
private_segment_fixed_size == 0 in the gfx950 code objects embedded in libicicle_hip.so (tools/kernel_regs.py). Template arguments:
the field's parameters, the words of an element (1 scalar, 4 quartic extension), and whether a lane moves 16 bytes per access."""
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "icicle_amd", "lib", "libicicle_hip.so")

KERNELS = [f"k_fri_fold<{f}_params, {w}, {v}>" for f in ("babybear", "koalabear") for w in (1, 4) for v in ("true", "false")]


def test_fold_kernels_are_present_and_do_not_use_scratch(tmp_path):
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
