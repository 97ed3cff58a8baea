"""ISA lint (CPU only), the method of tests/test_sumcheck_isa.py: every instantiation of the shared-inversion kernel and of the
reduction kernel is in the library and keeps its tile in registers -- the running products of a lane, and its elements where they are
one or two words --: private_segment_fixed_size == 0 in the gfx950 code objects embedded in libicicle_hip.so (tools/kernel_regs.py).
Template arguments: the element type of the field, then DIV (false = vector_inv, true = vector_div) or the operation (0 = sum,
1 = product)."""
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "icicle_amd", "lib", "libicicle_hip.so")

ELEMENTS = ("SmallElem<babybear_params>", "SmallElem<koalabear_params>", "GoldElem", "BigElem<bn254_fr_params>", "BigElem<bls12_381_fr_params>",
            "BigElem<bls12_377_fr_params>", "BigElem<stark252_fr_params>", "BigElem<bn254_fq_params>")  # the last one: grumpkin
KERNELS = [f"k_vec_inv<{e}, {d}>" for e in ELEMENTS for d in ("false", "true")] + [f"k_vec_reduce<{e}, {op}>" for e in ELEMENTS for op in (0, 1)]


def test_inversion_and_reduction_kernels_are_present_and_do_not_use_scratch(tmp_path):
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
    assert len(KERNELS) == 32 and seen == set(KERNELS), f"kernels not found in the library: {sorted(set(KERNELS) - seen)}"
