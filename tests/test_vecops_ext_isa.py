"""ISA lint (CPU only), the method of tests/test_vecops_inv_isa.py: every instantiation of the extension vector kernels is in the
library and uses no scratch: private_segment_fixed_size == 0 in the gfx950 code objects embedded in libicicle_hip.so
(tools/kernel_regs.py). The VGPR counts are printed (pytest -s), not asserted. Every kernel is instantiated with the extension element
type (word by word) and with its 16-byte form Vec16<>: the element-wise kernel k_vec2 and the inversion k_vec_inv (then DIV) that the
base fields use too, k_ext_mixed_mul, and the shared reduction (then the operation, 0 = sum, 1 = product); extension_bit_reverse is
k_bitrev_elems<4>."""
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "icicle_amd", "lib", "libicicle_hip.so")

ELEMENTS = ("SmallExtElem<babybear_params>", "SmallExtElem<koalabear_params>", "GoldExtElem")
B = ("false", "true")
ACCESS = [el for e in ELEMENTS for el in (e, f"Vec16<{e}>")]
KERNELS = ([f"k_vec2<{el}>" for el in ACCESS] + [f"k_ext_mixed_mul<{el}>" for el in ACCESS] + [f"k_vec_inv<{el}, {d}>" for el in ACCESS for d in B]
           + [f"{k}<{el}, {op}>" for k in ("k_vec_reduce", "k_vec_reduce_finish") for el in ACCESS for op in (0, 1)]
           + ["k_bitrev_elems<4>"])


def test_extension_kernels_are_present_and_do_not_use_scratch(tmp_path):
    assert os.path.exists(LIB), "library not built"
    spec = importlib.util.spec_from_file_location("kernel_regs", os.path.join(ROOT, "tools", "kernel_regs.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    rows = [k for co in kr.code_objects(LIB, str(tmp_path)) for k in kr.kernels(co)]
    dm = kr.demangle([r["name"] for r in rows])
    seen, bad = set(), []
    for r in rows:
        name = re.sub(r">\s+(?=>)", ">", re.sub(r"\(.*", "", dm[r["name"]]).replace("icicle_hip::", "").replace("void ", ""))
        if name in KERNELS:
            seen.add(name)
            scratch = int(r.get("private_segment_fixed_size", 0))
            print(f"{name}: {r.get('vgpr_count')} VGPRs, {r.get('sgpr_count')} SGPRs, {scratch} B scratch")
            if scratch != 0:
                bad.append(f"{name}: {scratch} B of scratch per lane, {r.get('vgpr_count')} VGPRs")
    assert not bad, "\n".join(bad)
    assert len(KERNELS) == 49 and seen == set(KERNELS), f"kernels not found in the library: {sorted(set(KERNELS) - seen)}"
