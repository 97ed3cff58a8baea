"""ISA lint (CPU only), the method of tests/test_vecops_inv_isa.py: every instantiation of the extension vector kernels is in the
library and uses no scratch: private_segment_fixed_size == 0 in the gfx950 code objects embedded in libicicle_hip.so
(tools/kernel_regs.py). The VGPR counts are printed (pytest -s), not asserted. Template arguments: the extension element type, then VEC
(true = 16-byte accesses, false = word by word), for k_ext_inv DIV before it; the shared reduction is instantiated with the element
type and with its 16-byte form Vec16<>, operation 0 = sum, 1 = product; extension_bit_reverse is k_bitrev_elems<4>."""
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "icicle_amd", "lib", "libicicle_hip.so")

ELEMENTS = ("SmallExtElem<babybear_params>", "SmallExtElem<koalabear_params>", "GoldExtElem")
B = ("false", "true")
KERNELS = ([f"k_ext_vec2<{e}, {v}>" for e in ELEMENTS for v in B] + [f"k_ext_mixed_mul<{e}, {v}>" for e in ELEMENTS for v in B]
           + [f"k_ext_inv<{e}, {d}, {v}>" for e in ELEMENTS for d in B for v in B]
           + [f"{k}<{el}, {op}>" for k in ("k_vec_reduce", "k_vec_reduce_finish") for e in ELEMENTS for el in (e, f"Vec16<{e}>") for op in (0, 1)]
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
        name = re.sub(r"\(.*", "", dm[r["name"]]).replace("icicle_hip::", "").replace("void ", "").replace("> >", ">>")
        if name in KERNELS:
            seen.add(name)
            scratch = int(r.get("private_segment_fixed_size", 0))
            print(f"{name}: {r.get('vgpr_count')} VGPRs, {r.get('sgpr_count')} SGPRs, {scratch} B scratch")
            if scratch != 0:
                bad.append(f"{name}: {scratch} B of scratch per lane, {r.get('vgpr_count')} VGPRs")
    assert not bad, "\n".join(bad)
    assert len(KERNELS) == 49 and seen == set(KERNELS), f"kernels not found in the library: {sorted(set(KERNELS) - seen)}"
