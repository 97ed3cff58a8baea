"""ISA lint (CPU only), the method of tests/test_poseidon2_isa.py: every instantiation of the two Poseidon2 kernels over Goldilocks
-- 8 widths, batch and padded-leaf -- is in the library, and up to width 16 the state stays in registers:
private_segment_fixed_size == 0 in the gfx950 code objects embedded in libicicle_hip.so (tools/kernel_regs.py). Widths 20 and 24
must be present; their scratch size is printed (profiles/poseidon2_notes.md records it), not asserted. Metadata only: no
instruction text is read."""
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "icicle_amd", "lib", "libicicle_hip.so")

WIDTHS = (2, 3, 4, 8, 12, 16, 20, 24)
KERNELS = {f"{k}<{t}>": t for k in ("k_poseidon2_gold_batch", "k_poseidon2_gold_leaves") for t in WIDTHS}


def test_poseidon2_gold_kernels_are_present_and_keep_the_state_in_registers(tmp_path):
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
            print(f"{name}: {r.get('vgpr_count')} VGPRs, {r.get('sgpr_count')} SGPRs, {scratch} B of scratch per lane")
            if scratch != 0 and KERNELS[name] <= 16:
                bad.append(f"{name}: {scratch} B of scratch per lane, {r.get('vgpr_count')} VGPRs")
    assert not bad, "\n".join(bad)
    assert len(KERNELS) == 16 and seen == set(KERNELS), f"kernels not found in the library: {sorted(set(KERNELS) - seen)}"
