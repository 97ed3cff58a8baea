"""ISA lint (CPU only), the method of tests/test_poseidon2_isa.py: every instantiation of the two Poseidon2 kernels over the 256-bit
fields -- 5 fields x 4 widths, batch and padded-leaf -- is in the library, and the state stays in registers at every width:
private_segment_fixed_size == 0 in the gfx950 code objects embedded in libicicle_hip.so (tools/kernel_regs.py). The register
counts are printed (profiles/poseidon2_notes.md records them)."""
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "icicle_amd", "lib", "libicicle_hip.so")

FIELDS = ("bn254_fr_params", "bls12_381_fr_params", "bls12_377_fr_params", "bn254_fq_params", "stark252_fr_params")
WIDTHS = (2, 3, 4, 8)
KERNELS = {f"{k}<{f}, {t}>" for k in ("k_poseidon2_wide_batch", "k_poseidon2_wide_leaves") for f in FIELDS for t in WIDTHS}


def test_wide_poseidon2_kernels_are_present_and_keep_the_state_in_registers(tmp_path):
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
            if scratch != 0:
                bad.append(f"{name}: {scratch} B of scratch per lane, {r.get('vgpr_count')} VGPRs")
    assert len(KERNELS) == 40 and seen == KERNELS, f"kernels not found in the library: {sorted(KERNELS - seen)}"
    assert not bad, "\n".join(bad)
