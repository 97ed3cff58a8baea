"""ISA lint (CPU only), the method of tests/test_poseidon2_isa.py: every instantiation of the two Poseidon kernels -- 15 (field, t)
pairs, batch and padded-leaf -- is in the library, and at widths 3 and 5 the state stays in registers: private_segment_fixed_size == 0
in the gfx950 code objects embedded in libicicle_hip.so (tools/kernel_regs.py). No kernel declares LDS. Widths 9 and 12 must be
present; their registers and scratch size are printed (profiles/poseidon_notes.md records them), not asserted."""
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "icicle_amd", "lib", "libicicle_hip.so")

# the parameter sets of the scalar fields: BN254, BLS12-381 (no t = 3), BLS12-377, Grumpkin (BN254's base field)
PAIRS = [(f, t) for f in ("bn254_fr_params", "bls12_381_fr_params", "bls12_377_fr_params", "bn254_fq_params") for t in (3, 5, 9, 12)
         if (f, t) != ("bls12_381_fr_params", 3)]
KERNELS = {f"{k}<{f}, {t}>": t for k in ("k_poseidon_batch", "k_poseidon_leaves") for f, t in PAIRS}


def test_poseidon_kernels_are_present_and_the_narrow_ones_keep_the_state_in_registers(tmp_path):
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
            scratch, lds = int(r.get("private_segment_fixed_size", 0)), int(r.get("group_segment_fixed_size", 0))
            print(f"{name}: {r.get('vgpr_count')} VGPRs, {r.get('agpr_count')} AGPRs, {r.get('sgpr_count')} SGPRs, {scratch} B of scratch per lane, {lds} B of LDS")
            if scratch != 0 and KERNELS[name] <= 5:
                bad.append(f"{name}: {scratch} B of scratch per lane, {r.get('vgpr_count')} VGPRs")
            if lds != 0:
                bad.append(f"{name}: {lds} B of LDS, none declared")
    assert not bad, "\n".join(bad)
    assert len(KERNELS) == 30 and seen == set(KERNELS), f"kernels not found in the library: {sorted(set(KERNELS) - seen)}"
