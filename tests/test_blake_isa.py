"""ISA lint (CPU only), the method of tests/test_hash_isa.py: the Blake kernels keep h[8], m[16] and v[16] in registers. An array that
is indexed by anything but a compile-time constant -- a message schedule looked up at run time, a per-lane stack of chaining values
-- ends up in scratch memory (private_segment_fixed_size > 0); this reads the figures of the gfx950 code objects embedded in
libicicle_hip.so (tools/kernel_regs.py). The fused top kernel, which now carries the Blake paths too, is a 1024-thread block: at most
128 VGPRs."""
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "icicle_amd", "lib", "libicicle_hip.so")

# (regex on the demangled kernel name, kernels that must match at least); 1 = Blake2s, 2 = Blake3
RULES = [
    (r"^k_blake_batch<1, (true|false)>", 2),
    (r"^k_blake_batch<2, (true|false)>", 2),
    (r"^k_blake_leaves<(1|2)>", 2),
    (r"^k_blake3_chunks<(true|false)>", 2),
    (r"^k_blake3_leaf_chunks$", 1),
    (r"^k_blake3_parents$", 1),
    (r"^k_merkle_top$", 1),
]


def test_blake_kernels_do_not_use_scratch(tmp_path):
    assert os.path.exists(LIB), "library not built"
    spec = importlib.util.spec_from_file_location("kernel_regs", os.path.join(ROOT, "tools", "kernel_regs.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    rows = [k for co in kr.code_objects(LIB, str(tmp_path)) for k in kr.kernels(co)]
    dm = kr.demangle([r["name"] for r in rows])
    seen = [0] * len(RULES)
    bad = []
    for r in rows:
        name = re.sub(r"\(.*", "", dm[r["name"]]).replace("icicle_hip::", "").replace("void ", "")
        for i, (pat, _) in enumerate(RULES):
            if re.search(pat, name):
                seen[i] += 1
                scratch = int(r.get("private_segment_fixed_size", 0))
                if scratch != 0:
                    bad.append(f"{name}: {scratch} B of scratch per lane, {r.get('vgpr_count')} VGPRs")
                if name == "k_merkle_top" and int(r.get("vgpr_count", 0)) + int(r.get("agpr_count", 0)) > 128:
                    bad.append(f"{name}: {r.get('vgpr_count')} VGPRs + {r.get('agpr_count')} AGPRs in a 1024-thread block")
    assert not bad, "\n".join(bad)
    missing = [RULES[i][0] for i, (_, n) in enumerate(RULES) if seen[i] < n]
    assert not missing, f"kernels not found in the library: {missing}"
