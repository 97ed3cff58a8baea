"""ISA lint (CPU only): the hash kernels keep the 25-lane Keccak state in registers. A state array that is indexed by anything but a
compile-time constant ends up in scratch memory (private_segment_fixed_size > 0) and every round then pays for it; this reads the
register / scratch figures of the gfx950 code objects embedded in libicicle_hip.so (tools/kernel_regs.py)."""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "icicle_amd", "lib", "libicicle_hip.so")

# (regex on the demangled kernel name, kernels that must match at least)
RULES = [
    (r"^k_keccak_batch<17, 4, (true|false)>", 2),
    (r"^k_keccak_batch<9, 8, (true|false)>", 2),
    (r"^k_keccak_leaves<(17, 4|9, 8)>", 2),
    (r"^k_merkle_top$", 1),
]


def test_hash_kernels_do_not_use_scratch(tmp_path):
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
    assert not bad, "\n".join(bad)
    missing = [RULES[i][0] for i, (_, n) in enumerate(RULES) if seen[i] < n]
    assert not missing, f"kernels not found in the library: {missing}"
