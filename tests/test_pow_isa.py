"""ISA lint (CPU only), the method of tests/test_blake_isa.py: every instantiation of the proof-of-work kernels is in the library and
keeps its hash state in registers -- the 25-lane Keccak state, h[8] / m[16] / v[16] of the Blake hashes -- with the message reader
(ReadPow) under the same absorb code as the batch kernels: private_segment_fixed_size == 0 in the gfx950 code objects embedded in
libicicle_hip.so (tools/kernel_regs.py). Template arguments: the hash kind (0 Keccak, 1 Blake2s, 2 Blake3), then Keccak's rate in
words (17: 256-bit digests, 9: 512-bit ones)."""
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "icicle_amd", "lib", "libicicle_hip.so")

INSTANCES = ["<0, 17>", "<0, 9>", "<1, 0>", "<2, 0>"]
KERNELS = [f"{k}{i}" for k in ("k_pow_search", "k_pow_eval") for i in INSTANCES]


def test_pow_kernels_are_present_and_do_not_use_scratch(tmp_path):
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
