#!/usr/bin/env python3
"""Launch sequence of the MSM over the shapes that take different routes, for a kernel trace:

  rocprofv3 --kernel-trace --output-format json -d DIR -o msm -- python tools/msm_launch_trace.py run
  python tools/msm_launch_trace.py list DIR/.../msm_results.json > launches.txt

`run` does one call each of: BN254 single MSMs at 2^10, 2^16, 2^20 and 2^22; one batch of 128 x 2^12; one precompute_factor = 2
call at 2^14; one forced 12-window mixed plan at 5000 terms; BLS12-381 at 2^16; BN254 G2 at 2^12 -- inputs resident on the
device, results to the host. `list` prints kernel name, grid, block and LDS bytes (the dispatch's group segment: static and
dynamic; the CSV trace's LDS column leaves the dynamic part out) of every dispatch in start order; the base
generator (k_generate) runs before every case and so separates the cases. Two builds of the library (ICICLE_HIP_LIB) that
launch the same kernels the same way give identical lists."""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run():
    import numpy as np
    import torch
    from icicle_amd import msm as M, runtime
    from icicle_amd._lib import MSMConfig, lib

    runtime.set_device(0)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(9)

    def case(curve, n, batch=1, g2=False, pf=1, windows=0):
        L = M.LIMBS[curve] * (2 if g2 else 1)
        bases = torch.empty((n, 2 * L), dtype=torch.int32, device=dev)
        M.generate_affine_points(curve, n, k0=1, out=bases.data_ptr(), g2=g2)
        sc = torch.randint(-(2 ** 31), 2 ** 31, (n * batch, 8), dtype=torch.int32, device=dev, generator=gen)
        sc[:, 7] = torch.randint(0, 0x30644E72, (n * batch,), dtype=torch.int32, device=dev, generator=gen)  # below every curve's r
        cfg = MSMConfig.default()
        cfg.batch_size = batch
        cfg.are_points_shared_in_batch = True
        ext = None
        if pf > 1:
            cfg.precompute_factor = pf
            table = torch.empty((n * pf, 2 * L), dtype=torch.int32, device=dev)
            M.precompute_bases(curve, bases.data_ptr(), cfg, output=table.data_ptr(), nof_bases=n, g2=g2)
            bases = table
        if windows:
            ext = lib.create_config_extension()
            lib.config_extension_set_int(ext, b"hip_msm_windows", windows)
            cfg.ext = ext
        out = np.zeros((batch, 3 * L), dtype=np.uint32)
        M.msm(curve, sc.data_ptr(), bases.data_ptr(), cfg, results=out, msm_size=n, g2=g2)
        torch.cuda.synchronize()
        if ext:
            lib.destroy_config_extension(ext)
        print(curve, "g2" if g2 else "g1", n, batch, pf, windows, "%08x" % int(out.view(np.uint32).sum() & 0xFFFFFFFF), flush=True)

    for logn in (10, 16, 20, 22):
        case("bn254", 1 << logn)
    case("bn254", 1 << 12, batch=128)
    case("bn254", 1 << 14, pf=2)
    case("bn254", 5000, windows=12)
    case("bls12_381", 1 << 16)
    case("bn254", 1 << 12, g2=True)


def listing(path):
    tool = json.load(open(path))["rocprofiler-sdk-tool"][0]
    names = {k["kernel_id"]: k.get("formatted_kernel_name") or k["kernel_name"] for k in tool["kernel_symbols"]}
    for r in sorted(tool["buffer_records"]["kernel_dispatch"], key=lambda r: r["start_timestamp"]):
        d = r["dispatch_info"]
        name = names[d["kernel_id"]]
        if "icicle_hip" not in name:
            continue  # (the tensor library's fill / random kernels)
        short = re.sub(r"^void\s+", "", re.sub(r"\(.*", "", name))
        print(short, "grid", *[d["grid_size"][a] for a in "xyz"], "block", *[d["workgroup_size"][a] for a in "xyz"], "lds", d["group_segment_size"])


if __name__ == "__main__":
    run() if sys.argv[1] == "run" else listing(sys.argv[2])
