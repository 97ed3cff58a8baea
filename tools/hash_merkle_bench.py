#!/usr/bin/env python3
"""Times the device hashers and the Merkle build (profiles/hash_merkle_notes.md): Keccak-256 over 2^k messages of 64 bytes, device to
device, and a binary Keccak-256 tree over 32-byte leaves with the fused top and with one launch per layer.
usage: tools/hash_merkle_bench.py [--log-batch 22] [--log-leaves 22 10] [--top-max 0 256 1024] [--reps 5]"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def best(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return min(ts) * 1e3, sorted(ts)[len(ts) // 2] * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-batch", type=int, default=22)
    ap.add_argument("--log-leaves", type=int, nargs="*", default=[22, 10])
    ap.add_argument("--top-max", type=int, nargs="*", default=[0, 1024])
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import icicle_amd
    from icicle_amd import runtime
    from icicle_amd._lib import lib
    from icicle_amd.hash import Hasher
    from icicle_amd.merkle import MerkleTree
    from icicle_amd.runtime import DeviceVec

    runtime.set_device(0)
    rng = np.random.default_rng(1)
    n = 1 << a.log_batch
    d_in = DeviceVec.from_host(rng.integers(0, 256, 64 * n, dtype=np.uint8))
    d_out = DeviceVec(32 * n)
    h = Hasher.keccak256(64)
    lo, med = best(lambda: h.hash(d_in, size=64, batch=n, out=d_out), a.reps)
    print(f"keccak256 batch 2^{a.log_batch} x 64 B device->device: best {lo:.3f} ms, median {med:.3f} ms, {n / lo * 1e3:.3e} hashes/s")
    for logl in a.log_leaves:
        leaves = 1 << logl
        L = logl  # 32-byte leaves, two per 64-byte layer-0 input: 2^(logl-1) hashes at the bottom, logl layers
        d_leaves = d_in if 32 * leaves <= d_in.nbytes else DeviceVec.from_host(rng.integers(0, 256, 32 * leaves, dtype=np.uint8))
        for top in a.top_max:
            ext = lib.create_config_extension()
            lib.config_extension_set_int(ext, b"hip_merkle_top_max_hashes", top)
            cfg = icicle_amd.MerkleTreeConfig.default()
            cfg.is_tree_on_device = True
            cfg.ext = ext

            def build():
                t = MerkleTree([h] * L, 32)
                t.build(d_leaves, size=32 * leaves, cfg=cfg)
                t.close()

            lo, med = best(build, a.reps)
            print(f"merkle build 2^{logl} x 32 B leaves, {L} layers, hip_merkle_top_max_hashes={top}: best {lo:.3f} ms, median {med:.3f} ms")
            lib.destroy_config_extension(ext)


if __name__ == "__main__":
    main()
