#!/usr/bin/env python3
"""Times the device hashers and the Merkle build (profiles/hash_merkle_notes.md): one hasher (Keccak-256, Blake2s or Blake3) over 2^k
messages of 64 bytes, device to device, and a binary tree of that hasher over 32-byte leaves with the fused top and with one launch
per layer. Several hashers (--hash keccak256 blake3) are timed in interleaved rounds of one process, so their ratio is a property of
the kernels and not of two runs. Every output line begins with its hasher's name; a run without --hash times Keccak-256 alone, as
the tool did before it knew other hashers.
--pow times the proof-of-work solver instead: a search over 2^26 nonces that cannot succeed (60 bits, hip_pow_count_log2 = 26) beside the
batch hash of 2^22 x 64 B in the same interleaved rounds, both as time per hash, and whole solves of the challenge bytes(range(32))
at --pow-bits by nonces per launch (--pow-span-log2).
usage: tools/hash_merkle_bench.py [--hash keccak256 [blake2s blake3]] [--log-batch 22] [--log-leaves 22 10] [--top-max 0 256 1024] [--reps 5]
       tools/hash_merkle_bench.py --pow [--hash keccak256 blake2s blake3] [--reps 9] [--pow-bits 20 25 30] [--pow-span-log2 24 28 32]"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def best_interleaved(fns, reps):
    """(best ms, median ms) of each callable after a warm-up call, one call of each per round"""
    for fn in fns:
        fn()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            t = time.perf_counter()
            fn()
            ts[i].append(time.perf_counter() - t)
    return [(min(t) * 1e3, sorted(t)[len(t) // 2] * 1e3) for t in ts]


def all_interleaved(fns, reps):
    """every timing in ms of each callable after a warm-up call, one call of each per round"""
    for fn in fns:
        fn()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            t = time.perf_counter()
            fn()
            ts[i].append((time.perf_counter() - t) * 1e3)
    return [sorted(t) for t in ts]


def pow_bench(a):
    """The solver does the batch kernel's hashing without its loads and its digest store, so its time per hash must not exceed the
    batch kernel's: medians of one run compared, the run's own spread (fastest and slowest repetition) printed beside them."""
    import icicle_amd
    from icicle_amd import PowConfig, runtime
    from icicle_amd._lib import lib
    from icicle_amd.hash import Hasher
    from icicle_amd.runtime import DeviceVec

    runtime.set_device(0)
    rng = np.random.default_rng(1)
    log_search, log_batch = 26, 22
    n = 1 << log_batch
    d_in = DeviceVec.from_host(rng.integers(0, 256, 64 * n, dtype=np.uint8))
    d_out = DeviceVec(32 * n)
    challenge = np.arange(32, dtype=np.uint8)
    d_challenge = DeviceVec.from_host(challenge)

    def cfg_with(**keys):
        ext = lib.create_config_extension()
        for k, v in keys.items():
            lib.config_extension_set_int(ext, k.encode(), v)
        cfg = PowConfig.default()
        cfg.ext = ext  # lives as long as the process
        return cfg

    hashers = [getattr(Hasher, name)(64) for name in a.hash]
    # the search as a caller gets it (default nonces per launch), and the kernel alone (the 2^26 nonces in one launch)
    fruitless = {"default spans": cfg_with(hip_pow_count_log2=log_search), "one launch": cfg_with(hip_pow_count_log2=log_search, hip_pow_span_log2=log_search)}

    def search(h, cfg):
        assert icicle_amd.pow_solve(h, d_challenge, 60, cfg)[0] is False

    fns = [f for h in hashers for f in [lambda h=h, c=c: search(h, c) for c in fruitless.values()] + [lambda h=h: h.hash(d_in, size=64, batch=n, out=d_out)]]
    ts = all_interleaved(fns, a.reps)
    print(f"time per hash, ps: solver over 2^{log_search} nonces | batch 2^{log_batch} x 64 B device->device; median (min .. max) of {a.reps}")
    k = len(fruitless) + 1
    for i, name in enumerate(a.hash):
        b = [t * 1e9 / n for t in ts[k * i + k - 1]]
        mb = b[len(b) // 2]
        print(f"{name} batch {mb:.2f} ({b[0]:.2f} .. {b[-1]:.2f}), {1e3 / mb:.2f} G hashes/s, whole call {ts[k * i + k - 1][len(b) // 2]:.3f} ms")
        for j, label in enumerate(fruitless):
            s = [t * 1e9 / (1 << log_search) for t in ts[k * i + j]]
            ms = s[len(s) // 2]
            print(f"{name} pow, {label}: {ms:.2f} ({s[0]:.2f} .. {s[-1]:.2f}), {1e3 / ms:.2f} G hashes/s, whole call {ts[k * i + j][len(s) // 2]:.3f} ms: "
                  f"solver {'<=' if ms <= mb else '>'} batch (medians)")
    for bits in a.pow_bits:
        for name, h in zip(a.hash, hashers):
            row = []
            for span in a.pow_span_log2:
                cfg = cfg_with(hip_pow_span_log2=span)
                got = []
                t = all_interleaved([lambda: got.append(icicle_amd.pow_solve(h, d_challenge, bits, cfg))], a.reps)[0]
                assert got[0][0] and all(g == got[0] for g in got)
                row.append(f"2^{span}: {t[len(t) // 2]:.3f} ms ({t[0]:.3f} .. {t[-1]:.3f})")
            print(f"{name} solve {bits} bits, nonce {got[0][1]}: " + " | ".join(row))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pow", action="store_true")
    ap.add_argument("--pow-bits", type=int, nargs="*", default=[20, 25, 30])
    ap.add_argument("--pow-span-log2", type=int, nargs="*", default=[24, 28, 32])
    ap.add_argument("--hash", choices=["keccak256", "blake2s", "blake3"], nargs="+", default=["keccak256"])
    ap.add_argument("--log-batch", type=int, default=22)
    ap.add_argument("--log-leaves", type=int, nargs="*", default=[22, 10])
    ap.add_argument("--top-max", type=int, nargs="*", default=[0, 1024])
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if a.pow:
        return pow_bench(a)
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
    hashers = [getattr(Hasher, name)(64) for name in a.hash]
    timed = best_interleaved([lambda h=h: h.hash(d_in, size=64, batch=n, out=d_out) for h in hashers], a.reps)
    for name, (lo, med) in zip(a.hash, timed):
        print(f"{name} batch 2^{a.log_batch} x 64 B device->device: best {lo:.3f} ms, median {med:.3f} ms, {n / lo * 1e3:.3e} hashes/s"
              + (f", {timed[0][1] / med:.2f}x {a.hash[0]} (medians)" if name != a.hash[0] else ""))
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

            def build(h):
                t = MerkleTree([h] * L, 32)
                t.build(d_leaves, size=32 * leaves, cfg=cfg)
                t.close()

            timed = best_interleaved([lambda h=h: build(h) for h in hashers], a.reps)
            for name, (lo, med) in zip(a.hash, timed):
                print(f"{name} merkle build 2^{logl} x 32 B leaves, {L} layers, hip_merkle_top_max_hashes={top}: best {lo:.3f} ms, median {med:.3f} ms")
            lib.destroy_config_extension(ext)


if __name__ == "__main__":
    main()
