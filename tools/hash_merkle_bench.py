#!/usr/bin/env python3
"""Times the device hashers and the Merkle build (profiles/hash_merkle_notes.md): one hasher (Keccak-256, Blake2s or Blake3) over 2^k
messages of 64 bytes, device to device, and a binary tree of that hasher over 32-byte leaves with the fused top and with one launch
per layer. Several hashers (--hash keccak256 blake3) are timed in interleaved rounds of one process, so their ratio is a property of
the kernels and not of two runs. Every output line begins with its hasher's name; a run without --hash times Keccak-256 alone, as
the tool did before it knew other hashers.
--pow times the proof-of-work solver instead: a search over 2^26 nonces that cannot succeed (60 bits, hip_pow_count_log2 = 26) beside the
batch hash of 2^22 x 64 B in the same interleaved rounds, both as time per hash, and whole solves of the challenge bytes(range(32))
at --pow-bits by nonces per launch (--pow-span-log2).
--fri times the FRI prover (--field, default the BabyBear extension; Blake2s trees and transcript, default config: 16 proof-of-work
bits, 100 queries) at --fri-log-n sizes from a device input: the whole fri_merkle_tree_prove, and its stages run one by one through the public API on the
same layers -- the tree builds, the folds, the proof of work, the query phase as one batch of openings per round (MerkleTree.proofs) and,
beside it, the same openings as 2 x queries x rounds get_proof calls --, the whole fri_merkle_tree_verify of the proof, then the
first fold's bytes per second (n + n/2 elements and n/2 twiddles of the field's table) beside a device-to-device copy that moves the same byte count, in
interleaved rounds of the same run.
--openings times batched Merkle openings and verification against loops of single calls for the same indices (--open-counts, default
200 and 4000 random indices with repeats) on a Blake2s tree over 2^--open-log-leaves 16-byte leaves kept on the device: MerkleTree.proofs
beside a loop of MerkleTree.proof, MerkleTree.verify_batch beside a loop of MerkleTree.verify, in interleaved rounds.
--poseidon2 times Poseidon2 over BabyBear and KoalaBear (profiles/poseidon2_notes.md, which it writes with --notes): batches of 2^--log-batch
messages of one permutation at t = 16 and t = 24, device to device, beside a device-to-device copy of the same input bytes and Blake3
over the same input, in interleaved rounds; and the build of a binary tree (leaf layer: a t = 16 sponge over 8 elements, upper layers:
t = 2 compressions) beside a Blake3 tree over the same leaves. The registers and scratch of every kernel come from the library
(tools/kernel_regs.py).
--poseidon2 --p2-fields bn254 bls12_381 bls12_377 grumpkin stark252 times Poseidon2 over the 256-bit fields instead: per field batches of
2^--log-batch (at most 2^18) two-to-one hashes at t = 3 beside a domain tag and of one permutation at t = 4, device to device, and the
build of a binary tree of 2^--p2w-log-leaves leaves of 32 bytes with tagged t = 3 layers; in the same interleaved rounds Poseidon t = 3
beside the same tag over the same input and the same leaves (where Poseidon is built: not over BLS12-381 at t = 3, not over
stark252) and a device-to-device copy of the same input bytes. With --notes the lines go to that file as one code block.
--poseidon2 --p2-fields goldilocks times Poseidon2 over Goldilocks: per width (2, 3, 4, 8, 12, 16, 20, 24) batches of 2^--log-batch (at
most 2^20) messages of t elements, device to device; the build of a binary tree of 2^--p2-log-leaves leaves of 8 bytes (leaves t = 2
with input_size 1, nodes t = 2) and of a tree whose leaves are rows of 8 elements (leaves t = 12 with input_size 8, nodes t = 8 with
input_size 2); in the same interleaved rounds the Keccak-256 and the Blake3 tree over the same leaves -- what Goldilocks FRI commits
with otherwise -- and a device-to-device copy of the same bytes. With --notes the lines go to that file as one code block.
--poseidon times Poseidon over the scalar fields of BN254, BLS12-381, BLS12-377 and Grumpkin (profiles/poseidon_notes.md): batches of
2^--log-batch messages of one permutation per built (field, t), device to device, as hashes/s and as Montgomery products/s beside two
yardsticks of the same run -- the register-resident product rate behind icicle_hip_ubench_mixed_add and the plain 256-bit vector_mul;
and the build of a tree of about 2^--p1-log-leaves leaves with tagged t = 3 (t = 5 over BLS12-381) layers.
usage: tools/hash_merkle_bench.py [--hash keccak256 [blake2s blake3]] [--log-batch 22] [--log-leaves 22 10] [--top-max 0 256 1024] [--reps 5]
       tools/hash_merkle_bench.py --pow [--hash keccak256 blake2s blake3] [--reps 9] [--pow-bits 20 25 30] [--pow-span-log2 24 28 32]
       tools/hash_merkle_bench.py --fri [--field babybear_extension|goldilocks|goldilocks_extension|stark252|bn254|bls12_381|bls12_377]
                                        [--fri-log-n 20 24] [--reps 5]
       tools/hash_merkle_bench.py --openings [--open-log-leaves 20] [--open-counts 200 4000] [--reps 5]
       tools/hash_merkle_bench.py --poseidon2 [--log-batch 20] [--p2-log-leaves 18] [--reps 5] [--notes profiles/poseidon2_notes.md]
       tools/hash_merkle_bench.py --poseidon2 --p2-fields bn254 .. [--log-batch 18] [--p2w-log-leaves 14] [--reps 5] [--notes <file>]
       tools/hash_merkle_bench.py --poseidon2 --p2-fields goldilocks [--log-batch 20] [--p2-log-leaves 18] [--reps 5] [--notes <file>]
       tools/hash_merkle_bench.py --poseidon [--log-batch 18] [--p1-log-leaves 16] [--reps 5] [--notes <file>]"""
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


def fri_bench(a):
    import icicle_amd
    from icicle_amd import FriConfig, FriTranscriptConfig, MerkleTreeConfig, fri, ntt, runtime
    from icicle_amd._lib import lib, check
    from icicle_amd.hash import Hasher
    from icicle_amd.merkle import MerkleTree
    from icicle_amd.runtime import DeviceVec

    runtime.set_device(0)
    # prefix -> field, extension, words of an element, words of a twiddle, a bound below p for every 32-bit word of a random element
    kinds = {"babybear_extension": ("babybear", True, 4, 1, 0x78000001), "goldilocks": ("goldilocks", False, 2, 2, 0xFFFFFFFF),
             "goldilocks_extension": ("goldilocks", True, 4, 2, 0xFFFFFFFF), "stark252": ("stark252", False, 8, 8, 0x08000000),
             "bn254": ("bn254", False, 8, 8, 0x30644E72), "bls12_381": ("bls12_381", False, 8, 8, 0x73EDA753), "bls12_377": ("bls12_377", False, 8, 8, 0x12AB655E)}
    field, ext, words, tw_words, bound = kinds[a.field]
    eb = 4 * words
    rng = np.random.default_rng(1)
    th, lh, ch = Hasher.blake2s(), Hasher.blake2s(eb), Hasher.blake2s(64)
    tc = FriTranscriptConfig.new_default_labels(th, 1)
    med = lambda t: t[len(t) // 2]
    for logn in a.fri_log_n:
        n = 1 << logn
        ntt.release_domain(field)
        ntt.init_domain(field, ntt.get_root_of_unity(field, n))
        d_x = DeviceVec.from_host(rng.integers(0, bound, size=(n, words), dtype=np.uint32))  # every word below p's top word: canonical
        cfg = FriConfig.default()
        proofs = []
        total = all_interleaved([lambda: proofs.append(icicle_amd.fri_merkle_tree_prove(field, cfg, tc, d_x, lh, ch, 0, extension=ext))], a.reps)[0]
        assert all(pr.pow_nonce == proofs[0].pow_nonce for pr in proofs)
        rounds, queries = proofs[0].nof_rounds, cfg.nof_queries
        del proofs
        # the stages, one by one, on layers folded with a fixed challenge (the work does not depend on its value)
        d_alpha = DeviceVec.from_host(np.arange(5, 5 + words, dtype=np.uint32))
        layers = [d_x] + [DeviceVec(eb * (n >> r)) for r in range(1, rounds + 1)]

        def folds():
            for r in range(rounds):
                fri.fri_fold(field, layers[r], d_alpha, extension=ext, out=layers[r + 1])
            runtime.device_synchronize()

        mcfg = MerkleTreeConfig.default()
        mcfg.is_tree_on_device = True
        trees = []

        def builds():
            for t in trees:
                t.close()
            trees[:] = [MerkleTree([lh] + [ch] * (logn - r), eb).build(layers[r], cfg=mcfg) for r in range(rounds)]

        challenge = np.frombuffer(b"domain_separator_label" + logn.to_bytes(4, "little") + bytes(eb) + b"nonce_label", dtype=np.uint8).copy()
        picks = [int(q) for q in rng.integers(1, n + 1, queries)]

        def query_phase():
            for r in range(rounds):
                size = n >> r
                for pr in trees[r].proofs(layers[r], [i for q in picks for i in (q % size, (q + size // 2) % size)], False, mcfg):
                    pr.close()

        def query_phase_single_calls():
            for q in picks:
                for r in range(rounds):
                    size = n >> r
                    for idx in (q % size, (q + size // 2) % size):
                        trees[r].proof(layers[r], idx, False, mcfg).close()

        proof = icicle_amd.fri_merkle_tree_prove(field, cfg, tc, d_x, lh, ch, 0, extension=ext)

        def verify():
            assert icicle_amd.fri_merkle_tree_verify(field, cfg, tc, proof, lh, ch, extension=ext)

        folds()
        st = all_interleaved([builds, folds, lambda: icicle_amd.pow_solve(th, challenge, cfg.pow_bits), query_phase, query_phase_single_calls, verify], a.reps)
        print(f"fri prove {a.field} 2^{logn}, blake2s, {cfg.pow_bits} pow bits, {queries} queries, {rounds} rounds, device input: median {med(total):.3f} ms "
              f"({total[0]:.3f} .. {total[-1]:.3f}) of {a.reps}")
        for label, t in zip(("tree builds", "folds", "proof of work", f"query phase ({rounds} get_proofs calls of {2 * queries} openings)"), st):
            print(f"fri stage 2^{logn} {label}: median {med(t):.3f} ms ({t[0]:.3f} .. {t[-1]:.3f}), {100 * med(t) / med(total):.0f}% of the prove")
        print(f"fri 2^{logn} the same openings as {2 * queries * rounds} get_proof calls (not part of the prove): median {med(st[4]):.3f} ms ({st[4][0]:.3f} .. {st[4][-1]:.3f})")
        print(f"fri verify {a.field} 2^{logn}: median {med(st[5]):.3f} ms ({st[5][0]:.3f} .. {st[5][-1]:.3f}) of {a.reps}")
        # the first fold against a copy of the same byte count: n + n/2 elements and n/2 twiddles
        moved = eb * n + eb * n // 2 + 4 * tw_words * n // 2
        d_src, d_dst = DeviceVec(moved // 2), DeviceVec(moved // 2)

        def fold0():
            fri.fri_fold(field, layers[0], d_alpha, extension=ext, out=layers[1])
            runtime.device_synchronize()

        def copy():
            check(lib.icicle_copy(d_dst.ptr, d_src.ptr, moved // 2))
            runtime.device_synchronize()

        f, c = all_interleaved([fold0, copy], max(a.reps, 9))
        print(f"fri fold 2^{logn} -> 2^{logn - 1}: {moved / 2**20:.0f} MiB moved, median {med(f):.3f} ms ({f[0]:.3f} .. {f[-1]:.3f}) = {moved / med(f) / 1e9:.2f} TB/s | "
              f"device-to-device copy of the same bytes: median {med(c):.3f} ms ({c[0]:.3f} .. {c[-1]:.3f}) = {moved / med(c) / 1e9:.2f} TB/s | fold / copy {med(f) / med(c):.2f}")
        for t in trees:
            t.close()
        ntt.release_domain(field)


def openings_bench(a):
    from icicle_amd import MerkleTreeConfig, runtime
    from icicle_amd.hash import Hasher
    from icicle_amd.merkle import MerkleTree
    from icicle_amd.runtime import DeviceVec

    runtime.set_device(0)
    rng = np.random.default_rng(1)
    logl, eb = a.open_log_leaves, 16
    n = 1 << logl
    d_leaves = DeviceVec.from_host(rng.integers(0, 256, eb * n, dtype=np.uint8))
    cfg = MerkleTreeConfig.default()
    cfg.is_tree_on_device = True
    tree = MerkleTree([Hasher.blake2s(eb)] + [Hasher.blake2s(64)] * logl, eb).build(d_leaves, cfg=cfg)
    med = lambda t: t[len(t) // 2]
    for count in a.open_counts:
        indices = [int(v) for v in rng.integers(0, n, count)]
        for pruned in (False, True):
            proofs = tree.proofs(d_leaves, indices, pruned, cfg)
            assert tree.verify_batch(proofs) == [True] * count

            def batch():
                for pr in tree.proofs(d_leaves, indices, pruned, cfg):
                    pr.close()

            def singles():
                for i in indices:
                    tree.proof(d_leaves, i, pruned, cfg).close()

            def verify_singles():
                assert all(tree.verify(pr) for pr in proofs)

            ts = all_interleaved([batch, singles, lambda: tree.verify_batch(proofs), verify_singles], a.reps)
            kind = "pruned" if pruned else "full"
            for label, b, s in (("get_proofs", ts[0], ts[1]), ("verify_batch", ts[2], ts[3])):
                print(f"openings blake2s 2^{logl} x {eb} B leaves, {count} indices, {kind}: {label} median {med(b):.3f} ms ({b[0]:.3f} .. {b[-1]:.3f}) | "
                      f"{count} single calls median {med(s):.3f} ms ({s[0]:.3f} .. {s[-1]:.3f}) | single / batch {med(s) / med(b):.1f}")
    tree.close()


def poseidon2_kernel_rows():
    """name -> (VGPRs, SGPRs, scratch bytes per lane) of every Poseidon2 kernel in the library"""
    return kernel_rows(("k_poseidon2_batch<", "k_poseidon2_leaves<"))


def kernel_rows(prefix):
    """name -> (VGPRs, SGPRs, scratch bytes per lane) of every kernel in the library whose name begins with `prefix`"""
    import importlib.util
    import re
    import tempfile

    import icicle_amd
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("kernel_regs", os.path.join(root, "tools", "kernel_regs.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        rows = [k for co in kr.code_objects(icicle_amd.LIB_PATH, tmp) for k in kr.kernels(co)]
        dm = kr.demangle([r["name"] for r in rows])
        for r in rows:
            name = re.sub(r"\(.*", "", dm[r["name"]]).replace("icicle_hip::", "").replace("void ", "")
            if name.startswith(prefix):
                out[name] = (r.get("vgpr_count"), r.get("sgpr_count"), int(r.get("private_segment_fixed_size", 0)))
    return out


def poseidon2_products(t, r_f, r_p, sbox):
    """Montgomery products of one permutation as poseidon2_wide.hpp computes it: `sbox` per S-box (2, 3, 5 for x^3, x^5, x^11), t per
    full round, one per partial round; at t = 4, 8 one more per element in M_I"""
    return sbox * (t * r_f + r_p) + (t * r_p if t >= 4 else 0)


def poseidon2_wide_bench(a, fields):
    from icicle_amd import MerkleTreeConfig, runtime
    from icicle_amd._lib import lib, check
    from icicle_amd.hash import Hasher
    from icicle_amd.merkle import MerkleTree
    from icicle_amd.runtime import DeviceVec

    runtime.set_device(0)
    rng = np.random.default_rng(1)
    logb, logl = min(a.log_batch, 18), a.p2w_log_leaves
    n = 1 << logb
    med = lambda t: t[len(t) // 2]
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    # alpha's product count and the partial rounds at t = 3, 4 (tests/poseidon2_model_wide.py EXPECTED_ROUNDS)
    rounds = {"bn254": (3, 56, 56), "grumpkin": (3, 56, 56), "bls12_381": (3, 56, 56), "bls12_377": (5, 37, 37), "stark252": (2, 83, 84)}
    cfg = MerkleTreeConfig.default()
    cfg.is_tree_on_device = True
    for field in fields:
        sbox, rp3, rp4 = rounds[field]
        has_p1 = field in ("bn254", "bls12_377", "grumpkin")  # Poseidon t = 3 is built over these
        d_in = DeviceVec.from_host(rng.integers(0, 1 << 26, 8 * 4 * n, dtype=np.uint64).astype(np.uint32))  # canonical: below 2^250
        d_out, d_out1, d_copy = DeviceVec(32 * n), DeviceVec(32 * n), DeviceVec(32 * 4 * n)
        h3, h4 = Hasher.poseidon2(field, 3, domain_tag=0), Hasher.poseidon2(field, 4)
        p3 = Hasher.poseidon(field, 3, domain_tag=0) if has_p1 else None

        def copy(nbytes):
            check(lib.icicle_copy(d_copy.ptr, d_in.ptr, nbytes))
            runtime.device_synchronize()

        fns = [lambda: h3.hash(d_in, size=64, batch=n, out=d_out), lambda: copy(64 * n), lambda: h4.hash(d_in, size=128, batch=n, out=d_out), lambda: copy(128 * n)]
        if p3:
            fns.append(lambda: p3.hash(d_in, size=64, batch=n, out=d_out1))
        ts = all_interleaved(fns, a.reps)
        for t, size, hs, cp, rp in ((3, 64, ts[0], ts[1], rp3), (4, 128, ts[2], ts[3], rp4)):
            prods = poseidon2_products(t, 8, rp, sbox)
            say(f"poseidon2 {field} t={t} batch 2^{logb} x {size} B device->device: median {med(hs):.3f} ms ({hs[0]:.3f} .. {hs[-1]:.3f}), "
                f"{n / med(hs) * 1e3:.3e} hashes/s, {prods} products per permutation | copy of the same bytes {med(cp):.3f} ms, poseidon2 / copy {med(hs) / med(cp):.1f}")
        if p3:
            say(f"poseidon {field} t=3 over the same 2^{logb} x 64 B: median {med(ts[4]):.3f} ms ({ts[4][0]:.3f} .. {ts[4][-1]:.3f}), "
                f"{n / med(ts[4]) * 1e3:.3e} hashes/s | poseidon2 t=3 / poseidon t=3 {med(ts[0]) / med(ts[4]):.2f}")
        else:
            say(f"poseidon {field} t=3: not built, nothing to compare with")
        p2_layers = [h3] * logl
        p1_layers = [p3] * logl if p3 else None

        def build(layers):
            tree = MerkleTree(layers, 32)
            tree.build(d_in, size=32 << logl, cfg=cfg)
            tree.close()

        fns = [lambda: build(p2_layers)] + ([lambda: build(p1_layers)] if p3 else [])
        ts = all_interleaved(fns, a.reps)
        hashes = (1 << logl) - 1
        say(f"poseidon2 {field} merkle build 2^{logl} leaves x 32 B (t=3 with a tag, arity 2), {logl} layers, {hashes} hashes: median {med(ts[0]):.3f} ms "
            f"({ts[0][0]:.3f} .. {ts[0][-1]:.3f}), {hashes / med(ts[0]) * 1e3:.3e} hashes/s"
            + (f" | poseidon t=3 tree over the same leaves {med(ts[1]):.3f} ms, poseidon2 / poseidon {med(ts[0]) / med(ts[1]):.2f}" if p3 else ""))
        for v in (d_in, d_out, d_out1, d_copy):
            v.free()
        for h in (h3, h4, p3):
            if h:
                h.close()
    regs = kernel_rows("k_poseidon2_wide_")
    for name in sorted(regs, key=lambda k: (k.split("<")[0], k.split("<")[1].split(",")[0], int(k.split(", ")[1].rstrip(">")))):
        v, sg, scratch = regs[name]
        say(f"{name}: {v} VGPRs, {sg} SGPRs, {scratch} B of scratch per lane")
    if a.notes:
        with open(a.notes, "w") as f:
            f.write("```\n" + "\n".join(lines) + "\n```\n")


def poseidon2_gold_bench(a):
    from icicle_amd import MerkleTreeConfig, runtime
    from icicle_amd._lib import lib, check
    from icicle_amd.hash import Hasher
    from icicle_amd.merkle import MerkleTree
    from icicle_amd.runtime import DeviceVec

    runtime.set_device(0)
    rng = np.random.default_rng(1)
    logb, logl = min(a.log_batch, 20), a.p2_log_leaves
    n, p = 1 << logb, (1 << 64) - (1 << 32) + 1
    med = lambda t: t[len(t) // 2]
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    r_p = {2: 27, 3: 23, 4: 21}  # 22 from t = 8 on; R_F = 8 (tests/poseidon2_model_gold.py EXPECTED_ROUNDS)
    d_in = DeviceVec.from_host(rng.integers(0, p, 24 * n, dtype=np.uint64))
    d_out, d_copy = DeviceVec(8 * n), DeviceVec(8 * 24 * n)
    for t in (2, 3, 4, 8, 12, 16, 20, 24):
        h = Hasher.poseidon2_goldilocks(t)

        def copy():
            check(lib.icicle_copy(d_copy.ptr, d_in.ptr, 8 * t * n))
            runtime.device_synchronize()

        ts = all_interleaved([lambda: h.hash(d_in, size=8 * t, batch=n, out=d_out), copy], a.reps)
        prods = 4 * t * 8 + (4 + t) * r_p.get(t, 22)
        say(f"poseidon2 goldilocks t={t} batch 2^{logb} x {8 * t} B device->device: median {med(ts[0]):.3f} ms ({ts[0][0]:.3f} .. {ts[0][-1]:.3f}), "
            f"{n / med(ts[0]) * 1e3:.3e} hashes/s, {prods} products per permutation, {prods * n / med(ts[0]) * 1e3:.3e} products/s | "
            f"copy of the same bytes {med(ts[1]):.3f} ms, poseidon2 / copy {med(ts[0]) / med(ts[1]):.1f}")
        h.close()
    cfg = MerkleTreeConfig.default()
    cfg.is_tree_on_device = True
    trees = (("leaves of 8 B (t=2 with input_size 1, then t=2)", 1, [Hasher.poseidon2_goldilocks(2, input_size=1)] + [Hasher.poseidon2_goldilocks(2)] * logl),
             ("leaves of 8 elements (t=12 with input_size 8, then t=8 with input_size 2)", 8,
              [Hasher.poseidon2_goldilocks(12, input_size=8)] + [Hasher.poseidon2_goldilocks(8, input_size=2)] * logl))
    for what, elems, p2_layers in trees:
        nbytes = 8 * elems << logl
        k_layers = [Hasher.keccak256(8 * elems)] + [Hasher.keccak256(64)] * logl
        b3_layers = [Hasher.blake3(8 * elems)] + [Hasher.blake3(64)] * logl

        def build(layers):
            tree = MerkleTree(layers, 8)
            tree.build(d_in, size=nbytes, cfg=cfg)
            tree.close()

        def copy():
            check(lib.icicle_copy(d_copy.ptr, d_in.ptr, nbytes))
            runtime.device_synchronize()

        ts = all_interleaved([lambda: build(p2_layers), lambda: build(k_layers), lambda: build(b3_layers), copy], a.reps)
        hashes = (2 << logl) - 1
        say(f"poseidon2 goldilocks merkle build 2^{logl} {what}, {logl + 1} layers, {hashes} hashes: median {med(ts[0]):.3f} ms "
            f"({ts[0][0]:.3f} .. {ts[0][-1]:.3f}), {hashes / med(ts[0]) * 1e3:.3e} hashes/s | keccak256 tree over the same leaves {med(ts[1]):.3f} ms "
            f"({ts[1][0]:.3f} .. {ts[1][-1]:.3f}) | blake3 tree {med(ts[2]):.3f} ms ({ts[2][0]:.3f} .. {ts[2][-1]:.3f}) | copy of the leaves {med(ts[3]):.3f} ms "
            f"({ts[3][0]:.3f} .. {ts[3][-1]:.3f}) | poseidon2 / keccak256 {med(ts[0]) / med(ts[1]):.2f}, poseidon2 / blake3 {med(ts[0]) / med(ts[2]):.2f}")
        for h in set(p2_layers + k_layers + b3_layers):
            h.close()
    for v in (d_in, d_out, d_copy):
        v.free()
    regs = kernel_rows("k_poseidon2_gold_")
    for name in sorted(regs, key=lambda k: (k.split("<")[0], int(k.split("<")[1].rstrip(">")))):
        v, sg, scratch = regs[name]
        say(f"{name}: {v} VGPRs, {sg} SGPRs, {scratch} B of scratch per lane")
    if a.notes:
        with open(a.notes, "w") as f:
            f.write("```\n" + "\n".join(lines) + "\n```\n")


def poseidon2_bench(a):
    from icicle_amd._lib import POSEIDON2_GOLD_FIELDS, POSEIDON2_WIDE_FIELDS

    if any(f in POSEIDON2_GOLD_FIELDS for f in a.p2_fields):
        if len(a.p2_fields) != 1:
            sys.exit("--p2-fields: goldilocks is timed in a run of its own")
        return poseidon2_gold_bench(a)
    wide = [f for f in a.p2_fields if f in POSEIDON2_WIDE_FIELDS]
    if wide:
        if len(wide) != len(a.p2_fields):
            sys.exit("--p2-fields: the 31-bit and the 256-bit fields are timed in runs of their own")
        return poseidon2_wide_bench(a, wide)
    from icicle_amd import MerkleTreeConfig, runtime
    from icicle_amd._lib import lib, check
    from icicle_amd.hash import Hasher
    from icicle_amd.merkle import MerkleTree
    from icicle_amd.runtime import DeviceVec

    runtime.set_device(0)
    rng = np.random.default_rng(1)
    logb = min(a.log_batch, 20)
    n = 1 << logb
    med = lambda t: t[len(t) // 2]
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    primes = {"babybear": 0x78000001, "koalabear": 0x7F000001}
    for field, p in primes.items():
        if field not in a.p2_fields:
            continue
        for t in (16, 24):
            d_in = DeviceVec.from_host(rng.integers(0, p, t * n, dtype=np.uint64).astype(np.uint32))
            d_out, d_out32, d_copy = DeviceVec(4 * n), DeviceVec(32 * n), DeviceVec(4 * t * n)
            h, b3 = Hasher.poseidon2(field, t), Hasher.blake3(4 * t)

            def copy():
                check(lib.icicle_copy(d_copy.ptr, d_in.ptr, 4 * t * n))
                runtime.device_synchronize()

            ts = all_interleaved([lambda: h.hash(d_in, size=4 * t, batch=n, out=d_out), copy, lambda: b3.hash(d_in, size=4 * t, batch=n, out=d_out32)], a.reps)
            say(f"poseidon2 {field} t={t} batch 2^{logb} x {4 * t} B device->device: median {med(ts[0]):.3f} ms ({ts[0][0]:.3f} .. {ts[0][-1]:.3f}), "
                f"{n / med(ts[0]) * 1e3:.3e} hashes/s | copy of the same bytes {med(ts[1]):.3f} ms | blake3 {med(ts[2]):.3f} ms | "
                f"poseidon2 / copy {med(ts[0]) / med(ts[1]):.1f}, poseidon2 / blake3 {med(ts[0]) / med(ts[2]):.2f}")
            for v in (d_in, d_out, d_out32, d_copy):
                v.free()
            h.close(), b3.close()
        logl = a.p2_log_leaves
        d_leaves = DeviceVec.from_host(rng.integers(0, p, 8 << logl, dtype=np.uint64).astype(np.uint32))
        cfg = MerkleTreeConfig.default()
        cfg.is_tree_on_device = True
        p2_layers = [Hasher.poseidon2(field, 16, input_size=8)] + [Hasher.poseidon2(field, 2)] * logl
        b3_layers = [Hasher.blake3(32)] + [Hasher.blake3(64)] * logl

        def build(layers, es):
            tree = MerkleTree(layers, es)
            tree.build(d_leaves, cfg=cfg)
            tree.close()

        ts = all_interleaved([lambda: build(p2_layers, 4), lambda: build(b3_layers, 32)], a.reps)
        say(f"poseidon2 {field} merkle build 2^{logl} leaves x 32 B (t=16 sponge, then t=2), {logl + 1} layers: median {med(ts[0]):.3f} ms "
            f"({ts[0][0]:.3f} .. {ts[0][-1]:.3f}) | blake3 tree over the same leaves {med(ts[1]):.3f} ms | poseidon2 / blake3 {med(ts[0]) / med(ts[1]):.2f}")
        d_leaves.free()
    regs = poseidon2_kernel_rows()
    for name in sorted(regs, key=lambda k: (k.split("<")[0], "koala" in k, int(k.split(", ")[1].rstrip(">")))):
        v, sg, scratch = regs[name]
        say(f"{name}: {v} VGPRs, {sg} SGPRs, {scratch} B of scratch per lane")
    if a.notes:
        with open(a.notes, "w") as f:
            f.write("# Poseidon2 on the device: first measurement\n\n"
                    "Written by `tools/hash_merkle_bench.py --poseidon2 --notes <this file>` on one MI355X; wall-clock times of synchronous\n"
                    "calls with device operands, medians of interleaved rounds (lowest .. highest in brackets). No target was set for this\n"
                    "kernel: these figures are the starting point. One lane computes one hash, the state in registers, the round loop rolled\n"
                    "(`DESIGN.md` 9e).\n\n```\n" + "\n".join(lines) + "\n```\n")


def poseidon_products(t, r_p):
    """Montgomery products of one hash as poseidon.hpp computes it: t conversions in and one out, 7 full rounds of t (t + 3), r_p partial
    rounds of 3 + t + (t - 1), the last round of 3 t S-box products and one column of t"""
    return t + 1 + 7 * t * (t + 3) + r_p * (3 + 2 * t - 1) + 3 * t + t


def poseidon_bench(a):
    import ctypes

    from icicle_amd import MerkleTreeConfig, runtime, vecops
    from icicle_amd._lib import lib, check, POSEIDON_FIELDS
    from icicle_amd.hash import Hasher
    from icicle_amd.merkle import MerkleTree
    from icicle_amd.runtime import DeviceVec

    runtime.set_device(0)
    rng = np.random.default_rng(1)
    logb = min(a.log_batch, 18)
    n = 1 << logb
    med = lambda t: t[len(t) // 2]
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    # the yardsticks of the same build and run: the integer-ALU roof as field products per second (an XYZZ mixed addition over
    # BN254's 9-limb base field is 8 multiplications and 2 squarings, every operand in registers) and the plain 256-bit vector_mul
    adds = ctypes.c_double(0)
    check(lib.icicle_hip_ubench_mixed_add(0, ctypes.byref(adds)), "icicle_hip_ubench_mixed_add")
    roof = 10 * adds.value
    say(f"register-resident roof: {adds.value:.3e} bn254 mixed additions/s = {roof:.3e} 9-limb products/s")
    va, vb, vo = (DeviceVec.from_host(rng.integers(0, 1 << 28, 8 * n, dtype=np.uint64).astype(np.uint32)) for _ in range(3))
    ts = all_interleaved([lambda: vecops.vector_mul("bn254", va, vb, out=vo, size=n)], a.reps)
    say(f"vector_mul bn254 2^{logb} elements device->device: median {med(ts[0]):.3f} ms ({ts[0][0]:.3f} .. {ts[0][-1]:.3f}), {n / med(ts[0]) * 1e3:.3e} products/s")
    for v in (va, vb, vo):
        v.free()
    for field in POSEIDON_FIELDS:
        for t in (3, 5, 9, 12):
            if (field, t) == ("bls12_381", 3):
                continue
            d_in, d_out = DeviceVec.from_host(rng.integers(0, 1 << 28, 8 * t * n, dtype=np.uint64).astype(np.uint32)), DeviceVec(32 * n)
            h = Hasher.poseidon(field, t)
            ts = all_interleaved([lambda: h.hash(d_in, size=32 * t, batch=n, out=d_out)], a.reps)
            rate = n / med(ts[0]) * 1e3
            prods = poseidon_products(t, 56 if t < 9 else 57)
            say(f"poseidon {field} t={t} batch 2^{logb} x {32 * t} B device->device: median {med(ts[0]):.3f} ms ({ts[0][0]:.3f} .. {ts[0][-1]:.3f}), "
                f"{rate:.3e} hashes/s | {prods} products per hash, {rate * prods:.3e} products/s = {rate * prods / roof:.2f} of the roof")
            d_in.free(), d_out.free()
            h.close()
    logl = a.p1_log_leaves
    cfg = MerkleTreeConfig.default()
    cfg.is_tree_on_device = True
    for field in POSEIDON_FIELDS:
        t = 3 if field != "bls12_381" else 5
        arity = t - 1
        layers = -(-logl // (arity.bit_length() - 1))
        count = arity ** layers
        d_leaves = DeviceVec.from_host(rng.integers(0, 1 << 28, 8 * count, dtype=np.uint64).astype(np.uint32))
        hashers = [Hasher.poseidon(field, t, domain_tag=0)] * layers

        def build():
            tree = MerkleTree(hashers, 32)
            tree.build(d_leaves, cfg=cfg)
            tree.close()

        ts = all_interleaved([build], a.reps)
        hashes = (count - 1) // (arity - 1)
        say(f"poseidon {field} merkle build {count} leaves x 32 B (t={t} with a tag, arity {arity}), {layers} layers, {hashes} hashes: median {med(ts[0]):.3f} ms "
            f"({ts[0][0]:.3f} .. {ts[0][-1]:.3f}), {hashes / med(ts[0]) * 1e3:.3e} hashes/s")
        d_leaves.free()
    regs = kernel_rows("k_poseidon_")
    for name in sorted(regs, key=lambda k: (k.split("<")[0], k.split("<")[1].split(",")[0], int(k.split(", ")[1].rstrip(">")))):
        v, sg, scratch = regs[name]
        say(f"{name}: {v} VGPRs, {sg} SGPRs, {scratch} B of scratch per lane")
    if a.notes:
        with open(a.notes, "w") as f:
            f.write("```\n" + "\n".join(lines) + "\n```\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poseidon2", action="store_true")
    ap.add_argument("--poseidon", action="store_true")
    ap.add_argument("--p1-log-leaves", type=int, default=16)
    ap.add_argument("--p2-log-leaves", type=int, default=18)
    ap.add_argument("--p2-fields", nargs="+", default=["babybear", "koalabear"],
                    choices=["babybear", "koalabear", "bn254", "bls12_381", "bls12_377", "grumpkin", "stark252", "goldilocks"])
    ap.add_argument("--p2w-log-leaves", type=int, default=14)
    ap.add_argument("--notes", default=None)
    ap.add_argument("--openings", action="store_true")
    ap.add_argument("--open-log-leaves", type=int, default=20)
    ap.add_argument("--open-counts", type=int, nargs="*", default=[200, 4000])
    ap.add_argument("--fri", action="store_true")
    ap.add_argument("--fri-log-n", type=int, nargs="*", default=[20, 24])
    ap.add_argument("--field", default="babybear_extension",
                    choices=["babybear_extension", "goldilocks", "goldilocks_extension", "stark252", "bn254", "bls12_381", "bls12_377"])
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
    if a.fri:
        return fri_bench(a)
    if a.openings:
        return openings_bench(a)
    if a.poseidon2:
        return poseidon2_bench(a)
    if a.poseidon:
        return poseidon_bench(a)
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
