"""CPU: bench.py's launcher contract (VERDICT r02 item 2 i): `python bench.py --gpus N` without a rendezvous in the
environment must not die on an assertion -- it launches itself one rank per GPU, or, on a box with fewer than N GPUs,
prints ONE JSON line with an "error" key and exits 0."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_gpus_n_without_enough_devices_reports_json_error():
    import torch

    have = torch.cuda.device_count() if torch.cuda.is_available() else 0
    want = max(2, have + 1)
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(want), "--size-log2", "16"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == want and out["value"] is None
    assert f"needs {want} devices" in out["error"]
    assert out["metric"] == "bn254_msm_2^26_per_sec" and out["unit"] == "MSM/s"


def test_bench_rank_count_mismatch_is_a_json_error_too():
    """WORLD_SIZE set by a launcher but different from --gpus: a JSON line, not a traceback"""
    env = dict(os.environ)
    env.update({"WORLD_SIZE": "3", "RANK": "0", "LOCAL_RANK": "0"})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads([ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")][-1])
    assert "error" in out and "WORLD_SIZE=3" in out["error"]


@pytest.mark.gpu
def test_bench_inprocess_leg_rehearsed_on_virtual_slots():
    """the single-process leg of `bench.py --gpus N` (ONE msm() / ntt() call with hip_num_devices = N, bases resident) run
    with 4 virtual device slots + loopback collectives on the one GPU of the test box: the leg's own code, its JSON and
    its wire-byte accounting (the second call ships scalars only)"""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env["ICICLE_BENCH_INPROC_VIRTUAL"] = "1"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--inproc-only", "--size-log2", "16", "--ntt-log2", "14", "--ntt-batch", "4"],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads([ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")][-1])
    assert "error" not in out, out
    assert out["n_gpus"] == 4 and out["value"] > 0 and "rehearsal" in out
    assert out["wire_bytes_per_call"]["bases"] == 0 and out["wire_bytes_per_call"]["scalars"] == 3 * (1 << 16) * 32  # three remote slots
    assert out["resident_base_hits_per_call"] == 3
    assert out["ntt"]["roundtrip_ok"] is True
    assert out["result_ok"] is True  # the timed result equals the sum of plain single-GPU MSMs over the shards


@pytest.mark.gpu
def test_bench_one_process_per_gpu_leg_rehearsed_with_two_ranks():
    """`bench.py --gpus 2 --full` end to end on the ONE GPU of the test box -- the self-launch under
    torch.distributed.run, two ranks (sharing GPU 0, collectives over gloo: ICICLE_BENCH_GLOO_REHEARSAL), the weak line, the
    strong object, the split transform with its all-to-alls, the watchdogs, and the in-process leg (virtual slots) -- so that
    every line of the N > 1 path has executed before the driver's 8-GPU node runs it over RCCL."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env["ICICLE_BENCH_GLOO_REHEARSAL"] = "1"
    env["ICICLE_BENCH_INPROC_VIRTUAL"] = "1"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--size-log2", "18",
                        "--ntt-log2", "16", "--ntt-batch", "8", "--full"], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    out = json.loads(lines[0])
    assert "error" not in out, out
    assert out["n_gpus"] == 2 and out["scaling"] == "weak" and out["value"] > 0 and "rehearsal" in out
    assert out["strong"]["value"] > 0 and out["strong"]["n_gpus"] == 2, out.get("strong")
    assert out["ntt"]["roundtrip_ok"] is True and out["ntt"]["value"] > 0
    assert out["ntt_split"]["roundtrip_ok"] is True, out.get("ntt_split")
    assert out["inproc"]["result_ok"] is True and out["inproc"]["n_gpus"] == 2, out.get("inproc")


@pytest.mark.gpu
def test_bench_dump_outputs_are_the_last_steps_results_and_repeat(tmp_path):
    """`--dump-outputs DIR`: after the timed steps the MSM result (affine) and a seeded sample of the
    NTT's forward / inverse outputs land in DIR as float64 .npy files of at most 64 MB; the line still reports exactly --steps
    timed steps with ms_per_step; and a second run with the same arguments dumps the same values (seeded inputs)."""
    import numpy as np

    from oracle import pyref

    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    dumped = []
    for run in range(2):
        d = tmp_path / f"run{run}"
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--size-log2", "16",
                            "--ntt-log2", "14", "--ntt-batch", "4", "--no-cpu-baseline", "--dump-outputs", str(d)],
                           capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        out = json.loads([ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")][-1])
        assert "error" not in out, out
        assert out["steps"] == 3 and out["ms_per_step"] > 0 and out["ntt"]["roundtrip_ok"] is True
        names = {"msm_result_affine.npy", "ntt_sample_index.npy", "ntt_forward_sample.npy", "ntt_inverse_sample.npy"}
        assert set(out["dump_outputs"]["files"]) == names == set(os.listdir(d))
        arrs = {n: np.load(d / n) for n in names}
        assert all(a.dtype == np.float64 for a in arrs.values())
        assert sum(os.path.getsize(d / n) for n in names) <= 64 << 20
        dumped.append(arrs)
    a = dumped[0]
    C = pyref.BN254
    w = [int(v) for v in a["msm_result_affine.npy"][0]]
    x, y = (sum(v << (32 * k) for k, v in enumerate(w[8 * i:8 * (i + 1)])) for i in range(2))
    assert (x, y) != pyref.INF and pyref.on_curve(C, (x, y))
    assert a["msm_result_affine.npy"].shape == (1, 16) and a["ntt_forward_sample.npy"].shape == (4 << 14,)  # 2^16 elements: all of them
    assert np.array_equal(a["ntt_sample_index.npy"], np.arange(4 << 14))
    assert a["ntt_forward_sample.npy"].max() < pyref.BABYBEAR.p and a["ntt_inverse_sample.npy"].max() < pyref.BABYBEAR.p
    for n in sorted(a):
        assert np.array_equal(a[n], dumped[1][n]), n


@pytest.mark.gpu
def test_bench_plain_run_is_the_headline_alone_and_full_adds_the_rest():
    """A plain `bench.py --gpus 1` run prints the headline line and nothing it does not need; `--full` adds the NTT secondary
    metric, the in-run ALU and gather roofs and the CPU baseline, as every run did before --full existed"""
    from oracle import ref

    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}

    def run(*extra):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--size-log2", "16",
                            "--ntt-log2", "14", "--ntt-batch", "4", *extra], capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
        assert len(lines) == 1, r.stdout[-3000:]
        out = json.loads(lines[0])
        assert "error" not in out, out
        assert out["metric"] == "bn254_msm_2^26_per_sec" and out["unit"] == "MSM/s" and out["higher_is_better"] is True
        assert out["steps"] == 2 and out["warmup"] == 1 and out["ms_per_step"] > 0 and out["value"] > 0 and out["dtype"]
        assert out["roofline"]["launches"] > 0 and out["roofline"]["avg_launch_ms"] > 0
        return out

    plain = run()
    assert not {"ntt", "cpu_baseline", "config3_shard", "config4_shard", "dump_outputs"} & set(plain), sorted(plain)
    assert not {"alu", "gather"} & set(plain["roofline"])
    full = run("--full")
    assert full["ntt"]["roundtrip_ok"] is True and full["ntt"]["value"] > 0 and full["ntt"]["roofline"]["alu"]["roof"] > 0
    assert full["roofline"]["alu"]["roof"] > 0 and full["roofline"]["gather"]["measured_ceiling"] > 0
    assert "cpu_baseline" in full
    if ref.available("bn254") and ref.available("babybear"):
        assert full["cpu_baseline"]["parity_with_gpu_on_sample"] is True, full["cpu_baseline"]
        assert full["ntt"]["cpu_baseline"]["parity_with_gpu_on_sample"] is True, full["ntt"]["cpu_baseline"]
