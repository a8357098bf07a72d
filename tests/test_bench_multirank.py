"""bench.py multi-rank path (the driver's 8-GPU scaling contract),
exercised here with world_size=2 on gloo + the host copy path
(KVC_BENCH_CPU_FULL=1). Covers rank coordination, barriers, the peer
phase, max-over-ranks reduction and the single-JSON-line contract."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent

# These are the CPU twins of the GPU runs: the launched ranks must take the
# gloo + host-copy path on every machine, so any GPU is hidden from them
# (with one visible, ranks >= 1 of a multi-rank run would find no device).
NO_GPU = {"CUDA_VISIBLE_DEVICES": "", "HIP_VISIBLE_DEVICES": ""}


@pytest.mark.timeout(420)
def test_bench_world2_cpu_full(tmp_path):
    env = dict(os.environ)
    env.update(NO_GPU)
    env.update({
        "KVC_BENCH_CPU_FULL": "1",
        "MASTER_ADDR": "127.0.0.1",
        "MASTER_PORT": "29571",
    })
    out = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29571", str(REPO / "bench.py"),
         "--gpus", "2", "--steps", "2", "--warmup", "1", "--full",
         "--root", str(tmp_path), "--device-blocks", "1536",
         "--io-threads", "2"],
        capture_output=True, text=True, timeout=400, env=env, cwd=str(REPO),
    )
    assert out.returncode == 0, f"stdout:\n{out.stdout}\nstderr:\n{out.stderr}"
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    d = json.loads(lines[0])
    assert d["metric"] == "kv_block_offload_GBps"
    assert d["value"] is not None and d["value"] > 0
    assert d["scaling"] == "weak"
    peer = d["aux"]["peer_xgmi"]
    assert peer["ok"] is True
    assert peer["n_pulls"] == 32
    assert peer["pull_GBps_aggregate"] > 0


@pytest.mark.timeout(240)
def test_bench_single_rank_cpu_control_plane():
    out = subprocess.run(
        [sys.executable, str(REPO / "bench.py"), "--steps", "2", "--warmup", "1",
         "--full"],
        capture_output=True, text=True, timeout=220, cwd=str(REPO),
    )
    assert out.returncode == 0, out.stderr
    d = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][0])
    assert d["aux"]["score_req_s"] > 100
    assert d["aux"]["ingest_batches_s"] > 100


@pytest.mark.timeout(600)
def test_bench_world8_tiny_cpu(tmp_path):
    """World-8 CPU sim of the driver's 8-GPU scaling run:
    the full bench path — rank coordination, barriers, the peer-mesh
    phase, max-over-ranks — at the scaling run's world size, tiny
    geometry."""
    env = dict(os.environ)
    env.update(NO_GPU)
    env.update({
        "KVC_BENCH_CPU_FULL": "1",
        "KVC_BENCH_TINY": "1",
        "MASTER_ADDR": "127.0.0.1",
        "MASTER_PORT": "29573",
    })
    out = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "8", "--master-addr", "127.0.0.1",
         "--master-port", "29573", str(REPO / "bench.py"),
         "--gpus", "8", "--steps", "1", "--warmup", "0", "--full",
         "--root", str(tmp_path), "--device-blocks", "512",
         "--io-threads", "1"],
        capture_output=True, text=True, timeout=580, env=env, cwd=str(REPO),
    )
    assert out.returncode == 0, f"stdout:\n{out.stdout}\nstderr:\n{out.stderr}"
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    d = json.loads(lines[0])
    assert d["config"]["parallelism"] == "dp8"
    assert d["value"] is not None and d["value"] > 0
    peer = d["aux"]["peer_xgmi"]
    assert peer["ok"] is True, peer
    assert peer["pull_GBps_aggregate"] > 0


def _plain_dump_run(tmp_path, tag):
    env = dict(os.environ)
    env.update({"KVC_BENCH_CPU_FULL": "1", "KVC_BENCH_TINY": "1"})
    dump = tmp_path / f"dump_{tag}"
    out = subprocess.run(
        [sys.executable, str(REPO / "bench.py"), "--gpus", "1",
         "--steps", "3", "--warmup", "1",
         "--root", str(tmp_path / f"root_{tag}"),
         "--device-blocks", "512", "--io-threads", "2",
         "--dump-outputs", str(dump)],
        capture_output=True, text=True, timeout=100, env=env, cwd=str(REPO),
    )
    assert out.returncode == 0, f"stdout:\n{out.stdout}\nstderr:\n{out.stderr}"
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0]), dump


@pytest.mark.timeout(240)
def test_bench_plain_run_is_lean_and_dumps_outputs(tmp_path):
    """A plain run (no --full) times its steps and nothing else — no aux
    phases — and --dump-outputs leaves the last step's loaded pages and
    stored-file bytes as float32 .npy files: the loaded pages are the bytes
    the store wrote, and a second run with the same arguments dumps the
    same arrays (tiny geometry; the GPU path where there is a GPU, the host
    copy path otherwise)."""
    import numpy as np

    d, dump = _plain_dump_run(tmp_path, "a")
    assert d["aux"] is None
    assert d["steps"] == 3 and d["ms_per_step"] > 0
    # 3 timed + 1 warmup generations of 16 files each went to storage
    assert d["config"]["files_written"] == 4 * 16
    names = ["loaded_kv.npy", "stored_file_first.npy", "stored_file_last.npy"]
    assert sorted(p.name for p in dump.iterdir()) == names
    kv = np.load(dump / "loaded_kv.npy")
    # tiny geometry: 4 layers x 64 KiB blocks -> 32 sampled blocks, the
    # step's first (0) and last (255) block among them
    assert kv.dtype == np.float32 and kv.shape == (4, 32, 64 * 1024)
    assert kv.min() >= 0 and kv.max() <= 254  # randint(0, 255) bytes
    total = kv.nbytes
    # Every generation stores pages [0, B) and the load scatters a stored
    # generation into the disjoint window [B, 2B), which starts out with
    # other random bytes. A raw KV file is the packed blocks, 64 KiB each,
    # so every sampled 4 KiB chunk of the first file that belongs to block
    # 0 (1/16 of the file, ~16 of the 256 chunks) must reappear in loaded
    # block 0, likewise the last file and block 255 — and none would if
    # the load had not run.
    for name, blk in (("stored_file_first.npy", 0), ("stored_file_last.npy", -1)):
        a = np.load(dump / name)
        assert a.dtype == np.float32 and a.shape == (256, 4096)
        assert a.min() >= 0 and a.max() <= 254
        total += a.nbytes
        pieces = {kv[layer, blk, o:o + 4096].tobytes()
                  for layer in range(4) for o in range(0, 64 * 1024, 4096)}
        hits = sum(row.tobytes() in pieces for row in a)
        assert hits >= 4, (name, hits)
    assert total <= 64 * 10**6

    # same arguments, new process: identical inputs, identical outputs
    _, dump_b = _plain_dump_run(tmp_path, "b")
    for name in names:
        assert np.array_equal(np.load(dump / name), np.load(dump_b / name)), name
