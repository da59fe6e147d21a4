"""bench.py under the driver's contract, on CPU/gloo with a tiny model: the single-process run and
the torchrun launch with world_size 2 (the multi-GPU command line, RCCL replaced by gloo). Checks
the one JSON line rank 0 prints: whole-job value, N, steps/warmup echo, weak scaling."""
import json
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--steps", "4", "--warmup", "2", "--model", "gpt2-tiny", "--batch", "2", "--seq", "32", "--H", "2"]


def _env():
    return dict(os.environ, OMP_NUM_THREADS="1", CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")


def _json_line(stdout: str) -> dict:
    lines = [ln for ln in stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, stdout[-2000:]
    return json.loads(lines[0])


def _check(rec: dict, n: int):
    assert rec["n_gpus"] == n and rec["steps"] == 4 and rec["warmup"] == 2
    assert rec["value"] > 0 and rec["ms_per_step"] > 0 and rec["higher_is_better"] is True
    assert rec["scaling"] == "weak" and rec["config"]["global_batch"] == 2 * n
    # value is the whole-job rate: N x per-peer batch x steps / max-over-ranks time
    assert abs(rec["value"] - n * 2 * 4 / (rec["ms_per_step"] * 4 / 1e3)) / rec["value"] < 1e-2


def test_bench_single_process():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *ARGS], cwd=ROOT, env=_env(),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    _check(_json_line(r.stdout), 1)


def test_bench_dump_outputs_repeat(tmp_path):
    """--dump-outputs writes, as float32 .npy files, what the timed path computes in one step from the seeded
    initial state on the first batch (run after the timed steps). It depends on the arguments that shape the
    inputs only: a second run, here with --full (which adds nothing at one rank) and another number of timed
    steps, writes the same arrays, and --steps is what sets the number of timed steps."""
    import numpy as np

    def run(out, *extra):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *ARGS, "--dump-outputs",
                            str(out), *extra], cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        return _json_line(r.stdout), {p.stem: np.load(p) for p in sorted(out.glob("*.npy"))}

    rec_a, a = run(tmp_path / "a")
    rec_b, b = run(tmp_path / "b", "--full", "--steps", "5")
    _check(rec_a, 1)
    assert rec_b["steps"] == 5 and rec_b["final_loss"] != rec_a["final_loss"]
    assert set(a) == set(b) == {"loss", "params", "grad", "adam_m", "adam_v"}
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    for k in a:
        assert a[k].dtype == np.float32 and np.isfinite(a[k]).all() and np.array_equal(a[k], b[k]), k
    assert a["params"].shape == a["grad"].shape == a["adam_m"].shape == a["adam_v"].shape
    assert np.abs(a["grad"]).max() > 0 and np.abs(a["adam_m"]).max() > 0
    assert abs(float(a["loss"][0]) - np.log(512)) < 0.5  # the first step of a random-init model: ~ln(vocab)


def test_dump_outputs_rewind_and_seeded_sample(tmp_path, monkeypatch):
    """_dump_outputs on a trainer that has moved on: the rewind restores the whole seeded start (its step equals a
    fresh trainer's first step, taken as the last of its round so the averaging round runs), and a state vector
    longer than DUMP_SAMPLE is written as the seeded, sorted index sample of the full vector."""
    import importlib.util

    import numpy as np
    import torch

    from distributedvolunteercomputing_amd.models.gpt2 import GPT2, GPT2Config
    from distributedvolunteercomputing_amd.parallel.local_sgd import LocalSGDConfig, LocalSGDTrainer

    spec = importlib.util.spec_from_file_location("vcx_bench_dump_mod", os.path.join(ROOT, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    cfg = GPT2Config.preset("gpt2-tiny")

    def make():
        torch.manual_seed(0)
        return LocalSGDTrainer(GPT2(cfg).to(dtype=torch.bfloat16), LocalSGDConfig(H=2), device=torch.device("cpu"))

    tok = torch.randint(0, cfg.vocab_size, (2, 33), generator=torch.Generator().manual_seed(5))
    x, y = tok[:, :-1], tok[:, 1:]
    tr = make()
    init = (tr.flat.param.clone(), tr.ostate.clone())
    for _ in range(3):
        tr.step(x, y)  # the timed steps: parameters, moments, optimizer state and anchor all move
    n, k = tr.flat.numel, 1000
    assert n > k

    def dump(name, sample):
        monkeypatch.setattr(b, "DUMP_SAMPLE", sample)
        b._dump_outputs(str(tmp_path / name), tr, init, x, y)
        return {p.stem: np.load(p) for p in sorted((tmp_path / name).glob("*.npy"))}

    full = dump("full", n)
    part = dump("part", k)  # second rewind of the same trainer
    ref = make()
    ref.t = ref.cfg.H - 1
    st = ref.step(x, y)
    assert st.synced and tr.t == ref.t
    for name, t in (("params", ref.master), ("grad", ref.flat.grad), ("adam_m", ref.m), ("adam_v", ref.v)):
        assert full[name].shape == (n,) and np.array_equal(full[name], t.float().numpy()), name
    assert np.array_equal(full["loss"], st.extra["loss_t"].detach().float().reshape(1).numpy())
    assert torch.equal(tr.anchor, ref.anchor) and torch.equal(tr.ostate, ref.ostate)
    idx = torch.randint(0, n, (k,), generator=torch.Generator().manual_seed(b.DUMP_SEED)).sort().values.numpy()
    assert len(np.unique(idx)) > k // 2 and idx.min() >= 0 and idx.max() < n
    for name in ("params", "grad", "adam_m", "adam_v"):
        assert part[name].dtype == np.float32 and np.array_equal(part[name], full[name][idx]), name
    assert np.array_equal(part["loss"], full["loss"])
    assert sum(v.nbytes for v in part.values()) == 4 * k * 4 + 4
    assert 4 * b.DUMP_SAMPLE * 4 + 4 <= 64 << 20  # the shipped sample size keeps a dump under 64 MB


@pytest.mark.slow
def test_bench_gpus_flag_spawns_ranks_without_torchrun(tmp_path):
    """The driver's literal `python bench.py --gpus 4` (no launcher): bench.py starts 4 ranks itself
    (a child torch.distributed.run, never an exec) and the JSON reports the group that formed. The
    spawning parent loads neither torch nor the HIP runtime, and the JSON carries
    the averaging round's bytes, time and bandwidth (measured with --full only)."""
    libs = tmp_path / "parent_libs.txt"
    env = dict(_env(), VCX_BENCH_PARENT_LIBS=str(libs))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--full", *ARGS], cwd=ROOT,
                       env=env, capture_output=True, text=True, timeout=400)
    assert r.returncode == 0, r.stderr[-3000:]
    rec = _json_line(r.stdout)
    _check(rec, 4)
    assert rec["rccl_world"] == 4 and rec["backend"] == "gloo" and len(rec["devices"]) == 4
    assert rec["sync_rounds_timed"] == 2 and rec["sync_ms_timed_mean"] > 0  # H = 2, 4 timed steps
    loaded = libs.read_text().split()
    assert loaded and not [x for x in loaded if "amdhip64" in x or "libtorch" in x or "hsa-runtime" in x], loaded
    assert rec["avg_bytes_per_rank"] > 0 and rec["avg_collective_ms_mean"] > 0
    assert rec["avg_algbw_GBps"] > 0 and abs(rec["avg_busbw_GBps"] / rec["avg_algbw_GBps"] - 1.5) < 5e-2
    assert rec["rccl_transports"] is None  # gloo: no RCCL connection lines


def test_bench_mismatched_launch_fails_loudly():
    """--gpus 4 under a 2-rank launch must not report a 2-rank number as a 4-GPU run."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(port), "bench.py", "--gpus", "4", *ARGS]
    r = subprocess.run(cmd, cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert "WORLD_SIZE=2" in r.stderr


def _torchrun(n, extra=()):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr",
           "127.0.0.1", "--master-port", str(port), "bench.py", "--gpus", str(n), *ARGS, *extra]
    r = subprocess.run(cmd, cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=400)
    assert r.returncode == 0, r.stderr[-3000:]
    rec = _json_line(r.stdout)
    _check(rec, n)
    assert f"dp{n}" in rec["config"]["parallelism"]
    return rec


@pytest.mark.slow
def test_bench_torchrun_two_ranks():
    rec = _torchrun(2)
    assert "allreduce=direct" in rec["config"]["parallelism"]  # the default averaging schedule


@pytest.mark.slow
@pytest.mark.parametrize("n,algo", [(4, "direct"), (4, "butterfly"), (4, "ring"), (4, "rs_ag"), (4, "rccl"),
                                    (8, "direct"), (8, "butterfly")])
def test_bench_torchrun_more_ranks(n, algo):
    """The driver's multi-GPU command line at 4 and 8 ranks, each averaging algorithm (gloo)."""
    rec = _torchrun(n, ["--algo", algo])
    assert f"allreduce={algo}" in rec["config"]["parallelism"]
    assert rec["sync_ms"] > 0


def test_rehearsal_launcher_propagates_a_failed_rank(tmp_path):
    """scripts/rccl_rehearsal_launch.py: every rank gets the torchrun env and its own NCCL_HOSTID;
    one rank failing ends the job with that rank's exit status (the others are killed)."""
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prog = ("import os, sys, time\n"
            "r = int(os.environ['RANK'])\n"
            "assert os.environ['WORLD_SIZE'] == '3' and os.environ['NCCL_HOSTID'] == f'vcx-rehearsal-{r}'\n"
            "sys.exit(7) if r == 1 else time.sleep(60)\n")
    cmd = [sys.executable, os.path.join(root, "scripts", "rccl_rehearsal_launch.py"), "--nproc", "3", "--timeout", "50",
           "--", sys.executable, "-c", prog]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=90)
    assert r.returncode == 7, r.stderr


def test_rccl_transport_parse_and_gpu_count(tmp_path, monkeypatch):
    """The transport counts come from RCCL's connection lines; the parent's GPU count from the
    visible-devices lists (intersection = the shortest) without any HIP call."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("vcx_bench_mod", os.path.join(ROOT, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    log = tmp_path / "rank0.log"
    log.write_text("host:1:2 [0] NCCL INFO Channel 00/0 : 0[0] -> 1[1] via P2P/IPC\n"
                   "host:1:2 [0] NCCL INFO Channel 01/0 : 0[0] -> 1[1] via P2P/IPC\n"
                   "host:1:2 [0] NCCL INFO Channel 00/1 : 0[0] -> 2[2] via SHM/direct/direct\n"
                   "host:1:2 [0] NCCL INFO Using network Socket\n")
    assert b._rccl_transports(str(log)) == {"P2P/IPC": 2, "SHM/direct/direct": 1}
    assert not log.exists()  # parsed once, then removed
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", "0,1,2,3")
    monkeypatch.setenv("ROCR_VISIBLE_DEVICES", "0,1")
    monkeypatch.delenv("CUDA_VISIBLE_DEVICES", raising=False)
    assert b._visible_gpus() == 2
