"""bench.py on the GPU: the JSON line of a short run (config 2, one solve) keeps the driver's contract, single-GPU and through
the multi-rank entry point with the ranks sharing the one GPU (host test transport)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
        "dtype", "data", "config", "roofline")


def run_bench(*args, env=None):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True, timeout=900,
                       cwd=ROOT, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", **(env or {})))
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    last = p.stdout.strip().splitlines()[-1]
    return json.loads(last)                                   # the JSON line is the LAST line of stdout


def check_common(d, n_gpus, steps, warmup):
    for k in KEYS:
        assert k in d, k
    assert d["metric"] == "chebyshev_filter_hemm_gflops" and d["unit"] == "GFLOP/s" and d["higher_is_better"] is True
    assert (d["n_gpus"], d["steps"], d["warmup"]) == (n_gpus, steps, warmup)
    assert d["scaling"] == "strong" and d["vs_baseline"] is None and d["data"] == "synthetic" and d["dtype"] == "complex f64"
    assert "workload" in d["config"] and "model" not in d["config"]
    r = d["roofline"]
    assert r["bound"] == "mfma" and r["unit"] == "TFLOP/s" and r["peak"] == 78.6
    assert 0.0 < r["frac"] <= 1.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12
    assert d["converged"] is True and d["spectrum_check"]["ok"] is True
    assert 0.0 < d["max_resid_recomputed"] < 1e-8                                            # independent check, fresh four-product H V
    assert len(d["timed"]["iterations"]) == steps
    assert d["ms_per_step"] > 0 and d["value"] > 0


def test_single_gpu_line_keeps_the_contract():
    d = run_bench("--workload", "cfg2", "--steps", "9", "--warmup", "0", "--cpu-budget", "3", "--full")
    check_common(d, 1, 9, 0)
    # the oracle's solve of config 2 at full size (tests/golden/oracle_cfg2_fullsize.json; the single-GPU Impl takes it count for
    # count from the oracle's matrix and start block, tests/test_gpu_fullsize.py): the bench workload differs from it by the
    # 1e-6 perturbation and the device generator's start block - same iterations, filtered vectors within 2 % (observed: 101 708
    # against the oracle's 102 614)
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "oracle_cfg2_fullsize.json")))["unperturbed"]
    assert d["iterations_per_solve"] == gold["iterations"]
    assert abs(d["filtered_vecs_per_solve"] - gold["filtered_vecs"]) <= 0.02 * gold["filtered_vecs"], d["filtered_vecs_per_solve"]
    assert d["roofline"]["frac"] > 0.5                                                       # a fallback path would not get here
    assert 1.0 < d["solve_seconds"] < 6.0 and d["eigenpairs_per_sec"] > 80                   # the solve's own seconds (2.5 s), no bench waits in them
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] >= 1 and c["value"] > 0 and "extrapolated" in c["sample"]
    for probe in ("roofline_4m", "roofline_3m_fullwidth"):
        assert 0.0 < d[probe]["frac"] <= 1.0
    assert d["roofline"]["executed_over_model"] == pytest.approx(0.75, abs=0.02)             # 3M filter products


def test_plain_single_gpu_run_is_lean_and_dumps_what_the_timed_steps_computed(tmp_path):
    """A plain run (no --full): the headline figure of K timed iterations after W warm-up ones and nothing else - no CPU
    baseline, no kernel probes, no extra solve; --dump-outputs writes the state after the last timed step, the same from
    run to run (seeded matrix and start block)."""
    import numpy as np
    runs = []
    for i in range(2):
        d = run_bench("--workload", "cfg2", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / str(i)))
        assert d["metric"] == "chebyshev_filter_hemm_gflops" and d["unit"] == "GFLOP/s" and d["higher_is_better"] is True
        assert (d["n_gpus"], d["steps"], d["warmup"], d["full"]) == (1, 3, 1, False) and d["dtype"] == "complex f64"
        assert d["value"] > 0 and d["ms_per_step"] > 0 and 0.0 < d["roofline"]["frac"] <= 1.0
        assert [(t["solve"], t["iteration"]) for t in d["timed"]["iterations"]] == [(1, 0), (1, 1), (1, 2)]
        assert d["complete_solves"] == 0
        for k in ("cpu_baseline", "roofline_4m", "roofline_3m_fullwidth", "converged", "spectrum_check"):
            assert k not in d, k
        runs.append({f.name: np.load(f) for f in (tmp_path / str(i)).glob("*.npy")})
    a, b = runs
    assert sorted(a) == ["residuals.npy", "ritz_values.npy", "ritz_vectors_sample.npy", "ritz_vectors_sample_rows.npy"]
    assert a["ritz_values.npy"].shape == (640,) and a["ritz_vectors_sample.npy"].shape == (1024, 512, 2)
    for k in a:
        assert a[k].dtype == np.float64 and np.all(np.isfinite(a[k]))
        assert np.allclose(a[k], b[k], rtol=1e-10, atol=1e-12), k


def test_multi_rank_entry_point_on_one_gpu():
    d = run_bench("--gpus", "4", "--workload", "cfg2", "--n", "8192", "--steps", "6", "--warmup", "0", "--no-cpu-baseline",
                  env={"CHASE_HIP_TRANSPORT": "host", "CHASE_HIP_PROBE_HOST": "1"})
    check_common(d, 4, 6, 0)
    assert d["config"]["grid"] == "2x2" and d["config"]["transport"] == "host"
    p = d["comm_probe"]
    assert p["col_group_panel_allreduce"]["ranks"] == 2 and p["panel_gemm_alone_ms_rounds4"] > 0
    # every multi-rank run times a 256 MB all-reduce per communicator before it solves (a host-staged RCCL group fails it)
    t = d["transport_proof"]
    assert t["ok"] and t["row_group"]["ranks"] == 2 and t["col_group"]["busbw_GBps"] > 0
    lat = t["small_allreduce_latency_us"]                       # 64-double all-reduces: per communicator and alternating
    assert lat["col_group"] > 0 and lat["row_group"] > 0 and lat["alternating"] > 0 and lat["comm_streams"] == 1


def test_thread_per_gpu_mode_on_one_gpu():
    """`bench.py --gpus 4 --ranks threads`: ONE process, one thread per rank - here four threads on this box's one
    device over the host test transport; on the multi-GPU node the same code opens device r in thread r and creates the RCCL
    communicators from the four threads."""
    d = run_bench("--gpus", "4", "--ranks", "threads", "--workload", "cfg2", "--n", "8192", "--steps", "6", "--warmup", "0",
                  "--no-cpu-baseline", "--no-probe", env={"CHASE_HIP_TRANSPORT": "host"})
    check_common(d, 4, 6, 0)
    assert d["config"]["grid"] == "2x2" and d["config"]["ranks"] == "threads of one process"
    assert d["transport_proof"]["ok"]


@pytest.mark.parametrize("ngpus,grid", [(2, "2x1"), (4, "2x2")])
def test_multi_rank_bench_with_real_rccl_collectives(ngpus, grid):
    """`bench.py --gpus N` end to end over REAL RCCL communicators of more than one rank (CHASE_BENCH_FAKE_HOSTS=1: one
    NCCL_HOSTID per rank process, socket transport, all ranks on this box's one GPU): the transport proof, the timed solves with
    the panel-pipelined all-reduces on the communication stream, the exposed-communication brackets, the independent residuals
    and the communication probe - a functional rehearsal of the multi-GPU run (the numbers say nothing about xGMI)."""
    d = run_bench("--gpus", str(ngpus), "--workload", "cfg2", "--n", "8192", "--steps", "6", "--warmup", "0", "--no-cpu-baseline",
                  env={"CHASE_BENCH_FAKE_HOSTS": "1"})
    check_common(d, ngpus, 6, 0)
    assert d["config"]["grid"] == grid and d["config"]["transport"] == "rccl" and "SOCKET transport" in d["config"]["workload"]
    assert d["ranks_seen_by_rccl"]["grid"] == ngpus                           # what ncclCommCount itself reports
    assert d["transport_proof"]["col_group"]["ranks"] == 2 and d["transport_proof"]["col_group"]["busbw_GBps"] > 0
    assert d["comm_waits"] > 0 and d["comm_exposed_ms"] > 0                      # the compute stream really waited on collectives
    assert d["comm_probe"]["col_group_panel_allreduce"]["ranks"] == 2
    # first contact with the "hardware": the panel-pipeline knobs were measured on identical full-width filter steps before
    # the first solve and the best setting locked (chase_amd/autotune.py); the table is in the line
    a = d["autotune"]
    assert a["base"] == {"panel_cols": a["base"]["panel_cols"], "panel_rounds": 4, "comm_streams": 1}
    assert 2 <= len(a["trials"]) <= 5 and a["trials"][0]["setting"] == a["base"]
    assert sum(t["kept"] for t in a["trials"]) == 1 and [t for t in a["trials"] if t["kept"]][0]["setting"] == a["chosen"]
    assert all(t["seconds"] > 0 for t in a["trials"])
    # two communication streams are opt-in until seen on xGMI (round-5 advisor): not tried, and the line says so
    assert all(t["setting"]["comm_streams"] == 1 for t in a["trials"]) and any(k["knob"] == "comm_streams" for k in a["skipped"])
    assert d["scaling_valid"] is False          # RCCL over fake hosts' sockets: a rehearsal, never a scaling number


def test_pseudo_hermitian_workload_over_real_rccl_with_self_tuning():
    """BASELINE configs[4]'s path (Solve_pseudo on the grid Impl, H^2 filter) through `bench.py --gpus 4` over REAL RCCL
    communicators (fake hosts: socket transport, four rank processes on this box's GPU) at N = 4096: the first-contact self-tuning
    runs its trial steps with HEMM_H2 (round 5: it used to be skipped for this workload, whose default panel then hid nothing of
    an all-reduce), the solve converges, the line carries the table."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--workload", "cfg5", "--n", "4096", "--steps", "6",
                        "--warmup", "0", "--no-cpu-baseline", "--no-probe"], capture_output=True, text=True, timeout=600, cwd=ROOT,
                       env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", CHASE_BENCH_FAKE_HOSTS="1", CHASE_HIP_AUTOTUNE_TRIALS="3"))
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-2500:])
    d = json.loads(p.stdout.strip().splitlines()[-1])
    assert d["n_gpus"] == 4 and d["config"]["grid"] == "2x2" and d["config"]["transport"] == "rccl"
    assert "pseudo-Hermitian" in d["config"]["workload"]
    assert d["converged"] is True and 0.0 < d["max_resid_recomputed"] < 1e-8
    a = d["autotune"]
    assert a["base"]["panel_cols"] == 128 and a["base"]["comm_streams"] == 1            # 320 filter columns: capped at 1 / 2.5 of them
    assert len(a["trials"]) == 3 and [t["setting"]["panel_cols"] for t in a["trials"]] == [128, 256, 512]
    assert sum(t["kept"] for t in a["trials"]) == 1 and all(t["seconds"] > 0 for t in a["trials"])
    assert d["scaling_valid"] is False


def test_config3_at_full_size_over_real_rccl_communicators():
    """BASELINE configs[2] exactly as the 4-GPU job runs it (N = 32768 real symmetric, nev = 1024, nex = 256, 2 x 2 block
    distribution, RCCL row / column all-reduces) - with the four rank processes sharing this box's one GPU and RCCL on its socket
    transport (one NCCL_HOSTID per rank): same iteration and filtered-vector counts as the host-fabric run of
    tests/test_gpu_fullsize.py, analytic spectrum, independent residuals."""
    d = run_bench("--gpus", "4", "--workload", "cfg3", "--steps", "9", "--warmup", "0", "--no-cpu-baseline", "--no-probe",
                  "--no-autotune", env={"CHASE_BENCH_FAKE_HOSTS": "1"})
    assert d["autotune"] is None
    assert d["n_gpus"] == 4 and d["config"]["grid"] == "2x2" and d["config"]["transport"] == "rccl" and d["dtype"] == "f64"
    assert d["ranks_seen_by_rccl"]["grid"] == 4
    assert d["iterations_per_solve"] == 9 and abs(d["filtered_vecs_per_solve"] - 207784) <= 0.005 * 207784
    assert d["converged"] is True and d["spectrum_check"]["ok"] is True and d["max_resid_recomputed"] < 1e-8
    assert d["comm_waits"] > 0


def test_launcher_ranks_settle_their_mode_with_real_probe_children():
    """the driver's multi-GPU call (`torch.distributed.run ... bench.py --gpus 2`) with `--ranks auto` and REAL RCCL (fake hosts):
    every rank starts its own probe child, the children build real communicators on their own port, run the 256 MB proof and
    agree; the ranks then bind and run the bench in the mode the probe passed"""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29741", os.path.join(ROOT, "bench.py"), "--gpus", "2", "--workload", "cfg2", "--size", "4096", "--steps", "4",
           "--warmup", "1", "--no-cpu-baseline", "--no-probe"]      # (--size: the launcher's own parser claims "--n...")
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT,
                       env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", CHASE_BENCH_FAKE_HOSTS="1"))
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-3000:])
    assert "probe of mode 'bound': exit status 0" in p.stderr and "bench probe [processes, one visible device each]" in p.stderr
    d = json.loads([l for l in p.stdout.strip().splitlines() if l.startswith("{")][-1])
    check_common(d, 2, 4, 1)
    assert d["config"]["ranks"] == "processes, one visible device each" and d["ranks_seen_by_rccl"]["grid"] == 2


def test_rank_of_a_torchrun_launch_on_one_gpu():
    """the driver's multi-GPU call: `python -m torch.distributed.run --nproc-per-node N bench.py --gpus N` - bench.py is then one
    of the ranks (RANK set by the launcher).  Two ranks sharing this box's one GPU through the host test transport (which
    leaves the device visibility alone; on the multi-GPU node every rank binds its runtime to its own device first)."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29723", os.path.join(ROOT, "bench.py"), "--gpus", "2", "--workload", "cfg2", "--size", "8192", "--steps", "4",
           "--warmup", "1", "--no-cpu-baseline", "--no-probe"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT,
                       env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", CHASE_HIP_TRANSPORT="host"))
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-3000:])
    lines = [l for l in p.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1                                      # rank 0 only
    d = json.loads(lines[-1])
    check_common(d, 2, 4, 1)
    assert d["config"]["grid"] == "2x1" and d["config"]["transport"] == "host"
    assert d["max_resid_recomputed"] < 1e-8
    audit = [l for l in p.stderr.splitlines() if "device bus id" in l]
    assert len(audit) == 2 and all("ncclCommCount" in l for l in audit)
