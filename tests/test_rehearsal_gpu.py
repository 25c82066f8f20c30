"""Multi-process pipeline on one GPU (EDGE_SHARED_GPU=1: ranks share cuda:0 over gloo with host-staged
p2p): the CUDA code path of the driver's N-GPU bench (graphs, streams, pipeline protocol) gives the same
PPL as the single-process run.  RCCL itself needs one GPU per rank and is covered by test_rccl_gpu.py."""
import json
import math
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["bench.py", "--model", "tiny-qwen2", "--batch", "4", "--microbatches", "2", "--steps", "3", "--warmup", "1",
        "--max-length", "256", "--split", "1"]


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(n, extra=(), env_extra=None, self_launch=False, full=False):
    """``bench.py --full`` on ``n`` ranks sharing cuda:0.  Without ``full`` the N = 1 extras (notebook-sweep timing,
    HF-eager comparison) and the N > 1 transports record are skipped: each test then stays well under a minute."""
    env = dict(os.environ, EDGE_SHARED_GPU="1", **(env_extra or {}))
    extra = list(extra) + ["--full"]
    if not full:
        extra = list(extra) + ["--no-sweep", "--no-hf-compare"] + (["--no-transports"] if n > 1 else [])
    if n == 1 or self_launch:
        cmd = [sys.executable] + ARGS + list(extra) + (["--gpus", str(n)] if self_launch else [])
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr",
               "127.0.0.1", "--master-port", str(_port())] + ARGS + ["--gpus", str(n)] + list(extra)
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    # the launcher's per-rank summary alone fills 3000 characters: keep enough to show the first rank's own message
    assert r.returncode == 0, r.stderr[-12000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def test_two_ranks_one_gpu_equals_single_process():
    one = _run(1, full=True)
    two = _run(2, full=True)
    assert two["config"]["parallelism"] == "pp2xdp1"
    assert two["ppl_random_weights"] == pytest.approx(one["ppl_random_weights"], rel=1e-9)
    # the N > 1 transports record on the CUDA path: torch p2p is the reference, the peer-copy transport must give the
    # same PPL, and RCCL - which refuses two ranks on one GPU (an error, or a blocked init) - is recorded as an error
    # entry without being attempted
    tr = two["transports"]
    assert tr["torch"]["ppl_random_weights"] > 1 and len(tr["torch"]["p2p"]) == 2
    assert tr["ipc"]["ppl_equal_torch"] is True and len(tr["ipc"]["p2p"]) == 2
    assert "ncclCommInitRank refuses" in tr["rccl"]["error"]
    assert "notebook_sweep" in one and one["notebook_sweep"]["windows_per_s"] > 0
    chk = _run(2, ["--no-graphs"], {"EDGE_P2P_CHECK": "1"})
    assert chk["ppl_random_weights"] == pytest.approx(one["ppl_random_weights"], rel=1e-9)


def test_plain_run_dumps_last_step_outputs(tmp_path):
    """``bench.py`` without ``--full`` on the HIP-graph path: the headline only, and ``--dump-outputs`` holds the last
    timed step's per-window NLL of every micro-batch (copies: the captured graph reuses its output buffer), whose
    token-weighted mean is the reported PPL when one step is timed."""
    import numpy as np
    from llm_inference_in_distributed_edge_networks_amd.eval.windows import sliding_windows
    cmd = ([sys.executable] + ARGS[:7] + ["--steps", "1", "--warmup", "1"] + ARGS[11:] +
           ["--dump-outputs", str(tmp_path)])
    r = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ), capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert j["steps"] == 1 and j["config"]["hip_graphs"] is True and j["ms_per_step"] > 0
    for k in ("value_bf16", "value_fp32_weights", "notebook_sweep", "same_node_reference_path", "box_calibration"):
        assert k not in j, k
    assert sorted(os.listdir(tmp_path)) == ["window_nll.npy"]
    a = np.load(tmp_path / "window_nll.npy")
    assert a.dtype in (np.float32, np.float64) and a.shape == (2, 4) and np.isfinite(a).all()
    assert not np.array_equal(a[0], a[1])
    # the timed step follows one warmup step of 2 micro-batches x 4 windows: it covers windows 8-15
    w = np.array([x.weight for x in sliding_windows(299_078, 256, 32)[8:16]], dtype=np.float64).reshape(2, 4)
    assert j["ppl_random_weights"] == pytest.approx(math.exp(float((a.astype(np.float64) * w).sum() / w.sum())),
                                                    rel=1e-9)


def test_self_launch_one_gpu_equals_single_process():
    """``bench.py --gpus 2`` with no launcher env spawns its two ranks itself (the path the driver takes if it runs
    ``bench.py --gpus N`` directly); same PPL as one process, n_gpus and the rank -> device map reported."""
    one = _run(1, ["--no-bf16", "--no-fp32-weights"])
    two = _run(2, ["--no-bf16", "--no-fp32-weights"], self_launch=True)
    assert two["n_gpus"] == 2 and two["launch"] == "self" and two["world_size"] == 2
    assert [d["device"] for d in two["rank_devices"]] == ["cuda:0", "cuda:0"]
    assert two["ppl_random_weights"] == pytest.approx(one["ppl_random_weights"], rel=1e-9)


def test_four_stage_pipeline_one_gpu_equals_local():
    """BASELINE config 4 shape (--pp 4): 4 ranks sharing cuda:0 == the 4 stages in one process (fp32 mode)."""
    one = _run(1, ["--pp", "4"])
    four = _run(4, ["--pp", "4"])
    assert four["config"]["parallelism"] == "pp4xdp1" and one["config"]["parallelism"] == "local-pp4"
    assert four["ppl_random_weights"] == pytest.approx(one["ppl_random_weights"], rel=1e-9)
    assert len(four["stages"]) == 4 and all("compute_ms" in s for s in four["stages"])


def test_four_stage_pipeline_poisoned_and_contended():
    """The round-5 one-off (4 ranks gave PPL 509.05 instead of 503.23 once) re-run under the two conditions that turn
    its candidate mechanisms into deterministic or frequent failures (docs/RESULTS.md section 2):

    * EDGE_POISON=2 (utils/poison.py): every torch.empty NaN-filled and LDS / registers poisoned before every kernel,
      so an uninitialised read gives NaN every time - the 4-rank and the 1-process run must still agree bit for bit;
    * a fifth process flooding the GPU with 2 GiB copies + fp16 GEMMs (tools/contention_check.py's hog) while the 4
      ranks run: a read that races its load (miscounted s_waitcnt) shows up as a different PPL."""
    extra = ["--pp", "4", "--no-bf16", "--no-fp32-weights"]
    one = _run(1, extra, {"EDGE_POISON": "2"})
    four = _run(4, extra, {"EDGE_POISON": "2"})
    assert math.isfinite(four["ppl_random_weights"]) and four["ppl_random_weights"] == one["ppl_random_weights"]
    hog = subprocess.Popen([sys.executable, os.path.join(ROOT, "tools", "contention_check.py"), "--hog-child",
                            "--hog-seconds", "90"], stdout=subprocess.PIPE, text=True)
    try:
        assert hog.stdout.readline().strip() == "hog running"
        plain = _run(1, extra)
        for _ in range(2):
            assert _run(4, extra)["ppl_random_weights"] == plain["ppl_random_weights"]
    finally:
        hog.terminate()
        hog.wait(timeout=60)


def test_deep_pipeline_secondary_one_gpu():
    """4 ranks sharing cuda:0 with the default parallelism: the headline pp2xdp2 plus the secondary measurement of
    the same step as one 4-stage pipeline (``value_pp4``, its stages, wire sizes and p2p probe; bench.deep_pipeline)
    on the CUDA path."""
    four = _run(4, ["--no-bf16", "--no-fp32-weights"])
    assert four["config"]["parallelism"] == "pp2xdp2"
    pp = four["pp4"]
    assert "error" not in pp and four["value_pp4"] > 0, pp
    assert pp["parallelism"] == "pp4xdp1" and len(pp["stages"]) == 4 and len(pp["p2p"]) == 6
    assert len(pp["wire_bytes_per_token"]) == 3 and all(w > 0 for w in pp["wire_bytes_per_token"])
    assert pp["ppl_random_weights"] > 1 and pp["wall_s"] > 0


def test_eight_ranks_one_gpu_headline_and_pp8():
    """The driver's 8-GPU shape rehearsed on one GPU: 8 ranks (gloo, host-staged p2p) run the pp2xdp4 headline and
    then the 8-stage secondary (one layer per stage on the 8-layer byte model), both through the CUDA-graph path."""
    r = _run(8, ["--model", "byte-qwen2", "--batch", "2", "--microbatches", "2", "--max-length", "128", "--split", "3",
                 "--no-bf16", "--no-fp32-weights"])
    assert r["config"]["parallelism"] == "pp2xdp4" and r["n_gpus"] == 8
    pp = r["pp8"]
    assert "error" not in pp and r["value_pp8"] > 0, pp
    assert pp["parallelism"] == "pp8xdp1" and len(pp["stages"]) == 8 and len(pp["wire_bytes_per_token"]) == 7


def test_serialized_kernel_mode_same_result():
    """SURVEY §5.2 race check: with every kernel serialised (AMD_SERIALIZE_KERNEL=3, HIP_LAUNCH_BLOCKING=1) the
    2-rank pipeline gives bit-identical PPL to the normal asynchronous run - no result depends on stream overlap."""
    fast = _run(2, ["--no-bf16"])
    ser = _run(2, ["--no-bf16", "--no-graphs"], {"AMD_SERIALIZE_KERNEL": "3", "HIP_LAUNCH_BLOCKING": "1"})
    assert ser["ppl_random_weights"] == fast["ppl_random_weights"]


def test_peer_copy_transport_one_gpu():
    """--transport ipc: boundary messages copied by the sender straight into the receiver's IPC-mapped slot ring
    (CUDA IPC between the two processes; flags / credits over gloo here) == the single-process run."""
    one = _run(1, ["--no-bf16"])
    ipc = _run(2, ["--no-bf16", "--transport", "ipc"])
    assert ipc["config"]["transport"] == "ipc"
    assert ipc["ppl_random_weights"] == pytest.approx(one["ppl_random_weights"], rel=1e-9)
    three = _run(3, ["--no-bf16", "--transport", "ipc", "--pp", "3"], {"EDGE_IPC_SLOT_BYTES": str(1 << 16)})
    one3 = _run(1, ["--no-bf16", "--pp", "3"])
    assert three["ppl_random_weights"] == pytest.approx(one3["ppl_random_weights"], rel=1e-9)
