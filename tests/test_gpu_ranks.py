"""GPU suite: the multi-rank bench on REAL kernels (VERDICT r04 missing 4 / next 6).  No box this project has seen holds
more than one GPU, and RCCL has therefore never run; what can run is everything else of the N-rank path: two processes,
launched by bench.py itself, each with the real GpuRunner on cuda:0 (--share-gpu), joined over gloo -- the setup blob
broadcast, per-rank seeds and shard ranges, the barrier-bracketed timed region with its max over ranks, a parity sample
per rank against the reference, the all-reduced counts and rank 0's one aggregated line.  It proves everything except
RCCL itself and DeviceGuard across devices (DESIGN section 7 says exactly that)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = [pytest.mark.gpu]


def _bench(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(args), env=env, capture_output=True, text=True,
                       timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout          # rank 0 alone prints, one line
    return json.loads(lines[0])


@pytest.mark.skipif(not ref.available(), reason="oracle/_ref not built (the per-rank parity sample needs it)")
def test_two_ranks_of_the_real_runner_on_one_gpu():
    common = ("--steps", "20", "--warmup", "3", "--blocks", "65536", "--full", "--no-cpu-baseline", "--no-neighbours", "--no-workloads")
    one = _bench("--gpus", "1", *common)
    two = _bench("--gpus", "2", "--backend", "gloo", "--share-gpu", *common)
    assert two["n_gpus"] == 2 and two["world"] == 2 and two["rccl_ranks_seen"] == 2 and two["backend"] == "gloo"
    assert two["share_gpu"] is True and two["collectives_on"] in ("device", "host") and "runner" not in two
    assert two["config"]["blocks_per_gpu"] == 65536 and one["config"]["blocks_per_gpu"] == 65536
    # every rank checked its own sample of its own shard against the reference: 128 + 128 units, none differing
    assert two["parity_sample"]["blocks"] == 256 and two["parity_sample"]["mismatches"] == 0
    assert two["parity_sample"]["checker"] == "reference"
    # two ranks share the one chip: the aggregate is about what one GPU does (twice the job in about twice the time; the
    # two processes overlap each other's launch gaps, so somewhat more)
    assert 0.5 * one["value"] < two["value"] < 1.6 * one["value"], (one["value"], two["value"])
    assert two["roofline"]["kernels_ms_per_step"]["noisemask"] > 0


@pytest.mark.skipif(not ref.available(), reason="oracle/_ref not built")
def test_two_ranks_default_line_carries_c5_host_fed_and_cpu_baseline():
    """The line a first multi-GPU run will print: with more than one rank the default run
    still yields C5, the host-fed figure and the CPU baseline (rank 0) -- rehearsed with two ranks on one GPU at reduced
    stream counts."""
    two = _bench("--gpus", "2", "--backend", "gloo", "--share-gpu", "--full", "--steps", "3", "--warmup", "1", "--streams", "48",
                 "--feed-streams", "16", "--feed-groups", "6", "--feed-lanes", "2", "--cpu-seconds", "2", "--no-neighbours")
    assert two["n_gpus"] == 2 and two["share_gpu"] is True
    c5 = two["workloads"]["c5"]
    assert "error" not in c5 and c5["parity_sample"]["mismatches"] == 0 and c5["value"] > 0
    assert set(two["workloads"]) == {"c5"}                     # (c2 / c3 are single-GPU lines)
    hf = two["host_fed"]["c4"]
    assert "error" not in hf and hf["n_gpus"] == 2 and hf["value"] > 0 and hf["parity_sample"]["mismatches"] == 0
    assert two["cpu_baseline"]["value"] > 0 and two["cpu_baseline"]["kind"] == "reference"
    # frac reproduces from the line's own figures
    for d in (two, c5):
        r = d["roofline"]
        assert abs(r["alg_bytes_per_step"] / (d["ms_per_step"] * 1e-3) / 1e9 / r["peak"] - r["frac"]) < 0.01 * r["frac"]


def test_plain_run_dumps_the_same_outputs_every_run(tmp_path):
    """--dump-outputs on the real kernels: the timed path's outputs of its last step, float32 / float64 only, within 64 MB,
    and the same arrays from a second run (the inputs are seeded); the mixed-size workload dumps both size classes."""
    common = ("--gpus", "1", "--steps", "2", "--warmup", "1", "--blocks", "4096")
    runs = []
    for k in range(2):
        line = _bench(*common, "--dump-outputs", str(tmp_path / ("c4_%d" % k)))
        assert "parity_sample" not in line and line["steps"] == 2
        runs.append({f.name: np.load(f) for f in sorted((tmp_path / ("c4_%d" % k)).iterdir())})
    assert {"mdct.npy", "logmask.npy", "posts.npy", "iwork.npy", "ampmax_out.npy"} <= set(runs[0])
    assert all(x.dtype in (np.float32, np.float64) for x in runs[0].values())
    assert sum(x.nbytes for x in runs[0].values()) <= 64 << 20
    for name, x in runs[0].items():
        assert np.array_equal(x, runs[1][name], equal_nan=True), name
    _bench("--gpus", "1", "--workload", "c5", "--streams", "32", "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path / "c5"))
    c5 = {f.name for f in (tmp_path / "c5").iterdir()}
    assert {"ampmax_state.npy", "stream_start.npy", "short_mdct.npy", "long_mdct.npy", "long_blocktype.npy"} <= c5
