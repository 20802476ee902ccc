"""CPU suite, part 3: the C ABI library loads and exports every symbol include/vorbis_amd.h
declares; host-side validation of setup blobs; the product never falls back to a CPU path; the
N>1 sharding/broadcast logic over gloo with world_size 2."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import checker
from tests.feed_cases import ABI, LIB

ROOT = checker.ROOT


def declared_symbols():
    src = open(os.path.join(ROOT, "include", "vorbis_amd.h")).read()
    return sorted(set(re.findall(r"^(?:int|void|long|const char \*|vamd_ctx \*)\s*(vamd_[a-z0-9_]+)\s*\(", src, re.M)))


def test_header_symbols_are_exported():
    assert os.path.exists(LIB), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    L = C.CDLL(LIB)
    syms = declared_symbols()
    assert len(syms) >= 12
    for s in syms:
        assert hasattr(L, s), "missing export: " + s
    import vorbis_amd
    assert sorted(vorbis_amd.EXPORTED_SYMBOLS) == syms


def test_create_rejects_bad_blobs_without_touching_the_gpu():
    """Blob validation happens before any HIP call, so the error paths are testable here."""
    L = C.CDLL(LIB)
    L.vamd_create_abi.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_size_t, C.c_int, C.c_int]
    h = C.c_void_p()
    good = np.fromfile(os.path.join(ROOT, "vorbis_amd", "data", "setup_44k_stereo_q4.bin"), dtype=np.uint8)
    assert L.vamd_create_abi(C.byref(h), None, 0, -1, ABI) == -131                       # OV_EINVAL
    bad = good.copy(); bad[0] ^= 0xff
    assert L.vamd_create_abi(C.byref(h), bad.ctypes.data_as(C.c_void_p), bad.size, -1, ABI) == -131
    ver = good.copy(); ver[8] = 99
    assert L.vamd_create_abi(C.byref(h), ver.ctypes.data_as(C.c_void_p), ver.size, -1, ABI) == -134  # OV_EVERSION
    trunc = good[:1000].copy()
    assert L.vamd_create_abi(C.byref(h), trunc.ctypes.data_as(C.c_void_p), trunc.size, -1, ABI) == -131
    chs = good.copy(); chs[16:20] = np.frombuffer(np.int32(9).tobytes(), np.uint8)   # beyond VAMD_MAX_CH
    assert L.vamd_create_abi(C.byref(h), chs.ctypes.data_as(C.c_void_p), chs.size, -1, ABI) == -130   # OV_EIMPL
    # a caller built against another release of the header (its structs may be shorter than what the library reads) is
    # refused before anything else is looked at -- and there is no un-versioned vamd_create symbol to slip through
    assert L.vamd_create_abi(C.byref(h), good.ctypes.data_as(C.c_void_p), good.size, -1, ABI - 1) == -134  # OV_EVERSION
    assert not hasattr(L, "vamd_create")
    assert not h.value


def _header_layout():
    """Byte offsets inside vamd_setup_header, read off the C header with a tiny compiled probe (no hand-kept copy)."""
    import tempfile
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "vamd_setup.h"
int main(void) {
  printf("total_bytes %zu\nxform0_off_trig %zu\nxform1_off_bitrev %zu\nxform1_log2n %zu\npsy2_off_octave %zu\npsy2_off_bark %zu\n"
         "floor1_hineighbor %zu\nfloor1_postlist %zu\nres1_end %zu\n",
         offsetof(vamd_setup_header, total_bytes), offsetof(vamd_setup_header, xform[0].off_mdct_trig),
         offsetof(vamd_setup_header, xform[1].off_mdct_bitrev), offsetof(vamd_setup_header, xform[1].log2n),
         offsetof(vamd_setup_header, psy[2].off_octave), offsetof(vamd_setup_header, psy[2].off_bark),
         offsetof(vamd_setup_header, mode[1].floor[0].hineighbor), offsetof(vamd_setup_header, mode[1].floor[0].postlist),
         offsetof(vamd_setup_header, res[1][0].end));
  return 0;
}'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), os.path.join(d, "p.c"), "-o", os.path.join(d, "p")])
        out = subprocess.check_output([os.path.join(d, "p")], text=True)
    return {ln.split()[0]: int(ln.split()[1]) for ln in out.splitlines()}


def test_create_rejects_truncated_stale_and_corrupt_tables():
    """Every table a kernel walks or indexes through is bounds- and range-checked at vamd_create(): a truncated,
    stale or bit-flipped blob comes back as OV_EINVAL instead of reading out of bounds on the device."""
    L = C.CDLL(LIB)
    L.vamd_create_abi.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_size_t, C.c_int, C.c_int]
    h = C.c_void_p()
    good = np.fromfile(os.path.join(ROOT, "vorbis_amd", "data", "setup_44k_stereo_q4.bin"), dtype=np.uint8)
    off = _header_layout()

    def create(b):
        return L.vamd_create_abi(C.byref(h), b.ctypes.data_as(C.c_void_p), b.size, -1, ABI)

    def put32(b, at, v):
        b[at:at + 4] = np.frombuffer(np.int32(v).tobytes(), np.uint8)

    def get32(b, at):
        return int(np.frombuffer(b[at:at + 4].tobytes(), np.int32)[0])

    # truncated behind the header: total_bytes still claims the full size
    assert create(good[:good.size // 2].copy()) == -131
    # total_bytes smaller than the header itself
    b = good.copy(); put32(b, off["total_bytes"], 64)
    assert create(b) == -131
    # transform tables pointing past the end / log2n not matching n
    b = good.copy(); put32(b, off["xform0_off_trig"], good.size - 16)
    assert create(b) == -131
    b = good.copy(); put32(b, off["xform1_log2n"], 10)
    assert create(b) == -131
    # a bit-reverse entry that would gather outside the MDCT work vector
    b = good.copy(); put32(b, get32(good, off["xform1_off_bitrev"]) + 12, 5000)
    assert create(b) == -131
    # octave[] outside the seed vector, bark[] window beyond the block
    b = good.copy(); put32(b, get32(good, off["psy2_off_octave"]) + 4 * 700, 1 << 20)
    assert create(b) == -131
    b = good.copy(); put32(b, get32(good, off["psy2_off_bark"]) + 4 * 100, (5 << 16) | 60000)
    assert create(b) == -131
    # floor: a neighbour index that is not an earlier post, a post beyond the fit range
    b = good.copy(); put32(b, off["floor1_hineighbor"] + 4 * 3, 40)
    assert create(b) == -131
    b = good.copy(); put32(b, off["floor1_postlist"] + 4 * 5, 99999)
    assert create(b) == -131
    # residue range beyond the interleaved bundle
    b = good.copy(); put32(b, off["res1_end"], 1 << 20)
    assert create(b) == -131
    # ... and random single-byte corruption never crashes the host-side validation
    rng = np.random.default_rng(5)
    for _ in range(300):
        b = good.copy()
        b[rng.integers(0, 6000)] ^= 1 << rng.integers(0, 8)      # somewhere in the header's tables
        r = create(b)                                            # a flip in a value nothing indexes through may pass:
        assert r in (0, -131, -130, -134, -129)                  # then it is a context (GPU box) or EFAULT (no GPU)
        if r == 0:
            L.vamd_destroy.argtypes = [C.c_void_p]
            L.vamd_destroy(h)
            h = C.c_void_p()
    assert not h.value


def test_no_cpu_fallback():
    """Without a GPU the product raises; it must never quietly compute on the host."""
    import torch
    import vorbis_amd
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(RuntimeError):
        vorbis_amd.Analyzer(vorbis_amd.default_setup_blob())
    # and nothing under vorbis_amd/ imports the oracle or the test build
    for dirpath, _, files in os.walk(os.path.join(ROOT, "vorbis_amd")):
        for f in files:
            if f.endswith((".py", ".h", ".hip", ".c", ".cpp")):
                text = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in text.replace("the oracle", "").replace("oracle/", "ORACLEPATH/") or \
                    "import oracle" not in text and "from oracle" not in text, f
                assert "from oracle" not in text and "import oracle" not in text and "tests.emul" not in text, f


def test_derived_tables_match_reference_walks():
    """vamd_derive.h freezes data-independent loops; check them against a direct python replay."""
    from tests.emul.emul import Emul
    blob = np.fromfile(os.path.join(ROOT, "vorbis_amd", "data", "setup_44k_stereo_q4.bin"), dtype=np.uint8)
    Emul(blob)  # build_image + derive run inside emul_open; golden/oracle tests cover the values


WORKER = r"""
import os, sys
sys.path.insert(0, %(root)r)
import numpy as np, torch, torch.distributed as dist
from vorbis_amd import sharding
rank, world, dev = sharding.init_from_env("gloo", use_cuda=False)
blob = np.fromfile(os.path.join(%(root)r, "vorbis_amd", "data", "setup_44k_stereo_q4.bin"), dtype=np.uint8)
got = sharding.broadcast_blob(blob if rank == 0 else None, dev)
assert np.array_equal(got, blob)
total = 1000003
lo, hi = sharding.shard_range(total, rank, world)
assert sharding.sum_over_ranks(hi - lo, dev) == total
edges = [torch.zeros(2, dtype=torch.int64) for _ in range(world)]
dist.all_gather(edges, torch.tensor([lo, hi], dtype=torch.int64))
for a, b in zip(edges[:-1], edges[1:]):
    assert int(a[1]) == int(b[0])
assert int(edges[0][0]) == 0 and int(edges[-1][1]) == total
assert sharding.max_over_ranks(1.0 + rank, dev) == float(world)
sharding.finish()
print("rank", rank, "ok")
"""


def _torchrun(script, port, timeout=300):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    return subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                           "--master-addr", "127.0.0.1", "--master-port", str(port), str(script)],
                          env=env, capture_output=True, text=True, timeout=timeout)


def test_two_rank_sharding_and_table_broadcast_gloo(tmp_path):
    """vorbis_amd/sharding.py -- the module bench.py runs on -- over gloo with two ranks."""
    script = tmp_path / "worker.py"
    script.write_text(WORKER % {"root": ROOT})
    r = _torchrun(script, 29617)
    assert r.returncode == 0, r.stdout + r.stderr


# bench.main()'s own distributed branch (process group from the environment, blob broadcast, barriers around the
# timed region, max-over-ranks, the parity sample's sums, JSON assembly on rank 0) with only the GPU work replaced:
# the stub runner lives HERE, bench.py has no dry-run path of its own.
BENCH_WORKER = r"""
import sys
sys.path.insert(0, @ROOT@)
import bench
from tests.stub_runner import StubRunner
rc = bench.main(["--gpus", "2", "--steps", "5", "--warmup", "1", "--backend", "gloo", "--blocks", "1000", "--full"], make_runner=StubRunner)
sys.exit(rc)
"""


def test_bench_distributed_branch_runs_under_gloo(tmp_path):
    script = tmp_path / "bench_worker.py"
    script.write_text(BENCH_WORKER.replace("@ROOT@", repr(ROOT)))
    r = _torchrun(script, 29619)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout          # rank 0 alone prints, one line
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["steps"] == 5 and line["scaling"] == "weak"
    assert line["config"]["blocks_per_gpu"] == 1000
    assert line["ms_per_step"] >= 19.0        # the slow rank sleeps 20 ms per step: max over ranks, not rank 0's 10 ms
    assert abs(line["value"] - 2 * 1000 * 5 / (line["ms_per_step"] * 5e-3)) < 1e-6 * line["value"]
    assert line["parity_sample"] == {"blocks": 256, "mismatches": 0, "checker": "stub",
                                     "compared": line["parity_sample"]["compared"]}
    assert "roofline" in line and line["roofline"]["kernels_ms_per_step"] == {"transform": 1.0, "noisemask": 2.0}


def _check_rehearsal_line(stdout):
    lines = [ln for ln in stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, stdout          # rank 0 alone prints, one line
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["world"] == 2 and line["rccl_ranks_seen"] == 2 and line["backend"] == "gloo"
    assert line["config"]["blocks_per_gpu"] == 1000
    assert line["ms_per_step"] >= 19.0
    return line


def test_bench_gpus_flag_launches_the_ranks_itself():
    """`python bench.py --gpus 2` as a plain command, no launcher and no WORLD_SIZE around it: bench.py starts the two
    ranks itself (the flag used to be parsed and ignored).  gloo and a stub runner, since this box has no
    GPU; everything else -- the spawn, the rendezvous, the broadcast, the reductions, the line -- is the shipped code."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--steps", "5",
                        "--warmup", "1", "--blocks", "1000", "--runner", "tests.stub_runner:StubRunner"],
                       env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    line = _check_rehearsal_line(r.stdout)
    assert line["runner"] == "tests.stub_runner:StubRunner"     # a rehearsal says that it is one


def test_bench_plain_run_is_lean_and_dumps_its_outputs(tmp_path):
    """A plain run times exactly --steps steps and prints the headline alone (the checks and the other figures are --full's);
    --dump-outputs writes the last step's outputs as float32 / float64 .npy files, a fixed sample when they would pass the
    budget, the same files on every run."""
    import numpy as np
    dumps = []
    for k in range(2):
        d = tmp_path / ("d%d" % k)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                            "--blocks", "8000", "--runner", "tests.stub_runner:StubRunner", "--dump-outputs", str(d)],
                           capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert r.returncode == 0, r.stdout + r.stderr
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, r.stdout
        line = json.loads(lines[0])
        assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] >= 9.0
        assert {"metric", "value", "unit", "higher_is_better", "dtype", "roofline"} <= set(line)
        assert not {"parity_sample", "cpu_baseline", "workloads", "host_fed", "neighbours", "shader_clock"} & set(line)
        dumps.append({f.name: np.load(f) for f in sorted(d.iterdir())})
    assert set(dumps[0]) == {"mdct.npy", "posts.npy", "sample_index.npy"}
    assert dumps[0]["mdct.npy"].dtype == np.float32 and dumps[0]["posts.npy"].dtype == np.float64
    assert sum(x.nbytes for x in dumps[0].values()) <= 64 << 20
    n = len(dumps[0]["sample_index.npy"])
    assert 0 < n < 8000 and dumps[0]["mdct.npy"].shape == (n, 2, 1024)
    for name, x in dumps[0].items():
        assert np.array_equal(x, dumps[1][name]), name


def test_bench_gpus_flag_must_agree_with_the_launcher():
    """--gpus 4 inside a world of 2 is a contradiction, not a run: exit code 2, no line."""
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29655")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--backend", "gloo",
                        "--runner", "tests.stub_runner:StubRunner"], env=env, capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 2 and "WORLD_SIZE" in r.stderr and not r.stdout.strip()


def test_abi_version_matches_the_header():
    """vamd_abi_version() is the VAMD_ABI_VERSION of the header the library was built from (a caller built against another
    header finds out before it hands over a struct the library reads further than the caller wrote)."""
    import re
    import vorbis_amd
    L = vorbis_amd.load_library()
    hdr = open(os.path.join(ROOT, "include", "vorbis_amd.h")).read()
    want = int(re.search(r"#define VAMD_ABI_VERSION (\d+)", hdr).group(1))
    L.vamd_abi_version.restype = C.c_int
    assert L.vamd_abi_version() == want
    assert "VAMD_EDOMAIN" in hdr and vorbis_amd.VAMD_EDOMAIN == int(re.search(r"#define VAMD_EDOMAIN\s+\((-\d+)\)", hdr).group(1))
    assert vorbis_amd.VAMD_ENONFINITE == int(re.search(r"#define VAMD_ENONFINITE\s+\((-\d+)\)", hdr).group(1))
    from vorbis_amd import api
    assert api.ABI_VERSION == want      # the ctypes mirror was written against this header
    assert api.STATUS_RANGE == int(re.search(r"#define VAMD_STATUS_RANGE\s+(\d+)", hdr).group(1))
    assert api.STATUS_NONFINITE == int(re.search(r"#define VAMD_STATUS_NONFINITE\s+(\d+)", hdr).group(1))


def test_bench_rooflines_read_the_committed_profiles():
    """bench.py's traffic and vector-issue figures come from the committed counter passes and are withheld when the sources
    have changed since (source hash).  At a commit whose profiles were regenerated they must load, scale with the unit count
    and stay inside what they describe; a stale profile must say so instead of reporting a number."""
    import bench
    stage_ms = {"transform": 1.47, "noisemask": 2.49, "tonemask": 0.46, "floor": 1.93, "couple": 0.47}
    v = bench.measured_valu("c4", 131072, stage_ms)
    traffic, per, note = bench.measured_traffic("c4", 131072)
    prof = json.load(open(os.path.join(ROOT, bench.VALU_PROFILE)))
    if prof["source_hash"] != bench.source_hash():       # (between a kernel edit and the next profiling run)
        assert v["value"] is None and "re-run" in v["note"] and traffic is None
        return
    assert 20000 < v["valu_insts_per_unit"] < 32000 and 2.6 < v["cycles_per_inst"] < 4.8
    assert abs(v["issue_ms_per_step"] - sum(d["issue_ms"] for d in v["per_stage"].values())) < 1e-9
    assert 0.3 < v["frac_valu"] < 1.2 and 0.5 < v["per_stage"]["floor"]["frac_valu"] < 1.3
    half = bench.measured_valu("c4", 65536, {k: x / 2 for k, x in stage_ms.items()})
    assert abs(half["issue_ms_per_step"] * 2 - v["issue_ms_per_step"]) < 1e-9
    assert 100e3 * 131072 < traffic < 200e3 * 131072 and set(per) >= {"k_floor", "k_noise", "k_transform", "k_couple"}
    assert bench.measured_valu("c2", 65536, {"mdct_forward": 0.2}) is None
    seen, aff, quota = bench.host_cpus()
    assert seen >= 1 and 1 <= aff <= seen and (quota is None or quota > 0)
