"""GPU test of bench.py's multi-rank path with the HIP library (not the CPU oracle): two ranks, started by bench.py itself because no
launcher set WORLD_SIZE, share the one visible GPU (--force-device 0) and talk over gloo; ONE read set dealt i mod 2 must reduce to
the per-sequence counts and the NAR histogram of a single-rank run of the whole set, and the weak / strong scaling lines must be there.
(On a multi-GPU node the same code runs with the RCCL backend, one rank per device.)  Those legs belong to `--full`; a plain run is
the headline alone, with the same clock and the same records."""
import json
import os
import subprocess
import sys

import pytest

import helpers

pytestmark = pytest.mark.gpu


def test_two_ranks_shard_one_read_set_like_a_single_rank():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(helpers.ROOT, "bench.py"), "--full", "--gpus", "2", "--force-device", "0", "--dist-backend", "gloo",
           "--genome-mbp", "30", "--reads", "400000", "--steps", "1", "--warmup", "1", "--cpu-baseline-secs", "0",
           "--stream-batch", "100000", "--shard-check-reads", "300000", "--no-live-traffic"]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    d = json.loads(line)
    assert d["n_gpus"] == 2 and d["scaling"] == "weak" and d["value"] > 0
    sc = d["shard_check"]
    assert sc["per_sequence_counts_equal_1gpu_run"] and sc["nar_histogram_equal_1gpu_run"] and sc["accepted"] > 0
    assert d["strong_scaling"]["reads_total_per_step"] == 400000 and d["strong_scaling"]["value"] > 0
    assert d["t_align_host_resident"]["results_bit_identical_to_kernel_only_steps"]
    # `value` is the host-in / host-out clock (SURVEY 8d T_align), the kernel-only rate stands beside it
    assert d["value"] == d["t_align_host_resident"]["value"] and d["value_kernel_only"] > 0 and "host memory" in d["value_clock"]
    # (the layout `biokanga align` picks for C2's 50 M reads per device: the partial window array)
    assert d["config"]["window_array"].startswith("partial") and d["roofline"]["window_array"] == "partial"


MOVED_BEHIND_FULL = ("roofline", "layouts", "cpu_baseline", "value_no_window_array", "value_window_array", "value_window_array_full",
                     "shard_check", "strong_scaling")


def _one_rank(tmp_path, name, extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    dump = str(tmp_path / name)
    cmd = [sys.executable, os.path.join(helpers.ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--genome-mbp", "30",
           "--reads", "400000", "--stream-batch", "100000", "--dump-outputs", dump] + extra
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines                          # ONE line on stdout
    return json.loads(lines[0]), dump, r.stderr


def test_plain_run_is_the_headline_alone_and_full_adds_the_rest(tmp_path):
    """a plain run: the host-in / host-out clock only - no kernel-only steps, no other layout or image, no counter passes, no CPU
    baseline; --full: all of them, in the same line.  Both dump the same records of the same reads."""
    import numpy as np
    d, dump, err = _one_rank(tmp_path, "plain", [])
    assert d["full"] is False and d["value"] > 0 and d["unit"] == "reads/s" and d["higher_is_better"] is True and d["dtype"] == "u8"
    assert d["metric"].startswith("aligned reads/s") and d["steps"] == 2 and d["warmup"] == 1
    h = d["t_align_host_resident"]
    assert d["value"] == h["value"] and d["ms_per_step"] == h["ms_per_step"] and "host memory" in d["value_clock"]
    assert abs(d["value"] - 400000 * 2 / (d["ms_per_step"] * 2e-3)) <= 1e-6 * d["value"]
    assert not [k for k in MOVED_BEHIND_FULL + ("value_kernel_only",) if k in d]
    assert "other" not in d["index_image"] and "library_binding_one_device" not in d["rccl"]
    assert "live traffic" not in err and "cpu_baseline" not in err
    assert d["config"]["window_array"].startswith("partial") and 0 < d["config"]["accepted_frac_rank0"] <= 1
    assert d["dump_outputs"]["path"] == "host-in / host-out" and d["dump_outputs"]["reads_sampled"] == 400000

    f, dump_full, _ = _one_rank(tmp_path, "full", ["--full", "--cpu-baseline-secs", "3", "--reference-reads", "0", "--no-live-traffic"])
    assert f["full"] is True and f["value"] == f["t_align_host_resident"]["value"] and f["value_kernel_only"] > 0
    assert f["t_align_host_resident"]["results_bit_identical_to_kernel_only_steps"] and f["config"]["results_bitwise_equal_across_steps"]
    assert f["roofline"]["window_array"] == "partial" and f["layouts"]["results_bit_identical_between_layouts"]
    assert f["index_image"]["other"]["results_bit_identical_to_the_headline_image"]
    assert f["rccl"]["library_binding_one_device"]["counts_equal_plain_path"]
    assert f["cpu_baseline"]["kind"] == "port" and f["cpu_baseline"]["parity_mismatching_fields_vs_gpu"] == 0
    assert {k: v for k, v in f["config"].items() if k in d["config"]} == d["config"]
    assert sorted(os.listdir(dump)) == sorted(os.listdir(dump_full)) == sorted(a + ".npy" for a in d["dump_outputs"]["arrays"])
    for a in os.listdir(dump):
        assert np.array_equal(np.load(os.path.join(dump, a)), np.load(os.path.join(dump_full, a))), a


def test_rank_count_mismatch_is_refused():
    """a launcher that started fewer ranks than --gpus asks for must not yield an N-GPU line"""
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(helpers.ROOT, "bench.py"), "--gpus", "2", "--genome-mbp", "30", "--reads", "1000"],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode != 0 and "refusing" in r.stderr
    assert not [l for l in r.stdout.splitlines() if l.startswith("{")]
