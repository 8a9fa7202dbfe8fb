"""Host logic of bench.py that needs no GPU: the configs[4] flag and the self-launch of `--gpus N`."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import bench


def test_config5_is_deepfm_with_one_100m_row_table():
    a = bench.parse_args(["--config5", "--gpus", "8"])
    assert a.model == "deepfm" and a.big_table_rows == 100_000_000 and a.batch == 4096 and a.gpus == 8
    a = bench.parse_args(["--config5", "--big-table-rows", "5000000"])
    assert a.big_table_rows == 5_000_000


def test_self_launch_refuses_more_gpus_than_present(monkeypatch):
    monkeypatch.delenv("RECALGO_DIST_BACKEND", raising=False)
    monkeypatch.setattr(bench.torch.cuda, "device_count", lambda: 1)
    monkeypatch.setattr(subprocess, "run", lambda *a, **k: pytest.fail("must not launch"))
    with pytest.raises(SystemExit) as e:
        bench.self_launch(bench.parse_args(["--gpus", "8"]))
    assert "refusing" in str(e.value)


def test_self_launch_command(monkeypatch):
    """One rank per GPU under torch.distributed.run, rendezvous on 127.0.0.1, the user's own flags passed through."""
    seen = {}
    monkeypatch.setattr(bench.torch.cuda, "device_count", lambda: 8)
    monkeypatch.setattr(subprocess, "run", lambda cmd, env: seen.update(cmd=cmd, env=env) or SimpleNamespace(returncode=3))
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "7", "--config5"])
    assert bench.self_launch(bench.parse_args(["--gpus", "4", "--steps", "7", "--config5"])) == 3     # the launcher's status
    cmd = seen["cmd"]
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"] and "--nproc-per-node=4" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and int(cmd[cmd.index("--master-port") + 1]) > 0
    i = cmd.index(os.path.abspath(bench.__file__))
    assert cmd[i + 1:] == ["--gpus", "4", "--steps", "7", "--config5"]
    assert seen["env"]["MASTER_ADDR"] == "127.0.0.1" and seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_in_step_table_reads_the_newest_committed_kernel_stats(tmp_path, monkeypatch):
    """bench.in_step_table: the `in_step` object of the bench line is the committed rocprofv3 summary of the same command —
    calls per step from the optimizer launch's call count, kernels that do not run every step left out."""
    import bench
    prof = tmp_path / "profiles"
    prof.mkdir()
    (prof / "r01a_dcn_kernel_stats.md").write_text("| `old_kernel(x)` | 10 | 10 | 1 | 1 | 1 | 1 |\n")
    (prof / "r02b_dcn_kernel_stats.md").write_text(
        "source: x\n\n| kernel | calls | total_ns | avg_ns | min_ns | max_ns | % |\n|---|---:|---:|---:|---:|---:|---:|\n"
        "| `void (anonymous namespace)::dense_bwd_kernel<true, true>((anonymous namespace)::DgradArgs)` | 300 | 7500000 | 25000 | 1 | 2 | 50 |\n"
        "| `(anonymous namespace)::adam_tf1_step_kernel((anonymous namespace)::AdamStepArgs)` | 100 | 600000 | 6000 | 1 | 2 | 10 |\n"
        "| `void at::native::reduce_kernel<512>(int)` | 1 | 260000 | 260000 | 1 | 2 | 1 |\n"
        "\nper launch shape (kernel, grid size):\n\n| `(anonymous namespace)::adam_tf1_step_kernel(x)` | 512 | 100 | 6000 | 1 | 2 |\n")
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    t = bench.in_step_table("dcn")
    assert t["source"] == "profiles/r02b_dcn_kernel_stats.md" and t["steps_profiled"] == 100
    assert [(k["kernel"], k["calls_per_step"], k["avg_us"]) for k in t["kernels"]] == [
        ("dense_bwd_kernel<true, true>", 3.0, 25.0), ("adam_tf1_step_kernel", 1.0, 6.0)]
    assert t["dispatches_per_step"] == 4.0 and t["kernel_us_per_step"] == 81.0
    assert bench.in_step_table("din") is None


def test_host_fed_leg_is_bounded_and_optional(monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--no-host-fed"])
    assert bench.parse_args().no_host_fed
    monkeypatch.setattr(sys, "argv", ["bench.py"])
    assert not bench.parse_args().no_host_fed


def test_full_is_off_by_default_and_dump_outputs_parses():
    a = bench.parse_args(["--gpus", "1", "--steps", "5", "--warmup", "2"])
    assert not a.full and a.dump_outputs is None and a.steps == 5 and a.warmup == 2
    a = bench.parse_args(["--full", "--dump-outputs", "out_dir"])
    assert a.full and a.dump_outputs == "out_dir"


def test_dump_outputs_writes_the_loss_and_a_bounded_seeded_sample_of_the_variables(tmp_path, monkeypatch):
    """--dump-outputs: every variable as <name>.npy in float32 / float64 (names with '/' -> '.'), the loss as float64;
    an array over its share of the limit as its first rows + a sample of the others seeded by its name (identical from run
    to run), everything within the limit."""
    g = torch.Generator().manual_seed(0)
    arrays = {"emb/table_a/embedding_weights": torch.randn(50_000, 16, generator=g),
              "dense/kernel": torch.randn(64, 32, generator=g), "step": torch.tensor([7], dtype=torch.int64)}
    seen = []
    est = SimpleNamespace(store=SimpleNamespace(named_arrays=lambda gather=False: seen.append(gather) or dict(arrays)))
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 1 << 20)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), est, 0.6931, 1, 0)
    assert seen == [False, False]
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["dense.kernel.npy", "emb.table_a.embedding_weights.npy", "loss.npy", "step.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= (1 << 20) + 4096
    assert np.load(tmp_path / "a" / "loss.npy").dtype == np.float64 and float(np.load(tmp_path / "a" / "loss.npy")[0]) == 0.6931
    assert np.load(tmp_path / "a" / "step.npy").dtype == np.float64
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "dense.kernel.npy"), arrays["dense/kernel"].numpy())
    t = np.load(tmp_path / "a" / "emb.table_a.embedding_weights.npy")
    assert t.dtype == np.float32 and t.shape[1] == 16 and 1000 < t.shape[0] < 50_000
    head = t.shape[0] // 2
    np.testing.assert_array_equal(t[:head], arrays["emb/table_a/embedding_weights"][:head].numpy())
    np.testing.assert_array_equal(t, np.load(tmp_path / "b" / "emb.table_a.embedding_weights.npy"))
    full = arrays["emb/table_a/embedding_weights"].numpy()
    assert all((full[head:] == row).all(axis=1).any() for row in t[head:head + 20])     # sampled rows are rows of the table
    bench.dump_outputs(str(tmp_path / "c"), est, 0.5, 2, 1)          # N > 1: every rank gathers, rank 0 alone writes
    assert seen[-1] is True and not os.path.exists(tmp_path / "c")
