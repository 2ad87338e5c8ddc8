"""bench.py's launch contract, checked without a GPU: `--gpus N` with no rank environment must start N ranks as
child processes of `torch.distributed.run` (never re-exec a process that touched the GPU)."""
import importlib.util
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load_bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_self_launch_command(monkeypatch):
    bench = _load_bench()
    seen = {}

    def fake_run(cmd, env=None, **kw):
        seen["cmd"], seen["env"] = cmd, env
        return types.SimpleNamespace(returncode=7)

    monkeypatch.setattr(bench.subprocess, "run", fake_run)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "5", "--warmup", "1"])
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    args = bench.parse_args()
    assert bench.self_launch(args) == 7                      # the children's exit code is passed through
    cmd = seen["cmd"]
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nproc-per-node=4" in cmd and "--nnodes=1" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert 0 < int(cmd[cmd.index("--master-port") + 1]) < 65536
    i = cmd.index(os.path.join(ROOT, "bench.py"))
    assert cmd[i + 1:] == ["--gpus", "4", "--steps", "5", "--warmup", "1"]
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_main_self_launches_before_touching_torch(monkeypatch):
    """With --gpus 2 and no WORLD_SIZE, main() must hand over to the children and exit with their code without
    importing torch.cuda state itself (torch may be imported by the test session; what matters is the early exit)."""
    bench = _load_bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2"])
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(bench, "self_launch", lambda a: 0)
    try:
        bench.main()
    except SystemExit as e:
        assert e.code == 0
    else:
        raise AssertionError("main() continued in the parent process")


def test_source_hash_is_shared_with_the_profile_summary():
    """profiles/pmc.json is only trusted for the kernel sources it was taken on: both sides hash the same files."""
    bench = _load_bench()
    spec = importlib.util.spec_from_file_location("pmc_summary", os.path.join(ROOT, "scripts", "pmc_summary.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.KERNEL_SOURCES == bench.KERNEL_SOURCES
    assert mod.kernel_source_hash() == bench.kernel_source_hash()


def test_dump_outputs_writes_what_a_caller_reads(tmp_path):
    """--dump-outputs: one finite float64 array per record field; path samples only where BatchResult.path() gives a
    path, over the n_total samples a record can hold; the record's inf / NaN markers of values that do not exist are
    zero; above the cap a fixed sample of the instances."""
    import numpy as np
    import pytest
    bench = _load_bench()
    from integrated_path_planning_amd import _abi
    n, n_total = 4, 51
    recs = (_abi.Result * n)()
    for i, r in enumerate(recs):
        r.status = {1: _abi.PLAN_NO_PATH, 3: _abi.PLAN_C2F_FAILED}.get(i, _abi.PLAN_OK)
        r.n_keep, r.cost, r.stats_valid, r.stats[6] = 10 + i, 0.5 * i, int(i != 2), 40 + i
        for k in range(6):
            r.frenet0[k], r.ref0[k] = i + k, -i - k
        for k in range(_abi.MAX_NT):
            r.x[k] = k + 1.0
    # what the kernels write where a value does not exist (include/fot.h)
    recs[1].cost = recs[3].cost = float("inf")
    recs[3].n_keep = 0
    for k in range(6):
        recs[3].frenet0[k] = recs[3].ref0[k] = float("nan")
    raw = np.frombuffer(recs, np.uint8).copy()
    bench.dump_outputs(str(tmp_path), raw, n, n_total)
    x = np.load(tmp_path / "path_x.npy")
    assert x.dtype == np.float64 and x.shape == (n, n_total)
    assert np.array_equal(x[0, :10], np.arange(1.0, 11.0)) and not x[0, 10:].any()
    assert not x[1].any() and not x[3].any()                    # no path: None for the caller
    assert np.array_equal(x[2, :12], np.arange(1.0, 13.0)) and not x[2, 12:].any()
    assert np.array_equal(np.load(tmp_path / "cost.npy"), [0.0, 0.0, 1.0, 0.0])
    assert np.array_equal(np.load(tmp_path / "frenet0.npy")[:, 1], [1.0, 2.0, 3.0, 0.0])
    assert np.array_equal(np.load(tmp_path / "ref0.npy")[:, 1], [-1.0, -2.0, -3.0, 0.0])
    assert np.array_equal(np.load(tmp_path / "stats.npy")[:, 6], [40, 41, 0, 43])  # stats_valid == 0: None
    assert np.array_equal(np.load(tmp_path / "instance.npy"), [0, 1, 2, 3])
    assert {p.name for p in tmp_path.iterdir()} >= {"path_" + f + ".npy" for f in _abi.PATH_FIELDS}
    for p in tmp_path.iterdir():
        a = np.load(p)
        assert a.dtype == np.float64 and np.isfinite(a).all(), p.name

    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), raw, n, n_total, cap=2)
    sample = np.load(tmp_path / "a" / "instance.npy")
    assert len(sample) == 2 and np.array_equal(sample, np.load(tmp_path / "b" / "instance.npy"))
    for f in ("cost", "frenet0", "path_x"):
        assert np.array_equal(np.load(tmp_path / "a" / (f + ".npy")), np.load(tmp_path / (f + ".npy"))[sample.astype(int)])

    # a non-finite value where the record says the value exists is an error, and nothing is written
    recs[0].x[3] = float("nan")
    with pytest.raises(ValueError, match="path_x"):
        bench.dump_outputs(str(tmp_path / "c"), np.frombuffer(recs, np.uint8).copy(), n, n_total)
    assert not (tmp_path / "c").exists()
