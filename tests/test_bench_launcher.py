"""CPU: `python bench.py --gpus N` typed without a launcher starts its own ranks -- the command it builds is the one the driver uses for
N > 1 (`python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py <same args>`), as a
child process (subprocess, never os.exec*), before torch is imported; under a launcher (WORLD_SIZE set) nothing is started."""
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_launch_ranks_command(monkeypatch):
    b = _bench()
    seen = {}

    def fake_call(cmd, env=None):
        seen["cmd"], seen["env"] = cmd, env
        return 7

    import subprocess
    monkeypatch.setattr(subprocess, "call", fake_call)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "3", "--warmup", "1"])
    monkeypatch.delenv("MASTER_PORT", raising=False)
    assert b.launch_ranks(4) == 7  # the child's exit code is the launcher's
    cmd = seen["cmd"]
    assert cmd[0] == sys.executable and cmd[1:4] == ["-m", "torch.distributed.run", "--nnodes=1"]
    assert cmd[cmd.index("--nproc-per-node") + 1] == "4" and cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert 1024 < int(cmd[cmd.index("--master-port") + 1]) < 65536
    i = cmd.index(os.path.join(ROOT, "bench.py"))
    assert cmd[i + 1:] == ["--gpus", "4", "--steps", "3", "--warmup", "1"]  # the same arguments, after the script
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"  # dmabuf IPC: RCCL across processes needs it on this platform


def test_main_starts_ranks_only_without_a_launcher(monkeypatch):
    b = _bench()
    calls = []
    monkeypatch.setattr(b, "launch_ranks", lambda n: calls.append(n) or 0)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2"])
    try:
        b.main()
    except SystemExit as e:
        assert e.code == 0
    assert calls == [2]
    # under a launcher: a rank, no child -- it gets as far as the GPU check (this container has none) or the world-size check
    calls.clear()
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    try:
        b.main()
        raised = None
    except SystemExit as e:
        raised = e
    except Exception as e:  # noqa: BLE001 -- no GPU here: anything but a launch
        raised = e
    assert calls == [] and raised is not None


def test_plain_run_is_the_default_and_full_is_opt_in(monkeypatch):
    b = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "5", "--warmup", "2"])
    a = b.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 5 and a.warmup == 2
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = b.parse()
    assert a.full is True and a.dump_outputs == "out"


def test_dump_outputs_writes_a_fixed_sample_of_float64_columns(tmp_path):
    """--dump-outputs: one float64 array per PAF column, 64-bit query coordinates whole, and above DUMP_READS reads the same seeded
    sample of reads every time (two builds compare read for read), within 64 MB in all."""
    import numpy as np

    import mapquik_amd as mq
    b = _bench()
    n = b.DUMP_READS + 70001
    rng = np.random.default_rng(3)
    hits = np.zeros(n, dtype=mq.hit_dtype)
    for c in mq.hit_dtype.names:
        hits[c] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    hits["status"] = rng.integers(0, 3, n)
    hits["q_start_hi"] = 0
    hits["q_start_hi"][5] = 3
    for d in ("a", "b"):
        b.dump_outputs(mq, hits, str(tmp_path / d), 0, 1)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted([c + ".npy" for c in b.DUMP_COLUMNS] + ["read_index.npy"])
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in names) <= 64 << 20
    idx = np.load(tmp_path / "a" / "read_index.npy")
    assert idx.dtype == np.float64 and idx.size == b.DUMP_READS and np.all(np.diff(idx) > 0) and idx[-1] < n
    for f in names:
        x, y = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert x.dtype == np.float64 and x.shape == (b.DUMP_READS,) and np.array_equal(x, y)
    sel = idx.astype(np.int64)
    assert np.array_equal(np.load(tmp_path / "a" / "r_end.npy"), hits["r_end"][sel].astype(np.float64))
    assert np.array_equal(np.load(tmp_path / "a" / "q_start.npy"), mq.hit_column(hits, "q_start")[sel].astype(np.float64))
    # a batch within the budget is written whole, in read order; ranks of a multi-GPU run share the budget under their own names
    b.dump_outputs(mq, hits[:1000], str(tmp_path / "c"), 1, 2)
    assert np.array_equal(np.load(tmp_path / "c" / "rank1_read_index.npy"), np.arange(1000, dtype=np.float64))
    assert np.array_equal(np.load(tmp_path / "c" / "rank1_status.npy"), hits["status"][:1000].astype(np.float64))
