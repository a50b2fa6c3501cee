"""bench.py's launcher contract (CPU): `--gpus N` without a launcher starts N ranks through
torch.distributed.run before anything in the parent touches the GPU, and a rank refuses to run
when WORLD_SIZE disagrees with --gpus."""
import importlib.util
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(REPO, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_launcher_command_starts_n_ranks():
    b = _bench()
    argv = ["--gpus", "8", "--steps", "2"]
    cmd = b.launcher_command(b.parse_args(argv), argv)
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nproc-per-node=8" in cmd and "--nnodes=1" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[-len(argv) - 1:] == [os.path.join(REPO, "bench.py"), *argv]


@pytest.mark.parametrize("gpus,world,ok", [(None, "1", True), (None, "4", True), (4, "4", True), (8, "4", False),
                                           (2, "1", False)])
def test_check_world(gpus, world, ok):
    b = _bench()
    args = b.parse_args([] if gpus is None else ["--gpus", str(gpus)])
    if ok:
        assert b.check_world(args, {"WORLD_SIZE": world}) == int(world)
    else:
        with pytest.raises(SystemExit) as e:
            b.check_world(args, {"WORLD_SIZE": world})
        assert e.value.code == 2


def test_main_spawns_before_touching_the_gpu(monkeypatch):
    import torch
    b = _bench()
    calls = []
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(b.subprocess, "call", lambda cmd, env=None: calls.append((cmd, env)) or 7)
    monkeypatch.setattr(b, "run", lambda args: pytest.fail("the parent must not render"))
    with pytest.raises(SystemExit) as e:
        b.main(["--gpus", "2", "--spp", "4"])
    assert e.value.code == 7                      # the launcher's exit status
    (cmd, env), = calls
    assert "--nproc-per-node=2" in cmd and cmd[-4:] == ["--gpus", "2", "--spp", "4"]
    assert env.get("HSA_ENABLE_IPC_MODE_LEGACY") == "0"
    assert not torch.cuda.is_initialized()


def test_defaults_are_the_baseline_workload():
    b = _bench()
    a = b.parse_args([])
    # N > 1 headline: the C4 1920x1080 frame strong-scaled over the ranks (the metric's resolution,
    # BASELINE.json north_star "1920x1080 ... at 1, 2, 4 and 8 GPUs"); weak scaling is a side field
    assert (a.gpus, a.config, a.scaling, a.walk, a.path) == (None, "c4", "strong", "ordered", "megakernel")
    assert b.parse_args(["--config", "c5"]).config == "c5"
    assert a.dispatch == 0   # the per-pass DispatchRay timing is opt-in, never the default line
    assert a.full is False and a.dump_outputs is None   # a plain run: the headline only, nothing written
    assert b.parse_args(["--full"]).full is True


def test_dump_outputs_whole_frame_and_seeded_sample(tmp_path):
    import numpy as np
    b = _bench()
    rng = np.random.default_rng(3)
    small = rng.random((36, 64, 4), dtype=np.float32)
    b.dump_outputs(str(tmp_path / "a"), small)
    got = np.load(tmp_path / "a" / "framebuffer.npy")
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got, small)
    # one pixel row past the limit: a sample of exactly the limit, the same pixels every time
    h = b.DUMP_MAX_BYTES // (1024 * 16) + 1
    big = np.arange(h * 1024 * 4, dtype=np.float32).reshape(h, 1024, 4)
    b.dump_outputs(str(tmp_path / "b"), big)
    b.dump_outputs(str(tmp_path / "c"), big)
    s1 = np.load(tmp_path / "b" / "framebuffer.npy")
    s2 = np.load(tmp_path / "c" / "framebuffer.npy")
    assert s1.dtype == np.float32 and s1.shape == (b.DUMP_MAX_BYTES // 16, 4) and s1.nbytes <= b.DUMP_MAX_BYTES
    np.testing.assert_array_equal(s1, s2)
    idx = (s1[:, 0] / 4).astype(np.int64)            # big's pixel p holds 4p .. 4p+3 (4p < 2^26 is exact in f32)
    assert (np.diff(idx) > 0).all() and idx[-1] < h * 1024
    np.testing.assert_array_equal(s1, big.reshape(-1, 4)[idx])
