"""bench.py's launcher logic (no GPU needed): `python bench.py --gpus N` must start N ranks by itself, one per GPU, the way the
driver's own N > 1 command does (python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 ...).
Also its command line (a plain run unless --full) and what --dump-outputs writes, over a stand-in engine."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_gpus_1_is_not_respawned(bench):
    assert bench.spawn_command(bench.parse(["--gpus", "1"]), ["--gpus", "1"], {}, 8) is None
    assert bench.spawn_command(bench.parse([]), [], {}, 1) is None


def test_gpus_n_reexecutes_under_torch_distributed_run(bench):
    argv = ["--gpus", "4", "--steps", "7", "--warmup", "2"]
    cmd = bench.spawn_command(bench.parse(argv), argv, {"PATH": "/usr/bin"}, 8)
    assert cmd[1:4] == ["-m", "torch.distributed.run", "--nnodes=1"]
    assert cmd[cmd.index("--nproc-per-node") + 1] == "4"
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and 0 < int(cmd[cmd.index("--master-port") + 1]) < 65536
    script = cmd.index(os.path.join(ROOT, "bench.py"))
    assert cmd[script + 1:] == argv                       # every rank sees the same command line


def test_a_rank_is_not_respawned_and_a_wrong_world_is_refused(bench):
    argv = ["--gpus", "2"]
    assert bench.spawn_command(bench.parse(argv), argv, {"WORLD_SIZE": "2", "RANK": "1"}, 2) is None
    with pytest.raises(SystemExit) as e:
        bench.spawn_command(bench.parse(argv), argv, {"WORLD_SIZE": "1"}, 2)
    assert "WORLD_SIZE=1" in str(e.value)


def test_too_few_devices_is_an_error_not_an_n1_line(bench):
    argv = ["--gpus", "8"]
    with pytest.raises(SystemExit) as e:
        bench.spawn_command(bench.parse(argv), argv, {}, 1)
    assert "--gpus 8" in str(e.value) and "only 1 HIP device" in str(e.value)


def test_plain_run_is_the_default_and_steps_are_counted(bench):
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 3
    assert bench.parse(["--full", "--dump-outputs", "out"]).full and bench.parse(["--dump-outputs", "out"]).dump_outputs == "out"
    with pytest.raises(SystemExit):
        bench.parse(["--steps", "0"])


class _FakeEngine(object):
    """The read-out side of lqrrt_amd.engine.Engine that dump_outputs uses, over fixed arrays."""

    def __init__(self, size, n=6, m=3, H=20, seed=0):
        rs = np.random.RandomState(seed)
        self.size, self.n, self.m, self.horizon_iters = size, n, m, H
        self._x, self._K = rs.standard_normal((size, n)), rs.standard_normal((size, m, n))
        self._pid = np.concatenate([[-1], rs.randint(0, np.arange(1, size))]).astype(np.int32)
        self._len = rs.randint(1, H + 1, size).astype(np.int32)
        self._ign = rs.random_sample(size) < 0.1
        self._ex, self._eu = rs.standard_normal((size, H, n)), rs.standard_normal((size, H, m))     # rows past a length: junk

    def states(self):
        return self._x.copy()

    def gains(self):
        return self._K.copy()

    def parents(self):
        return self._pid.copy()

    def ignored(self):
        return self._ign.copy()

    def edges(self):
        return self._ex.copy(), self._eu.copy(), self._len.copy()


def _load_dir(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_writes_the_whole_tree_in_float64(bench, tmp_path):
    eng = _FakeEngine(500)
    names = bench.dump_outputs(eng, (131072, 4242), str(tmp_path))
    got = _load_dir(str(tmp_path))
    assert sorted(got) == names and all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["node_ids"], np.arange(500))
    assert np.array_equal(got["tree_states"], eng._x) and np.array_equal(got["tree_gains"], eng._K)
    assert np.array_equal(got["tree_parents"], eng._pid) and np.array_equal(got["tree_ignored"], eng._ign)
    assert np.array_equal(got["last_step_counts"], [131072, 4242])
    ln = eng._len
    for k in range(500):                        # an edge's own rows as the engine returns them, the rest zero
        assert got["tree_edge_lengths"][k] == ln[k]
        assert np.array_equal(got["tree_edge_x"][k, :ln[k]], eng._ex[k, :ln[k]]) and not got["tree_edge_x"][k, ln[k]:].any()
        assert np.array_equal(got["tree_edge_u"][k, :ln[k]], eng._eu[k, :ln[k]]) and not got["tree_edge_u"][k, ln[k]:].any()


def test_dump_outputs_samples_a_large_tree_the_same_way_every_time(bench, tmp_path):
    eng = _FakeEngine(3000)
    budget = 1 << 20
    bench.dump_outputs(eng, (1, 1), str(tmp_path / "a"), budget=budget)
    bench.dump_outputs(_FakeEngine(3000), (1, 1), str(tmp_path / "b"), budget=budget)
    a, b = _load_dir(str(tmp_path / "a")), _load_dir(str(tmp_path / "b"))
    assert sum(os.path.getsize(str(tmp_path / "a" / (k + ".npy"))) for k in a) <= budget + 128 * len(a)     # (+ .npy headers)
    ids = a["node_ids"].astype(np.int64)
    assert 0 < len(ids) < 3000 and np.all(np.diff(ids) > 0)
    assert np.array_equal(a["tree_states"], eng._x[ids]) and np.array_equal(a["tree_parents"], eng._pid[ids])
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
