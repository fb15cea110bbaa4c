"""bench.py's multi-rank launch path (VERDICT r02 'Missing #1'): `python bench.py --gpus N`
without torchrun's environment starts N ranks itself and relays rank 0's line; a launch
whose WORLD_SIZE disagrees with --gpus is refused.  CPU only (--plumbing: rendezvous and
one all-reduce over gloo, no GPU work)."""
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, "bench.py")


def _run(args, env_extra=None, timeout=240):
    env = dict(os.environ, BPK_DIST_BACKEND="gloo")
    env.pop("WORLD_SIZE", None)
    env.update(env_extra or {})
    p = subprocess.run([sys.executable, BENCH] + args, env=env, capture_output=True, text=True,
                       timeout=timeout, cwd="/tmp")
    return p.returncode, p.stdout, p.stderr


def test_gpus_2_spawns_two_ranks_and_relays_one_line():
    rc, out, err = _run(["--gpus", "2", "--plumbing"])
    assert rc == 0, err[-2000:]
    lines = [l for l in out.splitlines() if l.strip()]
    assert len(lines) == 1, out
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["backend"] == "gloo"
    assert d["value"] == 3.0  # all-reduce of rank ids + 1 over both ranks
    # configs[2] strong scaling by default: global batch 64 sharded 32 per rank
    assert d["per_gpu_batch"] == 32 and d["scaling"] == "strong"


def test_weak_flag_keeps_the_whole_batch_per_rank():
    rc, out, err = _run(["--gpus", "2", "--plumbing", "--weak"])
    assert rc == 0, err[-2000:]
    d = json.loads(out.strip().splitlines()[-1])
    assert d["per_gpu_batch"] == 64 and d["scaling"] == "weak"


def test_global_batch_must_shard_evenly():
    rc, out, err = _run(["--gpus", "2", "--plumbing", "--global-batch", "7"])
    assert rc != 0 and "does not shard" in err


def test_gpus_1_runs_in_process():
    rc, out, err = _run(["--gpus", "1", "--plumbing"])
    assert rc == 0, err[-2000:]
    assert json.loads(out.strip())["n_gpus"] == 1


def test_mismatched_world_size_is_refused():
    rc, out, err = _run(["--gpus", "1", "--plumbing"], {"WORLD_SIZE": "2", "RANK": "0"})
    assert rc == 2 and "refusing" in err and not out.strip()


def test_full_and_dump_outputs_are_accepted():
    rc, out, err = _run(["--gpus", "1", "--plumbing", "--full", "--dump-outputs", "unused"])
    assert rc == 0, err[-2000:]
    assert json.loads(out.strip())["n_gpus"] == 1


def test_dump_outputs_float32_and_fixed_sample_beyond_the_cap(tmp_path):
    """dump_outputs writes <name>.npy in float32; past the byte cap each array becomes a
    seeded sample of its flat elements -- the same indices on every call, in order."""
    code = ("import sys, torch, bench\n"
            "arrs = {'a': torch.arange(100, dtype=torch.float64), 'b': torch.ones(2, 3)}\n"
            "bench.dump_outputs(sys.argv[1], arrs, cap=int(sys.argv[2]))\n")
    import numpy as np
    got = {}
    for tag, cap in (("whole", 1 << 20), ("s1", 80), ("s2", 80)):
        d = str(tmp_path / tag)
        p = subprocess.run([sys.executable, "-c", code, d, str(cap)], capture_output=True,
                           text=True, timeout=240, cwd=REPO)
        assert p.returncode == 0, p.stderr[-2000:]
        got[tag] = {n: np.load(os.path.join(d, n + ".npy")) for n in ("a", "b")}
    assert got["whole"]["a"].dtype == np.float32 and got["whole"]["b"].shape == (2, 3)
    np.testing.assert_array_equal(got["whole"]["a"], np.arange(100, dtype=np.float32))
    a = got["s1"]["a"]  # 80 bytes / (4 bytes x 2 arrays) = 10 elements each at the most
    assert a.shape == (10,) and np.all(np.diff(a) > 0) and got["s1"]["b"].shape == (2, 3)
    np.testing.assert_array_equal(a, got["s2"]["a"])
    assert sum(v.nbytes for v in got["s1"].values()) <= 80


def test_per_rank_of_gives_the_n_gpu_per_rank_batch():
    """--per-rank-of 8 on one process: every phase at the per-rank batch of the 8-GPU
    strong-scaled run (64 / 8 = 8 for configs[2])."""
    rc, out, err = _run(["--gpus", "1", "--plumbing", "--per-rank-of", "8"])
    assert rc == 0, err[-2000:]
    d = json.loads(out.strip().splitlines()[-1])
    assert d["per_gpu_batch"] == 8 and d["scaling"] == "strong"
