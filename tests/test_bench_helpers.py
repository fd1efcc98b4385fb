"""CPU: the arithmetic bench.py's roofline objects rest on, and its refusal to let ranks share a card silently."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_algorithmic_bytes_follow_survey_8d():
    import bench

    # S(N) = 24 N + 150 + 16 read once and written once per launch; per env-step D obs + 26 mask + 2 (agent, done) + 1 action byte
    assert bench.algorithmic_bytes_per_launch(1, 3, 31, 1) == 2 * 238 + 60
    assert bench.algorithmic_bytes_per_launch(65536, 3, 31, 88) == 377225216  # 377.2 MB per launch
    assert bench.algorithmic_bytes_per_launch(65536, 2, 31, 64, records=False) == 65536 * 2 * 214
    # one step per launch with an int32 action in and no fused state: SURVEY's 539 B/step at N = 3 is 4 + 31 + 26 + 2 + 2 * 238
    assert 4 + 31 + 26 + 2 + 2 * 238 == 539


def test_expected_rng_outputs_per_deal():
    import bench

    # shuffle(150) + shuffle(150 - 12 N) + N x permutation(12) with numpy's masked rejection sampling
    n3 = bench.rng_outputs_per_deal(3)
    assert 410 < n3 < 420  # 415 outputs on average at three players (profiles: rng_outputs_per_deal)
    assert bench.rng_outputs_per_deal(2) > n3 - 40 and bench.rng_outputs_per_deal(4) < n3 + 40


def test_bench_without_a_gpu_fails_loudly():
    """bench.py is the product path: on a box without a GPU it must fail, not fall back to anything."""
    import torch

    if torch.cuda.is_available():
        return
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "0", "--no-cpu-baseline"],
                         capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert out.returncode != 0 and "needs a GPU" in (out.stderr + out.stdout)


def test_traffic_is_tied_to_the_kernel_sources_it_was_measured_on(tmp_path, monkeypatch):
    """roofline.traffic comes from a committed PMC digest: bench.py reports it only when the digest carries the sha256 of the
    kernel sources that are built now (VERDICT r3 "weak" #9) - otherwise null with the reason."""
    import json

    import bench

    sha = bench.kernel_source_sha256()
    assert len(sha) == 64 and sha == bench.kernel_source_sha256()
    shape = bench.launch_shape(65536, 3, 64, "mt19937", "one kernel", True, False)
    prof = tmp_path / "t.json"
    monkeypatch.setattr(bench, "TRAFFIC_PROFILE", str(prof))
    assert bench.committed_traffic(shape)[0] is None and "not found" in bench.committed_traffic(shape)[2]
    prof.write_text(json.dumps({"kernel_source_sha256": sha, "shape": dict(shape, games=4096), "k_step_bytes_per_launch": 5}))
    assert bench.committed_traffic(shape)[0] is None and "launch shape" in bench.committed_traffic(shape)[2]
    prof.write_text(json.dumps({"kernel_source_sha256": "0" * 64, "shape": shape, "k_step_bytes_per_launch": 5}))
    t = bench.committed_traffic(shape)
    assert t[0] is None and t[1] is None and "other kernel sources" in t[2]
    prof.write_text(json.dumps({"kernel_source_sha256": sha, "shape": shape, "k_step_bytes_per_launch": 5, "k_deal_fabric": {"read_bytes": 3, "write_bytes": 4}}))
    assert bench.committed_traffic(shape)[:2] == (5, 7)


def test_the_source_hash_ignores_comments_and_white_space(tmp_path, monkeypatch):
    """A comment fix in a kernel source must not orphan the committed PMC digest; a code change must."""
    import bench

    a = bench._code_only('int f(int x) {  // add one\n  return x + 1; /* really */ }\n')
    b = bench._code_only('int f(int x) {\n\n return x + 1;   }')
    c = bench._code_only('int f(int x) { return x + 2; }')
    assert a == b and a != c
    assert bench._code_only('const char *s = "// not a comment"; // one') == 'const char *s = "// not a comment";'


class _HostEngine:
    """What dump_outputs reads of an engine, on host tensors."""

    def __init__(self, B, D, N):
        import torch

        self.num_envs, self.obs_dim, self.num_players = B, D, N
        self._rewards = torch.arange(B * N, dtype=torch.float64).reshape(B, N)

    def rewards_tensor(self):
        return self._rewards.clone()


def test_dump_outputs_reads_both_record_layouts_alike_and_keeps_to_its_budget(tmp_path, monkeypatch):
    """--dump-outputs: the tile-planar ring [iters, tiles, P, 64, 16] and the row-major one [iters, B, record_bytes] holding the
    same records give the same files (float32 / float64); past the byte budget the games are a seeded sample, the same every time."""
    import numpy as np
    import torch

    import bench

    B, D, N, rb, iters = 200, 31, 3, 64, 8
    tiles = (B + 63) // 64
    g = torch.Generator().manual_seed(0)
    planar = torch.randint(0, 256, (iters, tiles, rb // 16, 64, 16), dtype=torch.uint8, generator=g)
    rows = planar.permute(0, 1, 3, 2, 4).reshape(iters, tiles * 64, rb)[:, :B].contiguous()
    act = torch.randint(-1, 26, (iters, B), dtype=torch.int32, generator=g)
    stats = np.arange(19.0)[None]
    eng = _HostEngine(B, D, N)
    bench.dump_outputs(str(tmp_path / "p"), eng, planar, act, True, stats)
    bench.dump_outputs(str(tmp_path / "r"), eng, rows, act, False, stats)
    names = sorted(p.name for p in (tmp_path / "p").iterdir())
    assert names == sorted(p.name for p in (tmp_path / "r").iterdir()) and "seq_observations.npy" in names
    for n in names:
        a, b = np.load(tmp_path / "p" / n), np.load(tmp_path / "r" / n)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), n
    seq = np.load(tmp_path / "p" / "seq_games.npy").astype(int)
    obs = np.load(tmp_path / "p" / "seq_observations.npy")
    assert obs.shape == (iters, len(seq), D) and len(np.load(tmp_path / "p" / "last_games.npy")) == B
    assert np.array_equal(obs[3, 5], rows[3, seq[5], :D].numpy().view(np.int8))
    assert np.array_equal(np.load(tmp_path / "p" / "last_action.npy"), rows[-1, :, D].numpy().view(np.int8))
    assert np.array_equal(np.load(tmp_path / "p" / "rewards.npy"), eng.rewards_tensor().numpy())
    # a budget smaller than one iteration of every game: seeded samples, identical from call to call, within the budget
    monkeypatch.setattr(bench, "DUMP_BYTES", 30000)
    n1 = bench.dump_outputs(str(tmp_path / "s1"), eng, planar, act, True, stats)
    bench.dump_outputs(str(tmp_path / "s2"), eng, planar, act, True, stats)
    assert n1 <= 30000 and 0 < len(np.load(tmp_path / "s1" / "last_games.npy")) < B
    for n in names:
        assert np.array_equal(np.load(tmp_path / "s1" / n), np.load(tmp_path / "s2" / n)), n
