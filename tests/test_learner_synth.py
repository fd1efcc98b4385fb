"""The synthetic learner inputs of tests/learner_synth.py reach what they are meant to reach - asserted on the numpy restatements
alone, without a GPU, for exactly the cases tests/test_gpu_learner_synthetic.py feeds the kernels.

What a case cannot reach by construction is excepted here, by name: with T = 1 the flags value 2 (EPISODE_KNOWN without a target)
cannot occur - an episode end on the only row makes every seat TERMINAL, and a row that wipes that state is no transition; a
single game (B = 1) is either bootstrapped from ``values[T]`` or not, so B = 1 has two seeds and a case's seeds are judged together.
"""
import numpy as np
import pytest

from tests import learner_synth as synth
from tests import rollout_batches_ref as bref
from tests import rollout_targets_ref as tref


def _recursion(agent, done, episode_end, values, final_rewards, gamma, lam, fused):
    """``rollout_targets_ref.targets_f32``'s advantages with the states of the acting seat ('T'ERMINAL / 'N'EXT per row) - and, with
    ``fused``, the two multiply-adds of the NEXT branch contracted: the product exact (two float32 multiply exactly in float64), the
    sum formed in float64 and rounded once."""
    f, w = np.float32, np.float64
    T, B = episode_end.shape
    N = final_rewards.shape[2]
    g, gl = f(gamma), f(f(gamma) * f(lam))
    state = np.zeros((B, N), dtype=np.int8)
    R, nv, na = (np.zeros((B, N), dtype=f) for _ in range(3))
    rows = np.arange(B)
    boot = done[T] == 0
    s = agent[T].astype(np.int64)
    state[rows[boot], s[boot]] = 2
    nv[rows[boot], s[boot]] = values[T][boot]
    adv = np.zeros((T, B), dtype=f)
    branch = np.zeros((T, B), dtype=np.int8)
    for t in range(T - 1, -1, -1):
        e = episode_end[t] != 0
        state[e] = 1
        R[e] = final_rewards[t][e].astype(f)
        inv = done[t] != 0
        s = np.where(inv, 0, agent[t]).astype(np.int64)
        V = values[t]
        st = state[rows, s]
        if fused:
            d = (w(g) * nv[rows, s].astype(w) - V.astype(w)).astype(f)
            a_next = (d.astype(w) + w(gl) * na[rows, s].astype(w)).astype(f)
        else:
            d = g * nv[rows, s] - V
            a_next = d + gl * na[rows, s]
        A = np.where(st == 1, R[rows, s] - V, np.where(st == 2, a_next, f(0))).astype(f)
        A = np.where(inv, f(0), A).astype(f)
        adv[t] = A
        branch[t] = np.where(inv, 0, st)
        state[inv] = 0
        ok = ~inv
        state[rows[ok], s[ok]] = 2
        nv[rows[ok], s[ok]] = V[ok]
        na[rows[ok], s[ok]] = A[ok]
    return adv, branch


@pytest.mark.parametrize("T,B,N", synth.TARGET_CASES)
def test_targets_cases_reach_every_branch(T, B, N):
    seen_flags, terminal, nxt, booted, not_booted, no_target, contracted = set(), 0, 0, 0, 0, 0, 0
    ends_first = ends_last = end_and_done = done_last = unread = inexact = 0
    for seed in synth.target_seeds(T, B, N):
        case = synth.targets_case(T, B, N, seed)
        c = case["cols"]
        assert case["records"].shape == (T + 1, B, 64) and c["values"].shape == (T + 1, B) and c["final_rewards"].shape == (T, B, N)
        assert (c["agent"][c["done"] == 0] < N).all()
        for gamma, lam in synth.PARAMS:
            adv, tgt, ret, flags = tref.targets_f32(gamma=gamma, lam=lam, **c)
            mine, branch = _recursion(gamma=gamma, lam=lam, fused=False, **c)
            assert np.array_equal(mine.view(np.uint32), adv.view(np.uint32))     # the copy above IS the recursion
        adv, tgt, ret, flags = tref.targets_f32(gamma=0.99, lam=0.95, **c)
        mine, branch = _recursion(gamma=0.99, lam=0.95, fused=False, **c)
        fused, _ = _recursion(gamma=0.99, lam=0.95, fused=True, **c)
        contracted += int((fused.view(np.uint32) != adv.view(np.uint32)).sum())
        seen_flags |= set(np.unique(flags).tolist())
        terminal += int((branch == 1).sum())
        nxt += int((branch == 2).sum())
        b = (c["done"][T] == 0)
        booted, not_booted = booted + int(b.sum()), not_booted + int((~b).sum())
        no_target += int(((c["done"][:T] == 0) & ((flags & 1) == 0)).sum())
        e = c["episode_end"] != 0
        ends_first += int((e[0] & (c["done"][0] == 0)).sum())
        ends_last += int((e[T - 1] & (c["done"][T - 1] == 0)).sum())
        end_and_done += int((e & (c["done"][:T] != 0)).sum())
        done_last += int((c["done"][T] != 0).sum())
        unread += int((c["final_rewards"][~e] != 0).sum())
        inexact += int((c["final_rewards"][e].astype(np.float32).astype(np.float64) != c["final_rewards"][e]).sum())
        # the dirty planar image holds the same records, and something non-zero in every padding slot
        flat = case["planar"].reshape(-1)
        s_, b_, k_ = np.meshgrid(np.arange(T + 1), np.arange(B), np.arange(64), indexing="ij")
        assert np.array_equal(flat[bref.byte(s_ * case["planar"].shape[1] * 64 + b_, k_, 64, True)], case["records"])
        if B % 64:
            assert (case["planar"][:, -1, :, B % 64:, :] != 0).all()
    assert seen_flags == ({0, 1, 3} if T == 1 else {0, 1, 2, 3}), seen_flags
    assert terminal > 0 and nxt > 0 and booted > 0 and not_booted > 0 and no_target > 0
    assert ends_first > 0 and ends_last > 0 and unread > 0 and inexact > 0
    assert contracted > 0            # a contracted multiply-add changes bits of this very case
    if B > 1:
        assert end_and_done > 0 and done_last > 0
        top = np.abs(c["values"]).max(0)
        assert top.max() > 1e3 * top.min()                                           # games of different scales side by side


def test_gather_inputs_hold_every_edge_byte():
    pieces = set()
    for N, indirect in synth.GATHER_GEOMETRIES:
        case = synth.gather_case(N, indirect)
        g = case["geometry"]
        D, Dp, rb = g["obs_dim"], g["mask_offset"], g["record_bytes"]
        pieces.add(rb // 16)
        B, T = synth.GATHER_B, synth.GATHER_T
        rec, planar = case["records"], case["planar"]
        stride = planar.shape[1] * 64
        assert (planar[:, -1, :, B % 64:, :] != 0).all()
        assert [case["lists"][f"perm-{m}"].size for m in synth.GATHER_M] == list(synth.GATHER_M)
        n = T * B
        for name, index in case["lists"].items():
            a = bref.gather(rec, False, rb, D, B, T, B, index, **case["cols"])
            p = bref.gather(planar, True, rb, D, B, T, stride, index, **case["cols"])
            for k in a:
                assert np.array_equal(a[k], p[k]), (N, indirect, name, k)
            ok = (index >= 0) & (index < n)
            assert {"out-of-range": not ok.any(), "interleaved": ok.any() and (~ok).any()}.get(name, ok.all()), name
        index = case["lists"]["perm-600"]
        rows = rec[:T].reshape(n, rb)[index]
        assert all((rows[:, :D] == v).any() for v in synth.OBS_EDGES)
        assert all((rows[:, Dp:Dp + 26] == v).any() for v in synth.MASK_EDGES)
        assert rows[:, D:Dp].any() and rows[:, Dp + 30:].any()                      # the padding of a record is dirty
        assert (rows[:, Dp + 26] >= N).any()                                         # seats a game cannot name (on rows with done set)
        part = case["lists"]["partial-tile"]
        assert part.size == T * (B % 64) and ((part % B) >= (B // 64) * 64).all()
        assert set(np.int64([-1, n, 2 ** 63 - 1, -2 ** 63]).tolist()) <= set(case["lists"]["out-of-range"].tolist())
        assert set(np.int64([-1, n, 2 ** 63 - 1, -2 ** 63]).tolist()) <= set(case["lists"]["interleaved"].tolist())
        assert case["lists"]["copies"].size == 64 and len(set(case["lists"]["copies"].tolist())) == 1
    # every record size the engine has: record_bytes / 16 of both observation modes and 1 .. 12 players
    offered = set(synth.geometry(N, ind)["record_bytes"] // 16 for N in range(1, 13) for ind in (True, False))
    assert pieces == offered == set(range(4, 14)), (pieces, offered)
    mean, std = synth.GATHER_NORMS[1]
    assert float(np.float32(mean)) != mean and float(np.float32(std)) != std


@pytest.mark.parametrize("n", synth.SELECT_SIZES)
def test_select_patterns_select_what_they_say(n):
    nb = (n + synth.SEL_ROWS - 1) // synth.SEL_ROWS
    assert nb >= 1024                # every thread of the scan owns a block; beyond 1 024 some own two and trailing ones none
    for pattern in synth.SELECT_PATTERNS:
        f = synth.select_flags(n, pattern, np.random.default_rng(n % 1000 + len(pattern)))
        assert f.shape == (n,) and f.dtype == np.uint8
        for require in (1, 2, 3):
            idx = bref.select(f, require)
            share = idx.size / n
            if pattern == "random":
                assert 0.01 <= share <= 0.99
            elif pattern == "all":
                assert idx.size == n
            elif pattern == "none":
                assert idx.size == 0
            elif pattern == "first":
                assert idx.tolist() == [0]
            elif pattern == "last":
                assert idx.tolist() == [n - 1]
            else:   # islands: rows in the island blocks only, some in each of them (few of all rows, by design)
                blocks = set((idx // synth.SEL_ROWS).tolist())
                assert blocks == set(synth.island_blocks(n)) and len(blocks) >= 2
        assert (f >> 2).any()        # bits the definition ignores are set
    # (the workload's 20 971 520 random rows are generated the same way: the share of a random pattern does not depend on n)
    assert (synth.WORKLOAD_ROWS + synth.SEL_ROWS - 1) // synth.SEL_ROWS == 5120
