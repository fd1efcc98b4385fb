"""GPU: float64 rewards and final scores at EVERY episode end, for every player count and both observations, against the CPU
oracle - bit for bit, under settings at which the order of the float64 operations shows.

Everywhere else the suite compares rewards under ``score_penalty = 2``: with integer scores and a dyadic penalty every sum is
exact, and summation order, a contracted multiply-add and the pairwise branch of np.mean (eight players and more) are invisible.
Here every engine and every oracle uses ``score_penalty = 1/3``, ``mean_reward = 0.1``, ``reward_refunded = 0.007``; the oracle's
arithmetic under such settings is pinned to the reference by tests/test_scoring_order.py (tests/golden/scoring_order.npz).
B = 130 games: two full tiles and a tile of two lanes.  No tolerance anywhere: float64 is compared with ``==``; the one exception
is the per-seat sum of scores over all games, whose order of accumulation is not the oracle's (stated at the assertion).

  1. the two host-callable scoring helpers on every row of the fixture;
  2. the fused rollout (on-device policy), N = 1 .. 12 x both observations x both generators x every dealing form: one iteration,
     then launches of TWO iterations - a draw and a place alternate and a re-deal takes one iteration, so finished games stand
     finished after every odd iteration and at no other time - with the records, ``done``, and the rewards and scores of the games
     that stand finished compared after every launch;
  3. one long launch without auto-reset that plays all B games to their end (the one-kernel form over several dealing cycles in ONE
     launch where it exists: deferred scoring, cycle ends), every game's rewards and scores, the per-seat sums of ``counters()``;
  4. the caller-action path (observe_host, observe_host of a seat that is not on turn, step_host, skyjo_vec_step_collect on device
     pointers) with illegal actions and SKYJO_ACTION_SKIP in the draw, at B = 130 and - six tiles: no raw export, get_state and
     rewards_host read the device copy - at B = 321.
"""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest

from tests import scoring_order_ref as ref

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
B = 130
PENALTY, MEAN_REWARD, REWARD_REFUNDED = 1.0 / 3.0, 0.1, 0.007
POLICY_SEED = 77
PLAYERS = list(range(1, 13))

# Case 2.  SEED[N]: the first base seed (1, 2, ...) at which the oracle alone, under either generator, sees at least five finished
# games with an order-sensitive mean among the first T[N] iterations (N >= 8; below eight players any seed does: 1).
# T[N] = 1 + 2k: the smallest such count of iterations after which the oracle alone reports at least B finished episodes under
# both generators (the observation does not change the play).  Computed on the CPU: tools/dev/scoring_geometry_tables.py.
# Order-sensitive means among the finished games by T[N], MT19937 / Philox: N = 8: 16 / 25, 9: 26 / 25, 10: 18 / 27, 11: 23 / 13,
# 12: 14 / 19 - the first seed tried does for every N.
SEED = {1: 1, 2: 1, 3: 1, 4: 1, 5: 1, 6: 1, 7: 1, 8: 1, 9: 1, 10: 1, 11: 1, 12: 1}
T = {1: 67, 2: 117, 3: 159, 4: 197, 5: 241, 6: 269, 7: 311, 8: 351, 9: 379, 10: 423, 11: 475, 12: 507}
# Case 3.  K_END[N]: iterations after which every one of the B games (base seed SEED[N], generator (N + indirect) % 2, no auto-reset)
# has ended under either generator, rounded up to a multiple of 64.
K_END = {1: 128, 2: 192, 3: 256, 4: 256, 5: 256, 6: 320, 7: 320, 8: 384, 9: 384, 10: 448, 11: 512, 12: 512}
# Case 4.  STEPS[N]: steps of the caller-action loop (seed 40 + N below), enough for at least ten SCORED episode ends at B = 130
# although 0.2 % illegal actions end most long games early.
STEPS = {1: 50, 2: 100, 3: 100, 4: 150, 5: 150, 6: 200, 7: 200, 8: 250, 9: 250, 10: 300, 11: 300, 12: 300}


def _cfg(N, ind, rng_mode, auto_reset=True):
    return dict(num_players=N, score_penalty=PENALTY, observe_other_player_indirect=bool(ind), mean_reward=MEAN_REWARD,
                reward_refunded=REWARD_REFUNDED, rng_mode=rng_mode, auto_reset=auto_reset)


def _oracle(num_envs, **cfg):
    from oracle import skyjo_oracle as so
    return so.OracleVec(num_envs=num_envs, **cfg)


def _oracle_scores(ora, games):
    N = ora.num_players
    return np.array([[ora.game(int(i)).final_score[p] for p in range(N)] for i in games], dtype=np.float64).reshape(len(games), N)


def _oracle_eplen(ora):
    return np.ctypeslib.as_array(ora.v.contents.ep_len, shape=(ora.num_envs,)).astype(np.uint16)


def _record_bytes(obs, action, mask, meta, eplen):
    """The defined bytes of the engine's records (include/skyjo_vec.h), built from what the oracle shows: observation, the applied
    action (byte D), the action mask, agent, phase, done, status, episode steps.  (What follows them up to record_bytes is padding.)"""
    D = obs.shape[-1]
    assert D % 4 == 3  # 31, or 19 + 12 N: the action byte fills the word, the mask starts at D + 1
    dp = D + 1
    out = np.zeros(obs.shape[:-1] + (dp + 32,), dtype=np.uint8)
    out[..., :D] = obs.view(np.uint8)
    out[..., D] = np.asarray(action).astype(np.int8).view(np.uint8)
    out[..., dp:dp + 26] = mask.view(np.uint8)
    out[..., dp + 26:dp + 30] = meta
    e = np.asarray(eplen).astype(np.uint16)
    out[..., dp + 30], out[..., dp + 31] = e & 0xff, e >> 8
    return out


# ----------------------------------------------------------------------------------------------------------------- 1. helpers
@pytest.mark.parametrize("N", PLAYERS)
def test_scoring_helpers_on_the_order_fixture(N):
    """skyjo_vec_evaluate_game / skyjo_vec_calc_final_rewards on every row of tests/golden/scoring_order.npz: all four penalties, all four
    reward pairs, the hands' integer scores and the arbitrary float64 score vectors."""
    from skyjo_rl_amd import _lib

    L = _lib.load()
    fx = np.load(os.path.join(GOLDEN, "scoring_order.npz"))
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    p = "N%d_" % N
    hands = np.ascontiguousarray(fx[p + "hands"], dtype=np.int8)
    fin = np.ascontiguousarray(fx[p + "finisher"], dtype=np.int32)
    E = hands.shape[0]
    for k, pen in enumerate(fx["penalties"]):
        sc = np.zeros((E, N), dtype=np.float64)
        _lib.check(L.skyjo_vec_evaluate_game(0, E, N, vp(hands), vp(fin), float(pen), vp(sc)))
        np.testing.assert_array_equal(sc, fx[p + "scores"][k], err_msg=f"scores N={N} penalty={pen}")
        for j, (mr, rr) in enumerate(fx["reward_cfgs"]):
            rows = np.flatnonzero(fx[p + "cfg"][k] == j)
            assert len(rows) > 0
            s = np.ascontiguousarray(fx[p + "scores"][k][rows])
            rf = np.ascontiguousarray(fx[p + "refunded"][rows], dtype=np.int32)
            rew = np.zeros((len(rows), N), dtype=np.float64)
            _lib.check(L.skyjo_vec_calc_final_rewards(0, len(rows), N, vp(s), vp(rf), float(mr), float(rr), vp(rew)))
            np.testing.assert_array_equal(rew, fx[p + "rewards"][k][rows], err_msg=f"rewards N={N} penalty={pen} pair={j}")
    fs = np.ascontiguousarray(fx[p + "fscores"])
    frf = np.ascontiguousarray(fx[p + "frefunded"], dtype=np.int32)
    for j, (mr, rr) in enumerate(fx["reward_cfgs"]):
        rew = np.zeros(fs.shape, dtype=np.float64)
        _lib.check(L.skyjo_vec_calc_final_rewards(0, fs.shape[0], N, vp(fs), vp(frf), float(mr), float(rr), vp(rew)))
        np.testing.assert_array_equal(rew, fx[p + "frewards"][j], err_msg=f"rewards of score vectors N={N} pair={j}")


# ----------------------------------------------------------------------------------------------------------------- 2. fused rollout
def rollout_reference(N, ind, rng_mode, iterations=None):
    """The oracle's side of case 2, once per (N, observation, generator): per launch (one iteration, then two at a time) the actions,
    the records' defined bytes, done, and for the games that stand finished their indices, rewards and scores; and the counters."""
    ora = _oracle(B, **_cfg(N, ind, rng_mode))
    ora.seed(None, SEED[N])
    launches, total = [], 0
    iterations = T[N] if iterations is None else iterations
    while total < iterations:
        k = 1 if total == 0 else 2
        oact, obs, mask, meta, eplen = ora.rollout(k, POLICY_SEED, record_obs=True)
        done = ora.dones
        idx = np.flatnonzero(done)
        launches.append((k, oact, _record_bytes(obs, oact, mask, meta, eplen), done, idx, ora.rewards[idx], _oracle_scores(ora, idx)))
        total += k
    return launches, ora.counters()


_cached_rollout_reference = functools.lru_cache(maxsize=2)(rollout_reference)  # (the dealing forms of one configuration follow each other)

FORMS = {"in line": 0, "two streams": 2, "one kernel": 3, "one kernel, tile-planar records": 3}


def _rollout_cases():
    for N in PLAYERS:
        for ind in (True, False):
            for rng_mode in (0, 1):
                for form in FORMS:
                    if FORMS[form] == 3 and N not in (2, 3, 4):
                        continue  # the one-kernel form is compiled for two to four players
                    yield pytest.param(N, ind, rng_mode, form, id=f"N{N}-{'indirect' if ind else 'direct'}-{'philox' if rng_mode else 'mt19937'}-{form.replace(' ', '_').replace(',', '')}")


@pytest.mark.parametrize("N,ind,rng_mode,form", list(_rollout_cases()))
def test_fused_rollout_rewards_and_scores_at_every_episode_end(N, ind, rng_mode, form):
    import torch
    from skyjo_rl_amd import SkyjoVecEnv

    launches, oc = _cached_rollout_reference(N, ind, rng_mode)
    eng = SkyjoVecEnv(B, **_cfg(N, ind, rng_mode))
    eng.set_overlap(FORMS[form])
    assert eng.dealing_form() == form.split(",")[0]
    eng.seed(None, SEED[N])
    planar = form.endswith("tile-planar records")
    if planar:
        eng.set_record_layout("tile-planar")
    rec = {k: eng.new_planar_records(k) if planar else eng.new_records(k) for k in (1, 2)}
    act = {k: torch.empty((k, B), dtype=torch.int32, device="cuda") for k in (1, 2)}
    finished = sensitive = 0
    for c, (k, oact, want, odone, idx, orew, osc) in enumerate(launches):
        at = f"launch {c} ({k} iteration{'s' if k > 1 else ''})"
        eng.rollout(k, policy_seed=POLICY_SEED, records=rec[k], actions=act[k])
        rows = eng.rows_from_planar(rec[k]) if planar else rec[k]
        np.testing.assert_array_equal(rows.cpu().numpy()[..., :want.shape[-1]], want, err_msg="records, " + at)
        np.testing.assert_array_equal(act[k].cpu().numpy(), oact, err_msg="actions, " + at)
        rew, sc, done = eng.rewards_host()
        np.testing.assert_array_equal(done, odone, err_msg="done, " + at)
        np.testing.assert_array_equal(rew[idx], orew, err_msg="rewards of the finished games, " + at)
        np.testing.assert_array_equal(sc[idx], osc, err_msg="scores of the finished games, " + at)
        finished += len(idx)
        sensitive += sum(ref.order_sensitive(s) for s in osc)
    cn = eng.counters()
    for key in ("steps", "episodes", "resets", "sum_len", "illegal"):
        assert cn[key] == oc[key], (key, cn[key], oc[key])
    print(f"{len(launches)} launches, {finished} finished games compared, {sensitive} of them with an order-sensitive mean")
    assert finished >= B and cn["episodes"] == finished and cn["illegal"] == 0, (finished, cn["episodes"])
    if N >= 8:
        assert sensitive >= 5, sensitive  # games whose np.mean differs from the left-to-right sum / N: the pairwise branch shows
    eng.close()


# ----------------------------------------------------------------------------------------------------------------- 3. long launches
@pytest.mark.parametrize("ind", [True, False], ids=["indirect", "direct"])
@pytest.mark.parametrize("N", PLAYERS)
def test_one_launch_plays_every_game_to_its_end(N, ind):
    """tests/test_gpu_parity.py::test_rollout_without_auto_reset_runs_every_game_to_its_end for every (N, observation): ONE rollout
    call long enough for all B games to end and then stand still.  Two to four players: the one-kernel form over several dealing
    cycles in one launch (games are scored deferred, on the LDS copy of their card rows, and at the cycle ends); in line otherwise."""
    import torch
    from skyjo_rl_amd import SkyjoVecEnv

    rng_mode = (N + int(ind)) % 2
    cfg = _cfg(N, ind, rng_mode, auto_reset=False)
    eng = SkyjoVecEnv(B, **cfg)
    one_kernel = N in (2, 3, 4)
    eng.set_overlap(3 if one_kernel else 0)
    assert eng.dealing_form() == ("one kernel" if one_kernel else "in line")
    K = K_END[N]
    if one_kernel:
        eng.set_deal_interval(eng.deal_interval())  # pinned: a launch of whole cycles
        cycles = -(-K // eng.deal_interval())
        assert 2 <= cycles <= 16, cycles  # (sixteen: the most one launch takes)
        K = cycles * eng.deal_interval()
    ora = _oracle(B, **cfg)
    eng.seed(None, SEED[N])
    ora.seed(None, SEED[N])
    rec = eng.new_records(K)
    act = torch.empty((K, B), dtype=torch.int32, device="cuda")
    eng.rollout(K, policy_seed=POLICY_SEED, records=rec, actions=act)
    got, gact = rec.cpu().numpy(), act.cpu().numpy()
    for s0 in range(0, K, 256):
        n = min(256, K - s0)
        oact, obs, mask, meta, eplen = ora.rollout(n, POLICY_SEED, record_obs=True)
        want = _record_bytes(obs, oact, mask, meta, eplen)
        np.testing.assert_array_equal(got[s0:s0 + n, :, :want.shape[-1]], want, err_msg=f"records, iterations {s0}..{s0 + n - 1}")
        np.testing.assert_array_equal(gact[s0:s0 + n], oact, err_msg=f"actions, iterations {s0}..{s0 + n - 1}")
    c, oc = eng.counters(), ora.counters()
    for key in ("steps", "episodes", "resets", "sum_len", "illegal"):
        assert c[key] == oc[key], (key, c[key], oc[key])
    assert c["episodes"] == B and c["resets"] == 0 and c["illegal"] == 0
    rew, sc, done = eng.rewards_host()
    assert done.all() and ora.dones.all()
    osc = _oracle_scores(ora, range(B))
    np.testing.assert_array_equal(rew, ora.rewards)
    np.testing.assert_array_equal(sc, osc)
    if N >= 8:
        assert sum(ref.order_sensitive(s) for s in osc) >= 5
    # Per-seat sums over the finished episodes.  num_refunded: integers, exact in any order - equal.
    oscore, orefunded = ora.seat_sums()
    np.testing.assert_array_equal(c["sum_refunded"], orefunded)
    # Final scores: the penalised finisher's is inexact under penalty 1/3, so the order of accumulation shows, and it is NOT the
    # oracle's.  The oracle adds game 0, 1, ... B - 1 in turn (one accumulator per game and seat, numpy's sum down the rows).  The
    # engine keeps one accumulator per lane (= game), adds the 64 lanes of a tile as a shuffle tree (lane l + lane l + 32, + 16, ...),
    # then the tiles' sums (k_reduce_stats: another tree, then atomics).  Either is a sum of the same B numbers in some order: both
    # lie within  B * 2^-53 * sum |x|  of the exact sum.
    for s in range(N):
        x = osc[:, s]
        exact, bound = math.fsum(x), B * 2.0 ** -53 * math.fsum(np.abs(x))
        assert abs(float(c["sum_score"][s]) - exact) <= bound, (s, float(c["sum_score"][s]), exact, bound)
        assert abs(float(oscore[s]) - exact) <= bound, (s, float(oscore[s]), exact, bound)
    eng.close()


# ----------------------------------------------------------------------------------------------------------------- 4. caller actions
def caller_actions(rng, mask, n, share=0.002):
    """One step's actions: a uniformly random legal action per game, 0.2 % (``share``) arbitrary ones from -2 .. 28 (mostly illegal),
    1 % SKYJO_ACTION_SKIP."""
    from oracle import skyjo_oracle as so

    acts = np.argmax(rng.random((n, 26)) * mask, axis=1).astype(np.int32)
    bad = rng.random(n) < share
    acts[bad] = rng.integers(-2, 29, size=int(bad.sum()))
    acts[rng.random(n) < 0.01] = so.ACTION_SKIP
    return acts


def _caller_path(N, ind, num_envs, steps, min_scored):
    import torch
    from oracle import skyjo_oracle as so
    from skyjo_rl_amd import SkyjoVecEnv, _lib

    L = _lib.load()
    rng_mode = (N + int(ind)) % 2
    cfg = _cfg(N, ind, rng_mode)
    eng = SkyjoVecEnv(num_envs, **cfg)
    ora = _oracle(num_envs, **cfg)
    eng.seed(None, 40 + N)
    ora.seed(None, 40 + N)
    rng = np.random.default_rng(1000 + N)
    rec_d = eng.new_records()
    act_d = torch.empty(num_envs, dtype=torch.int32, device="cuda")
    fr_d = torch.empty((num_envs, N), dtype=torch.float64, device="cuda")
    ee_d = torch.empty(num_envs, dtype=torch.uint8, device="cuda")
    vp = lambda t: C.c_void_p(t.data_ptr())
    scored = illegal_ends = skipped = states = 0
    for t in range(steps):
        obs, mask, agent, phase = ora.observe()
        if t % 4 == 0:
            o = eng.observe_host()
            np.testing.assert_array_equal(o.observations, obs, err_msg=f"obs t={t}")
            np.testing.assert_array_equal(o.action_mask, mask, err_msg=f"mask t={t}")
            np.testing.assert_array_equal(o.agent, agent, err_msg=f"agent t={t}")
            np.testing.assert_array_equal(o.phase, phase, err_msg=f"phase t={t}")
        if t % 8 == 3 and N > 1:  # a seat that is not on turn (skyjo_env.py:199-214)
            seats = ((agent.astype(np.int32) + 1 + t % (N - 1)) % N).astype(np.int32)
            assert (seats != agent).all()
            oo = eng.observe_host(seats)
            oobs, omask, _, _ = ora.observe(seats)
            np.testing.assert_array_equal(oo.observations, oobs, err_msg=f"obs of the other seat t={t}")
            np.testing.assert_array_equal(oo.action_mask, omask, err_msg=f"mask of the other seat t={t}")
        acts = caller_actions(rng, mask, num_envs)
        done_before = ora.dones.astype(bool)
        skip = acts == so.ACTION_SKIP
        acted = ~done_before & ~skip
        ora.step(acts)
        obs, mask, agent, phase = ora.observe()
        odone, ostatus = ora.dones, ora.status
        byte_d = np.where(acted, np.where((acts >= 0) & (acts < 26), acts, -2), -1)  # include/skyjo_vec.h: -1 none applied, -2 out of range
        want = _record_bytes(obs, byte_d, mask, np.stack([agent, phase, odone, ostatus], axis=-1), _oracle_eplen(ora))
        ended = acted & odone.astype(bool)  # this step ended the episode: by its natural end or by an illegal action
        natural = ended & (ostatus == so.ST_OK)
        idx = np.flatnonzero(natural)
        osc = _oracle_scores(ora, idx)
        if t % 2 == 0:
            o = eng.step_host(acts)
            got = _record_bytes(o.observations, o.action, o.action_mask, np.stack([o.agent, o.phase, o.done, o.status], axis=-1), o.episode_steps)
            np.testing.assert_array_equal(got, want, err_msg=f"records of step_host t={t}")
        else:
            act_d.copy_(torch.from_numpy(acts))
            _lib.check(L.skyjo_vec_step_collect(eng._h, vp(act_d), vp(rec_d), vp(fr_d), vp(ee_d), eng._stream()))
            np.testing.assert_array_equal(rec_d.cpu().numpy()[:, :want.shape[-1]], want, err_msg=f"records of step_collect t={t}")
            np.testing.assert_array_equal(ee_d.cpu().numpy(), ended.astype(np.uint8), err_msg=f"episode_end t={t}")
            np.testing.assert_array_equal(fr_d.cpu().numpy(), np.where(ended[:, None], ora.rewards, 0.0), err_msg=f"final_rewards t={t}")
        rew, sc, done = eng.rewards_host()
        dn = odone.astype(bool)
        np.testing.assert_array_equal(done, odone, err_msg=f"done t={t}")
        np.testing.assert_array_equal(rew[dn], ora.rewards[dn], err_msg=f"rewards t={t}")
        np.testing.assert_array_equal(sc[idx], osc, err_msg=f"scores t={t}")
        for j, g in enumerate(idx[:2]):  # a few finished games, one at a time
            s = eng.get_state(int(g))
            assert s["is_terminated"] and s["done"]
            np.testing.assert_array_equal(s["final_score"], osc[j], err_msg=f"get_state final_score t={t} game {g}")
            np.testing.assert_array_equal(s["rewards"], ora.rewards[g], err_msg=f"get_state rewards t={t} game {g}")
            states += 1
        scored += len(idx)
        illegal_ends += int((ended & ~natural).sum())
        skipped += int((skip & done_before).sum())
    c, oc = eng.counters(), ora.counters()
    for key in ("steps", "episodes", "resets", "sum_len", "illegal"):
        assert c[key] == oc[key], (key, c[key], oc[key])
    print(f"{steps} steps: {scored} scored episode ends, {illegal_ends} illegal ones, {skipped} skips of a finished game, {states} get_state calls")
    assert scored >= min_scored and illegal_ends > 0 and states > 0 and c["episodes"] == scored and c["illegal"] == illegal_ends, (scored, illegal_ends, states, c)
    eng.close()
    return scored, illegal_ends, skipped


@pytest.mark.parametrize("ind", [True, False], ids=["indirect", "direct"])
@pytest.mark.parametrize("N", PLAYERS)
def test_caller_action_path_at_every_geometry(N, ind):
    _caller_path(N, ind, B, STEPS[N], 10)


@pytest.mark.parametrize("N", [7, 11])
def test_caller_action_path_above_four_tiles(N):
    """B = 321: six tiles.  Above four the host-style calls bring no raw export of the games back: get_state and rewards_host read the
    device copy.  The direct observation with 7 and 11 players: 104 + 32 -> 144 and 152 + 32 -> 192 bytes per record."""
    _caller_path(N, False, 321, STEPS[N], 10)
