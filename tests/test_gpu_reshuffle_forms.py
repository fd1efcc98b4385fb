"""Mid-game reshuffles at two to four players in every rollout form, against the oracle (tests/pile_inject.py: what is injected and
what is compared; tests/test_pile_inject.py: the oracle's reshuffle against numpy, and that every injected game does reshuffle inside
the compared iterations).

Uninjected random play never reshuffles at these player counts, so the forms the benchmark and the training loop use had never run
reshuffle_dispatch (csrc/skyjo_transition.h): the step kernels with a compile-time player count under the on-device policy (deferred
scoring, register accumulators, the rare paths' scratch aliasing the record staging area), the tile-planar record path, the
one-kernel form - whose step wavefront waits for, rolls back and cancels a deal made by a dealing wavefront of its own workgroup,
inside a launch of several dealing cycles -, the two-stream forms, and counter-based reshuffle sessions beyond the first of an
episode.  Every case: ~100 compared warm-up iterations, then twice [reset of all games -> injection into all games -> ONE rollout call
of 48 (near-empty) or 96 (thin) iterations], every record of every iteration, the full piles of every game afterwards, the counters
(reshuffles included), rewards and scores of the games that stand finished, and a clean skyjo_vec_check_error.
"""
import ctypes as C

import numpy as np
import pytest

from tests import pile_inject as pi

pytestmark = pytest.mark.gpu
FORMS = {"in line": 0, "two streams": 2, "one kernel": 3}


def _pair(N, rng_mode, ind, B, form, interval, opts=None, layout="row-major"):
    from oracle import skyjo_oracle as so
    from skyjo_rl_amd import SkyjoVecEnv, _lib

    cfg = pi.oracle_config(N, rng_mode, ind)
    eng = SkyjoVecEnv(B, **cfg)
    opts = dict(opts or {})
    if "cycle_s" in opts:
        eng.set_option(_lib.OPT_CYCLE_S, opts.pop("cycle_s"))  # (before the engine is seeded)
    eng.set_deal_interval(interval)
    eng.set_overlap(FORMS[form])
    ids = {"work_list": _lib.OPT_INLINE_WORK_LIST, "unpipelined": _lib.OPT_UNPIPELINED, "max_cycles": _lib.OPT_MAX_CYCLES_PER_LAUNCH}
    for k, v in opts.items():
        eng.set_option(ids[k], v)
    assert eng.dealing_form() == form, (eng.dealing_form(), form)
    if layout != "row-major":
        eng.set_record_layout(layout)
        assert eng.record_layout == layout and eng.dealing_form() == form
    return eng, so.OracleVec(num_envs=B, **cfg)


def _check_round(name, B, r, st, waits_before):
    """What the comparison itself does not say: the reshuffles the segment covered, the clean device error, the in-place deals."""
    e, o = st["eng"], st["seg"]
    assert e["error"] is None, (name, e["error"])
    covered = e["counters"]["reshuffles"] - int(o["resh_before"].sum())  # (the segment and the iteration after it)
    assert covered == o["counters"]["reshuffles"] - int(o["resh_before"].sum()) and covered >= st["total"] >= B, (name, r, covered, st["total"])
    print(f"{name} round {r}: {covered} reshuffles ({st['min_per_game']} .. {int(st['per_game'].max())} per game, at most {st['max_in_episode']} inside an "
          f"episode), {st['finished']} games stand finished, {st['redealt_after_rollback']} dealt again after a reshuffle, waits {waits_before} -> {e['waits']}")


@pytest.mark.parametrize("name", list(pi.ROLLOUT_CASES))
def test_reshuffles_in_every_rollout_form(name):
    N, rng_mode, ind, B, family, form, interval, opts, layout = pi.ROLLOUT_CASES[name]
    eng, ora = _pair(N, rng_mode, ind, B, form, interval, opts, layout)
    waits = [0]
    must_wait = [False]

    def on_segment(r, st):
        _check_round(name, B, r, st, waits[-1])
        waits.append(st["eng"]["waits"])
        # in line at an interval the run never reaches, nothing refills a bank inside a segment: an MT19937 game whose roll-back
        # emptied its bank and which is dealt again afterwards (the oracle's records say so) is dealt in place - every such game
        if interval == 1000 and rng_mode == pi.MT and st["redealt_after_rollback"] > 0:
            must_wait[0] = True
            assert waits[-1] - waits[-2] >= st["redealt_after_rollback"] > 0, (name, r, st["redealt_after_rollback"], waits)

    rounds = pi.play(ora, family, eng=eng, on_segment=on_segment)
    assert len(rounds) == 2
    if family == "thin" and rng_mode == pi.PHILOX:
        assert min(st["max_in_episode"] for st in rounds) >= 3  # the sessions (episode, H_RESH = 1) and (episode, 2) were compared
    print(f"{name}: waits {waits}" + (" (asserted: at least one per game dealt again after a roll-back)" if must_wait[0] else " (recorded)"))
    eng.close()


@pytest.mark.parametrize("name", list(pi.CALLER_CASES))
def test_reshuffles_under_caller_actions(name):
    """The same injection stepped with step_host - the POLICY = false kernel with a compile-time player count: actions from the oracle's
    mask (the draw pile whenever it is legal); status, done, observation and mask of every step, the piles at the end."""
    N, rng_mode, ind, family, form = pi.CALLER_CASES[name]
    B = pi.CALLER_GAMES
    eng, ora = _pair(N, rng_mode, ind, B, form, 8)

    def after_step(t, acts, ended):
        o = eng.step_host(acts)
        obs, mask, agent, phase = ora.observe()
        np.testing.assert_array_equal(o.status, ora.status, err_msg=f"status t={t}")
        np.testing.assert_array_equal(o.done, ora.dones, err_msg=f"done t={t}")
        np.testing.assert_array_equal(o.observations, obs, err_msg=f"observations t={t}")
        np.testing.assert_array_equal(o.action_mask, mask, err_msg=f"masks t={t}")
        np.testing.assert_array_equal(o.agent, agent, err_msg=f"agent t={t}")
        np.testing.assert_array_equal(o.phase, phase, err_msg=f"phase t={t}")

    per_game, deepest, ends = pi.play_caller(ora, family, pi.CALLER_STEPS, after_step=after_step, eng=eng)
    assert per_game.min() >= 1
    for g in range(B):
        s, want = eng.get_state(g), pi.oracle_state(ora, g)
        np.testing.assert_array_equal(s["draw"], want["draw"], err_msg=f"draw pile of game {g}")
        np.testing.assert_array_equal(s["disc"], want["disc"], err_msg=f"discard pile of game {g}")
        assert s["reshuffles"] == want["reshuffles"], (g, s["reshuffles"], want["reshuffles"])
    c, oc = eng.counters(), ora.counters()
    for k in pi.COUNTERS:
        assert c[k] == oc[k], (k, c[k], oc[k])
    assert c["reshuffles"] == int(per_game.sum()) >= B
    eng.check_error()
    print(f"{name}: {c['reshuffles']} reshuffles, at most {deepest} inside an episode")
    eng.close()


def test_episode_end_columns_of_games_that_reshuffle():
    """skyjo_vec_step_collect in a device loop - the step kernel of skyjo_vec_model_rollout, where training meets reshuffles: episode_end
    and final_rewards of every step against the oracle's dones and rewards (the actions turn hidden cards over, so episodes end)."""
    import torch
    from skyjo_rl_amd import _lib

    N, rng_mode, ind, family, B, steps = pi.COLLECT_CASE
    eng, ora = _pair(N, rng_mode, ind, B, "in line", 8)
    L = eng._L
    rec = eng.new_records()
    act = torch.empty(B, dtype=torch.int32, device="cuda")
    fr = torch.empty((B, N), dtype=torch.float64, device="cuda")
    ee = torch.empty(B, dtype=torch.uint8, device="cuda")
    vp = lambda t: C.c_void_p(t.data_ptr())
    seen = [0]

    def after_step(t, acts, ended):
        act.copy_(torch.from_numpy(acts))
        _lib.check(L.skyjo_vec_step_collect(eng._h, vp(act), vp(rec), vp(fr), vp(ee), eng._stream()))
        np.testing.assert_array_equal(ee.cpu().numpy(), ended.astype(np.uint8), err_msg=f"episode_end t={t}")
        np.testing.assert_array_equal(fr.cpu().numpy(), np.where(ended[:, None], ora.rewards, 0.0), err_msg=f"final_rewards t={t}")
        v = eng.split(rec)
        obs, mask, agent, phase = ora.observe()
        np.testing.assert_array_equal(v.observations.cpu().numpy(), obs, err_msg=f"observations t={t}")
        np.testing.assert_array_equal(v.action_mask.cpu().numpy(), mask, err_msg=f"masks t={t}")
        np.testing.assert_array_equal(v.done.cpu().numpy(), ora.dones, err_msg=f"done t={t}")
        np.testing.assert_array_equal(v.status.cpu().numpy(), ora.status, err_msg=f"status t={t}")
        seen[0] += int(ended.sum())

    per_game, deepest, ends = pi.play_caller(ora, family, steps, after_step=after_step, reveal=True, eng=eng)
    assert per_game.min() >= 1 and ends == seen[0] > 0
    c, oc = eng.counters(), ora.counters()
    for k in pi.COUNTERS:
        assert c[k] == oc[k], (k, c[k], oc[k])
    eng.check_error()
    print(f"step_collect: {ends} episode ends, {c['reshuffles']} reshuffles")
    eng.close()


@pytest.mark.parametrize("name", list(pi.SNAPSHOT_CASES))
def test_snapshot_carries_a_bank_that_a_roll_back_has_emptied(name):
    """After the first compared segment (every game has reshuffled: its banked deals were taken back, some are being dealt again):
    snapshot, 60 iterations, restore, the same 60 iterations - the actions equal the first run's and the oracle's."""
    import torch

    N, rng_mode, ind, B, family, form, interval = pi.SNAPSHOT_CASES[name]
    eng, ora = _pair(N, rng_mode, ind, B, form, interval)
    (st,) = pi.play(ora, family, eng=eng, rounds=1)
    _check_round(name, B, 0, st, 0)
    K = 60
    snap = eng.snapshot()
    runs = []
    for _ in range(2):
        act = torch.empty((K, B), dtype=torch.int32, device="cuda")
        eng.rollout(K, policy_seed=pi.POLICY_SEED, actions=act)
        runs.append(act.cpu().numpy())
        if not runs[1:]:
            eng.restore(snap)
    want = ora.rollout(K, pi.POLICY_SEED, record_actions=True)
    np.testing.assert_array_equal(runs[0], want, err_msg="the run after the snapshot")
    np.testing.assert_array_equal(runs[1], want, err_msg="the run after the restore")
    obs, mask, agent, phase = ora.observe()
    o = eng.observe_host()
    np.testing.assert_array_equal(o.observations, obs)
    np.testing.assert_array_equal(o.action_mask, mask)
    c, oc = eng.counters(), ora.counters()
    for k in pi.COUNTERS:
        assert c[k] == oc[k], (k, c[k], oc[k])
    eng.check_error()
    snap.close()
    eng.close()
