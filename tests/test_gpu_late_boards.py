"""Late boards in every form of the environment kernels, against the reference's recorded word and the oracle (tests/board_inject.py:
what is injected; tests/test_board_inject.py: what the injected games reach, on the oracle alone; tests/test_oracle_golden.py:
the oracle against tests/golden/late_boards_*.npz, which oracle/gen_golden.py recorded from the reference).

csrc/skyjo_transition.h keeps per seat the open-card sum, the hidden count and num_refunded in one packed word, the minima over seats,
a u8[15] histogram under dword LDS atomics, the visible-byte image and an 8-bit discard count - incrementally, in the place action, the
collapse branch, the reshuffle's histogram walk, set_state's rebuild, the deferred scoring and the dealing wavefront's reset.  Random
play never shows three refunded columns, so this file injects them:

  1. golden replay: every recorded board through step_host (observation and mask of both seats before each step, get_state after it,
     scores, metrics and rewards at the end); one board per player count also through step() with device records in both layouts;
  2. every action (-2 .. 28) from 40 boards of all three families in both phases, one step_host == the oracle: record, rewards, the
     state of every game, counters() - compile-time kernels (2, 3, 4 players) and generic ones (1, 5, 12);
  3. every rollout form from late boards: each record field, counters, rewards, scores, piles and the per-seat sums == the oracle's;
  4. step_collect's episode_end / final_rewards on the brink family, and snapshot -> play -> restore -> play.
"""
import ctypes as C
import glob
import os

import numpy as np
import pytest

from tests import board_inject as bi
from tests import pile_inject as pi

pytestmark = pytest.mark.gpu
FORMS = {"in line": 0, "two streams": 2, "one kernel": 3}
GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "late_boards_*.npz")))
REWARD_CFG = 0  # (1.0, 0.001): the engine's default


def _pair(N, rng_mode, ind, B, form, interval, opts=None, layout="row-major", auto_reset=True):
    from oracle import skyjo_oracle as so
    from skyjo_rl_amd import SkyjoVecEnv, _lib

    cfg = dict(pi.oracle_config(N, rng_mode, ind), auto_reset=auto_reset)
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


def _same_counters(eng, ora, tag):
    c, oc = eng.counters(), ora.counters()
    for k in pi.COUNTERS:
        assert c[k] == oc[k], (tag, k, c[k], oc[k])
    score, refunded = ora.seat_sums()  # integers times the penalty 2: exact
    np.testing.assert_array_equal(c["sum_score"], score, err_msg=f"{tag}: per-seat sum of final scores")
    np.testing.assert_array_equal(c["sum_refunded"], refunded, err_msg=f"{tag}: per-seat sum of num_refunded")
    return c


# ------------------------------------------------------------------------------------------ 1. the reference's recorded boards
LATE_STATE = ("n_draw", "n_disc", "top_draw", "top_disc", "hand", "player", "phase")


def _init(d, b):
    nd, ns = int(d["init_n_draw"][b]), int(d["init_n_disc"][b])
    return (d["init_cards"][b], d["init_masked"][b], d["init_draw"][b][:nd], d["init_disc"][b][:ns], int(d["init_hand"][b]),
            int(d["init_player"][b]), int(d["init_phase"][b]))


def _same_golden_state(s, d, prefix, t, tag):
    np.testing.assert_array_equal(s["cards"], d[prefix + "cards"][t], err_msg=f"{tag}: cards")
    np.testing.assert_array_equal(s["masked"], d[prefix + "masked"][t], err_msg=f"{tag}: masked")
    got = dict(s, top_draw=int(s["draw"][-1]) if s["n_draw"] else 99, top_disc=int(s["disc"][-1]) if s["n_disc"] else 99)
    assert tuple(got[k] for k in LATE_STATE) == tuple(int(d[prefix + k][t]) for k in LATE_STATE), (tag, [got[k] for k in LATE_STATE])


def _put(eng, games, d, b):
    for i in range(games):
        eng.set_state(i, *_init(d, b))
        if eng.rng_mode == 0:
            eng.seed_raw(i, int(d["np_seed"][b]))  # (a draw from an empty pile reshuffles on the reference's global stream)


def test_golden_late_board_files_are_all_there():
    """Six player counts in both observation modes: a missing or renamed file would only empty the parameter set below."""
    assert [os.path.basename(p) for p in GOLDEN] == sorted("late_boards_N%d_%s.npz" % (n, o) for n in (1, 2, 3, 4, 5, 12) for o in ("ind", "dir"))


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[12:-4] for p in GOLDEN])
def test_golden_late_boards(path):
    """test_golden_scenarios' scheme for every recorded board: a two-game engine, set_state, then the reference's own actions through
    step_host to the episode's end (the first board of a file also through step() with device records - row-major and, at two to four
    players, tile-planar -, unpacked with unpack / unpack_tiles); and every one of the 26 actions from a fresh copy of the board on a 26-game engine."""
    import torch
    from skyjo_rl_amd import SkyjoVecEnv

    d = dict(np.load(path))  # (every array once: an NpzFile decompresses at each access)
    N, ind = int(d["num_players"]), bool(d["indirect"])
    cfg = dict(num_players=N, score_penalty=float(d["score_penalty"]), observe_other_player_indirect=ind, auto_reset=False)
    eng, one = SkyjoVecEnv(2, **cfg), SkyjoVecEnv(26, **cfg)
    engines = [eng, one]
    runs = [("host", eng), ("row-major", eng)]
    if 2 <= N <= 4 and ind:  # (step writes tile-planar records at two to four players, of the indirect observation)
        engines.append(SkyjoVecEnv(2, **cfg))
        engines[-1].set_record_layout("tile-planar-all")
        runs.append(("tile-planar-all", engines[-1]))
    for e in engines:
        e.seed(None, 5)
    for b, name in enumerate(str(x) for x in d["names"]):
        for layout, eng in (runs if b == 0 else runs[:1]):
            device_records = layout != "host"
            _put(eng, 2, d, b)
            o = eng.observe_host()
            for t in range(int(d["step_start"][b]), int(d["step_start"][b + 1])):
                a, pid, over = int(d["actions"][t]), int(d["step_actor"][t]), int(d["step_over"][t])
                assert (o.agent[1], o.done[1]) == (pid, 0), (name, t)
                np.testing.assert_array_equal(o.observations[1], d["step_obs"][t], err_msg=f"{name} obs t={t}")
                np.testing.assert_array_equal(o.action_mask[1], d["step_mask"][t], err_msg=f"{name} mask t={t}")
                oo = eng.observe_host(np.full(2, (pid + 1) % N, dtype=np.int32))
                np.testing.assert_array_equal(oo.observations[0], d["step_obs_next"][t], err_msg=f"{name} next seat's obs t={t}")
                np.testing.assert_array_equal(oo.action_mask[0], d["step_mask_next"][t], err_msg=f"{name} next seat's mask t={t}")
                if device_records:
                    rec = eng.step(torch.full((2,), a, dtype=torch.int32, device="cuda"))
                    if layout == "row-major":
                        obs, mask = eng.unpack(rec)
                    else:
                        obs, mask = (x[:2] for x in eng.unpack_tiles(rec))
                        rec = eng.rows_from_planar(rec)
                    v = eng.split(rec)
                    obs, mask = obs.cpu().numpy(), mask.cpu().numpy()
                    assert (v.done.cpu().numpy() == over).all() and (v.status.cpu().numpy() == 0).all(), (name, t)
                    assert (v.action.cpu().numpy() == a).all(), (name, t)
                    if t + 1 < int(d["step_start"][b + 1]):  # the record a step writes is the next step's observation: the reference's
                        assert (v.agent.cpu().numpy() == d["step_actor"][t + 1]).all(), (name, t)
                        for i in range(2):
                            np.testing.assert_array_equal(obs[i], d["step_obs"][t + 1], err_msg=f"{name} device record's obs t={t}")
                            np.testing.assert_array_equal(mask[i], d["step_mask"][t + 1], err_msg=f"{name} device record's mask t={t}")
                    o = eng.observe_host()  # (after the last step there is no recorded observation: the engine's own, the terminal state)
                    np.testing.assert_array_equal(obs, o.observations, err_msg=f"{name} device record t={t}")
                    np.testing.assert_array_equal(mask, o.action_mask, err_msg=f"{name} device record t={t}")
                    if layout != "row-major":  # (unpack_tiles against the row-major copy of the same blocks)
                        np.testing.assert_array_equal(obs, v.observations.cpu().numpy(), err_msg=f"{name} unpack_tiles t={t}")
                        np.testing.assert_array_equal(mask, v.action_mask.cpu().numpy(), err_msg=f"{name} unpack_tiles t={t}")
                else:
                    o = eng.step_host(np.full(2, a, dtype=np.int32))
                    assert np.all(o.done == over) and np.all(o.status == 0), (name, t)
                _same_golden_state(eng.get_state(1), d, "step_", t, f"{name} t={t}")
            s = eng.get_state(0)
            assert s["is_terminated"] and s["done"], name
            np.testing.assert_array_equal(s["draw"], d["end_draw"][b][:int(d["end_n_draw"][b])], err_msg=f"{name}: draw pile at the end")
            np.testing.assert_array_equal(s["disc"], d["end_disc"][b][:int(d["end_n_disc"][b])], err_msg=f"{name}: discard pile at the end")
            np.testing.assert_array_equal(s["final_score"], d["final_score"][b], err_msg=name)
            np.testing.assert_array_equal(s["num_refunded"], d["num_refunded"][b], err_msg=name)
            np.testing.assert_array_equal(s["num_placed"], d["num_placed"][b], err_msg=name)
            np.testing.assert_array_equal(s["rewards"], d["rewards"][b][REWARD_CFG], err_msg=name)
            np.testing.assert_array_equal(eng.rewards_host()[0][1], d["rewards"][b][REWARD_CFG], err_msg=name)
        # every action from a fresh copy: the mask bit, and for the legal ones the successor
        _put(one, 26, d, b)
        legal = d["act_legal"][b]
        np.testing.assert_array_equal(one.observe_host().action_mask, np.tile(legal, (26, 1)), err_msg=f"{name}: mask")
        o = one.step_host(np.arange(26, dtype=np.int32))
        np.testing.assert_array_equal(o.status, np.where(legal != 0, 0, 1), err_msg=f"{name}: status of each action")
        k = int(d["act_start"][b])
        for a in np.flatnonzero(legal):
            s = one.get_state(int(a))
            _same_golden_state(s, d, "act_", k, f"{name} action {a}")
            assert bool(s["is_terminated"]) == bool(d["act_over"][k]) == bool(o.done[a]), (name, a)
            k += 1
        assert k == d["act_start"][b + 1]
    for e in engines:
        e.check_error()
        e.close()


# ------------------------------------------------------------------------------------------ 2. every action from every board
@pytest.mark.parametrize("name", list(bi.ACTION_CASES))
def test_every_action_from_every_board(name):
    """board_inject.every_action holds the whole case, the comparison included: 40 boards x 31 actions on one engine and one OracleVec;
    before the step observation, mask, agent and phase; after ONE step_host the record (observation, mask, agent, phase, done, status,
    action byte), rewards_host where done, get_state of all 1 240 games (boards, piles, hand, turn, num_refunded, num_placed, final
    scores), counters() with the per-seat sums, `illegal` = the number of zero mask bits; with auto_reset one more step, in which the
    finished games are dealt again - all == the oracle's."""
    N, rng_mode, ind, form, auto_reset = bi.ACTION_CASES[name]
    eng, ora = _pair(N, rng_mode, ind, bi.BOARDS * len(bi.ACTIONS), form, 8, auto_reset=auto_reset)
    n = bi.every_action(ora, bi.ACTION_SEED, ind, eng=eng)
    print(f"{name}: " + ", ".join(f"{k} {v}" for k, v in n.items() if v))
    eng.close()


# ------------------------------------------------------------------------------------------ 3. every rollout form
@pytest.mark.parametrize("name", list(bi.ROLLOUT_CASES))
def test_late_boards_in_every_rollout_form(name):
    N, rng_mode, ind, B, form, interval, opts, layout = bi.ROLLOUT_CASES[name]
    eng, ora = _pair(N, rng_mode, ind, B, form, interval, opts, layout)
    waits = [0]

    def on_segment(r, st):
        e = st["eng"]
        assert e["error"] is None, (name, e["error"])
        _same_counters(eng, ora, f"{name} round {r}")
        waits.append(e["waits"])

    rounds, n = bi.play(ora, ind, eng=eng, on_segment=on_segment)
    assert len(rounds) == 2
    print(f"{name}: " + ", ".join(f"{k} {v}" for k, v in n.items()) + f", waits {waits}")
    eng.close()


# ------------------------------------------------------------------------------------------ 4. callers that consume ends
def test_episode_end_columns_on_the_brink():
    """skyjo_vec_step_collect in a device loop on boards one or two actions from the end: episode_end and final_rewards of every step
    against the oracle's dones and rewards - penalty, negative penalty, tie, all-zero scores among them from the first steps on."""
    import torch
    from skyjo_rl_amd import _lib

    N, rng_mode, ind, B, steps = bi.COLLECT_CASE
    eng, ora = _pair(N, rng_mode, ind, B, "in line", 8)
    L = eng._L
    rec = eng.new_records()
    act = torch.empty(B, dtype=torch.int32, device="cuda")
    fr = torch.empty((B, N), dtype=torch.float64, device="cuda")
    ee = torch.empty(B, dtype=torch.uint8, device="cuda")
    vp = lambda t: C.c_void_p(t.data_ptr())
    seen, early = [0], [0]

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
        early[0] += int(ended.sum()) if t < 2 * N + 2 else 0

    per_game, deepest, ends = pi.play_caller(ora, bi.brink_only, steps, after_step=after_step, reveal=True, eng=eng)
    assert ends == seen[0] and early[0] >= B // 4, (ends, seen, early)  # (four of the seven kinds end at the acting seat's first draw)
    _same_counters(eng, ora, "step_collect")
    eng.check_error()
    print(f"step_collect: {ends} episode ends, {early[0]} of them within the injected boards' first turns")
    eng.close()


def test_snapshot_and_restore_on_late_boards():
    """After a board went into every game: snapshot, 60 iterations, restore, the same 60 iterations - records and actions of both runs
    equal each other and the oracle's."""
    import torch

    N, rng_mode, ind, B, form, interval = bi.SNAPSHOT_CASE
    eng, ora = _pair(N, rng_mode, ind, B, form, interval)
    ora.seed(None, pi.SEED), eng.seed(None, pi.SEED)
    ora.reset(), eng.reset_host()
    pi.inject(bi.mixed, np.random.default_rng(pi.INJECT_SEEDS[0]), ora, eng)
    K = 60
    snap = eng.snapshot()
    runs = []
    for _ in range(2):
        runs.append(pi.engine_segment(eng, K, pi.POLICY_SEED, range(0, B, 16), tail=0))
        if not runs[1:]:
            eng.restore(snap)
    want = pi.oracle_segment(ora, K, pi.POLICY_SEED, range(0, B, 16), tail=0)
    pi.assert_same(runs[0], want, "the run after the snapshot")
    pi.assert_same(runs[1], want, "the run after the restore")
    assert int(want["done"].sum()) > 0  # (finished games stood in the records)
    eng.check_error()
    snap.close()
    eng.close()
