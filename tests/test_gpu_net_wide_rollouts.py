"""Model rollouts whose episodes END, at the player counts where the step behind a net is the generic-N kernel: boards one or two actions
from the end (tests/board_inject.py: ``brink_only``) go into every game of an engine and of the oracle, then

  1. ``rollout.collect`` with a freshly initialised model plays BRINK_T iterations: every record, ``episode_end`` and ``final_rewards`` ==
     the oracle's stepped under the buffer's actions, the games dealt again after an end included (auto_reset) - two, five and twelve
     players on the direct observation (43, 79, 163 inputs), five on the indirect one.  At least a quarter of the games end inside the
     buffer; tests/test_net_wide_ref.py shows without a GPU that the oracle's random policy reaches twice that on the same boards.
  2. ``arena.collect`` with mixed seats - three policy nets, two value nets, a seat without one, greedy and random seats - at twelve
     players direct and five indirect: the six columns are the bits of the per-iteration composition (``arena.act``, then
     ``skyjo_vec_step_collect``), the records the oracle's; ``compute_targets``, ``select_rows(seats=(N - 1,))`` and
     ``arena.episode_stats`` on that buffer against their numpy references and the oracle's episode log.
"""
import ctypes as C
import math

import numpy as np
import pytest

from tests import board_inject as bi, net_wide_ref as wref, pile_inject as pi
from tests.test_gpu_net_wide import COLUMNS, _cfg, _column, records_against_the_oracle

pytestmark = pytest.mark.gpu

B, T, SEED = wref.BRINK_GAMES, wref.BRINK_T, wref.BRINK_SEED
DRAW_SEED, TICKET0 = 8, 1000


def _ids(cases):
    return ["N%d_%s" % (n, "ind" if i else "dir") for n, i in cases]


def _brink_pair(N, indirect):
    """An engine and an oracle seeded alike with a brink board in every game (pile_inject.inject asserts that both stand on one deal)."""
    from oracle import skyjo_oracle as so
    from skyjo_rl_amd import SkyjoVecEnv

    env, ora = SkyjoVecEnv(B, **_cfg(N, indirect)), so.OracleVec(num_envs=B, **_cfg(N, indirect))
    assert env.obs_dim == ora.obs_dim == (31 if indirect else 19 + 12 * N)
    env.seed(None, SEED), ora.seed(None, SEED)
    injected = pi.inject(bi.brink_only, np.random.default_rng(SEED), ora, env)
    assert len(injected) == B
    return env, ora


def _model_nets(N, indirect, seed, policy=True, value=True):
    import torch
    from skyjo_rl_amd.action_mask_model import ActionMaskModel, FusedNet

    torch.manual_seed(seed)
    model = ActionMaskModel(obs_dim=31 if indirect else 19 + 12 * N).cuda()
    return (FusedNet(model.policy) if policy else None), (FusedNet(model.value) if value else None)


# ---------------------------------------------------------------- 1. collect on the brink
@pytest.mark.parametrize("N,indirect", wref.BRINK_CASES, ids=_ids(wref.BRINK_CASES))
def test_collect_on_brink_boards_holds_the_oracles_episode_ends(N, indirect):
    from skyjo_rl_amd.rollout import RolloutBuffer, collect

    env, ora = _brink_pair(N, indirect)
    pol, val = _model_nets(N, indirect, 40 + N)
    buf = RolloutBuffer(env, T)
    collect(env, pol, val, buf, seed=DRAW_SEED, first_ticket=TICKET0)
    ends, ended = records_against_the_oracle(env, buf, ora, whole_rewards=True)
    again = int((buf.views().status[1:] == pi.ST_RESET).sum())
    print("brink collect N=%d %s: %d of %d games end inside %d iterations, %d episode ends, %d records of a game dealt again"
          % (N, "indirect" if indirect else "direct", int(ended.sum()), B, T, ends, again))
    assert int(ended.sum()) >= wref.BRINK_SHARE * B and ends == int(buf.episode_end.sum())
    assert again > 0                                            # the re-dealt games' records were compared as well
    c, oc = env.counters(), ora.counters()
    assert c["illegal"] == 0 and all(c[k] == oc[k] for k in ("steps", "episodes", "resets"))
    env.check_error()
    pol.close(), val.close(), env.close()


# ---------------------------------------------------------------- 2. mixed seats
MIXED_CASES = ((12, False), (5, True))
# seat -> (kind, policy net), value net: three policy nets, two value nets, seat 3 without a value, greedy and random seats
SEAT_PATTERN = [("sample", 0), ("greedy", 1), "random", ("sample", 2), ("greedy", 0), ("sample", 1), "random", ("greedy", 2), ("sample", 0), "random",
                ("sample", 2), ("greedy", 1)]
VALUE_PATTERN = [0, 1, 0, None, 1, 0, 1, 0, 1, 0, 1, 0]


def _mixed(N, indirect):
    nets = [_model_nets(N, indirect, 60 + i) for i in range(3)]
    pols, vals = [p for p, _ in nets], [v for _, v in nets[:2]]
    nets[2][1].close()
    seats = [s if isinstance(s, str) else (s[0], pols[s[1]]) for s in SEAT_PATTERN[:N]]
    values = [None if v is None else vals[v] for v in VALUE_PATTERN[:N]]
    assert len({id(s[1]) for s in seats if not isinstance(s, str)}) == 3 and len({id(v) for v in values if v is not None}) == 2
    assert values.count(None) == 1 and "random" in seats and any(s[0] == "greedy" for s in seats if not isinstance(s, str))
    return seats, values, pols + vals


@pytest.mark.parametrize("N,indirect", MIXED_CASES, ids=_ids(MIXED_CASES))
def test_arena_collect_with_mixed_seats_on_brink_boards(N, indirect):
    import torch
    from skyjo_rl_amd import _lib, arena
    from skyjo_rl_amd.rollout import RolloutBuffer, compute_targets, select_rows
    from tests import arena_ref, rollout_batches_ref as rbr, rollout_targets_ref as tref, seat_stats_ref as ssr

    seats, values, nets = _mixed(N, indirect)
    env, ora = _brink_pair(N, indirect)
    twin, _ = _brink_pair(N, indirect)
    got, want = RolloutBuffer(env, T), RolloutBuffer(twin, T)
    for b in (got, want):                                       # (every byte the calls must write starts out different)
        b.logp.fill_(7.0), b.values.fill_(-7.0), b.actions.fill_(-5)
    assert arena.collect(env, seats, values, got, seed=DRAW_SEED, first_ticket=TICKET0) is got
    # the per-iteration composition on the twin: arena.act, then the engine's step
    L = _lib.load()
    vp = lambda t: C.c_void_p(t.data_ptr())
    sp, vn = arena.seat_policies(twin, seats), arena.value_nets(twin, values)
    twin.observe(out=want.records[0])
    for t in range(T):
        arena.act(twin, sp, vn, want.records[t], seed=DRAW_SEED, ticket=TICKET0 + t, actions=want.actions[t], logp=want.logp[t], values_out=want.values[t])
        _lib.check(L.skyjo_vec_step_collect(twin._h, vp(want.actions[t]), vp(want.records[t + 1]), vp(want.final_rewards[t]), vp(want.episode_end[t]),
                                            twin._stream()))
    arena.act(twin, sp, vn, want.records[T], seed=DRAW_SEED, ticket=TICKET0 + T, values_out=want.values[T], values_only=True)
    for name in COLUMNS:
        a, b = _column(got, name), _column(want, name)
        assert a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8)), name
    # the oracle under the buffer's actions, with the log of the episodes that end
    log = ssr.EpisodeLog(ora)
    ends, ended = records_against_the_oracle(env, got, ora, step=log.step, whole_rewards=True)
    agent = got.views().agent.cpu().numpy()
    valid = got.valid.cpu().numpy()
    acted = [int(((agent[:T] == s) & valid).sum()) for s in range(N)]
    print("mixed N=%d %s: %d of %d games end, %d episode ends; rows per seat %s" % (N, "indirect" if indirect else "direct", int(ended.sum()), B, ends, acted))
    assert int(ended.sum()) >= wref.BRINK_SHARE * B and min(acted) > 0 and env.counters()["illegal"] == 0
    assert ends == len(log.entries) and all(e.kind == ssr.NATURAL for e in log.entries)
    # a seat without a value net holds 0.0 in its rows, a random seat - log(legal count)
    vals = got.values[:T, :, 0].cpu().numpy()
    none_seat = VALUE_PATTERN.index(None)
    assert (vals.view(np.uint32)[agent[:T] == none_seat] == 0).all() and (vals[agent[:T] != none_seat] != 0).any()
    mask = got.views().action_mask[:T].cpu().numpy()
    lp = got.logp.cpu().numpy()
    rnd = np.isin(agent[:T], [s for s in range(N) if seats[s] == "random"]) & valid
    assert rnd.sum() > 0 and np.abs(lp[rnd] + np.log(mask[rnd].sum(1))).max() <= 1e-5 + 4 * 2.0 ** -24 * np.log(26)
    # targets: the float32 recursion over twelve (five) seats
    cols = tref.columns_from_buffer(got)
    for gamma, lam in ((0.99, 0.95), (1.0, 1.0)):
        compute_targets(got, gamma=gamma, lam=lam)
        ref_cols = tref.targets_f32(gamma=gamma, lam=lam, **cols)
        for name, x, w in zip(("advantages", "value_targets", "returns", "flags"), (got.advantages, got.value_targets, got.returns, got.target_flags), ref_cols):
            x, w = x.cpu(), torch.from_numpy(w)
            same = torch.equal(x.view(torch.int32), w.view(torch.int32)) if x.dtype == torch.float32 else torch.equal(x, w)
            assert x.shape == w.shape and same, (name, gamma, lam)
    # the last seat's rows
    flags, adv = got.target_flags.cpu().numpy().reshape(-1), got.advantages.cpu().numpy().reshape(-1)
    sel = select_rows(got, seats=(N - 1,))
    index = rbr.select(flags, _lib.TGT_HAS_TARGET)
    index = index[agent[:T].reshape(-1)[index] == N - 1]
    assert sel.count == index.size > 0 and np.array_equal(sel.index.cpu().numpy(), index)
    mean, std = rbr.mean_std(*rbr.moments(adv, index), index.size)
    assert abs(sel.mean - mean) <= 1e-9 and abs(sel.std - std) <= 1e-9
    assert sum(select_rows(got, seats=(s,)).count for s in range(N)) == select_rows(got).count
    # the episodes that ended: per seat against the oracle's log (a mean is a sum within (n - 1) 2^-53 sum |x| of fsum, divided by n)
    st = arena.episode_stats(got)
    n = len(log.entries)
    add = ssr.addends(log, N)
    fr, ee = got.final_rewards.cpu().numpy(), got.episode_end.cpu().numpy()
    _, _, ref_std, ref_win = arena_ref.episode_stats(fr, ee)
    assert st.episodes == n
    for s in range(N):
        xs = add["sum_reward"][s]
        assert len(xs) == n
        want_mean = math.fsum(xs) / n
        assert abs(st.mean_reward[s] - want_mean) <= (n - 1) * 2.0 ** -53 * math.fsum(abs(x) for x in xs) / n + 2.0 ** -52 * abs(want_mean), s
        wins = sum(e.rewards[s] == max(e.rewards) for e in log.entries)
        assert st.win_rate[s] == wins / n == ref_win[s], s
        assert math.isclose(st.std_reward[s], ref_std[s], rel_tol=1e-9, abs_tol=0.0), s
    used = ssr.check(env.counters(), log, N)                    # the engine's own per-seat sums over the same episodes
    print("mixed N=%d: episode_stats over %d episodes; counters() allowance used %s" % (N, n, used))
    env.check_error()
    for net in nets:
        net.close()
    env.close(), twin.close()
