"""CPU: the reference of the per-seat sums (tests/seat_stats_ref.py) tested on itself, and the case tables of
tests/test_gpu_seat_stats.py (tests/seat_stats_cases.py) held to their conditions - all with the oracle alone.

  1. ``check`` accepts the oracle's OWN per-game accumulators (``acc_score`` / ``acc_refunded``, summed down the games - another order
     than the log's) beside the plainly accumulated reward sums, in both regimes and under both drivers;
  2. ``check`` rejects each of seven restated index slips applied to ONE episode of a log, in both regimes;
  3. the exact regime's bit budget holds on every exact case: every addend a multiple of its unit, n * max|x| / unit < 2^53;
  4. every case of the GPU module meets ``seat_stats_ref.conditions``; the printed counts are the tables of EXPERIMENTS.md.
"""
import numpy as np
import pytest

from tests import seat_stats_cases as sc
from tests import seat_stats_ref as ssr


def _oracle_counters(log, N):
    c = ssr.naive_counters(log, N)
    score, refunded = log.ora.seat_sums()
    c["sum_score"], c["sum_refunded"] = np.array(score), np.array(refunded)
    oc = log.ora.counters()
    c["episodes"], c["illegal"] = oc["episodes"], oc["illegal"]
    return c


def _report(name, log, N, figures):
    print(f"{name}: {'exact' if log.exact else 'bound'} regime, {figures['natural']} natural ends ({figures['penalised']} with a penalised "
          f"finisher), {figures['illegal']} illegal ends, {log.iteration} iterations")


# ----------------------------------------------------------------------------------------------------------------- 1. accepts
@pytest.mark.parametrize("N", [1, 2, 3, 4, 8, 11])
def test_check_accepts_the_oracles_own_accumulators(N):
    for driver in ("policy", "caller", "caller without auto-reset"):
        if driver == "policy":
            log = sc.rollout_log(N, N % 2, 300 + 60 * N)
        else:
            log, _ = sc.caller_log(N, True, driver == "caller", 200 + 40 * N)
        assert log.exact == (N in (1, 2, 4, 8))
        nat, ill = ssr.counts(log)
        assert nat > 0 and (driver == "policy") == (ill == 0), (driver, nat, ill)
        used = ssr.check(_oracle_counters(log, N), log, N)
        assert set(used) == set(ssr.KINDS) and all(0.0 <= u <= 1.0 for u in used.values())
        if log.exact:
            assert not any(used.values())


def test_steps_and_skips_of_finished_games_are_no_episode():
    """Without auto-reset a finished game stays done: SKYJO_ST_NOOP_DONE steps and skips of it add no entry; under auto-reset a game
    stands done for one iteration, so the entries equal the oracle's own counts."""
    log, acts = sc.caller_log(3, True, False, 400)
    nat, ill = ssr.counts(log)
    assert nat + ill == sc.B == len({e.game for e in log.entries})
    oc = log.ora.counters()
    assert (oc["episodes"], oc["illegal"]) == (nat, ill)
    before = len(log.entries)
    for _ in range(5):
        log.step(np.where(np.arange(sc.B) % 2 == 0, 24, ssr.so.ACTION_SKIP))
    assert len(log.entries) == before and (log.ora.status[::2] == ssr.so.ST_NOOP_DONE).all()
    log2 = sc.rollout_log(3, 0, 500)
    oc = log2.ora.counters()
    assert ssr.counts(log2) == (oc["episodes"], 0) and oc["episodes"] > 3 * sc.B


# ----------------------------------------------------------------------------------------------------------------- 2. rejects
@pytest.mark.parametrize("slip", ssr.SLIPS)
@pytest.mark.parametrize("N", [2, 3, 8, 12])
def test_check_rejects_a_restated_slip_in_one_episode(N, slip):
    log, _ = sc.caller_log(N, False, True, 200 + 60 * N)
    ssr.check(ssr.naive_counters(log, N), log, N)  # (the unslipped sums pass)
    with pytest.raises(AssertionError):
        ssr.check(ssr.slipped_counters(log, N, slip), log, N)


def test_check_rejects_wrong_integer_counters_and_an_unfit_exact_log():
    log = sc.rollout_log(2, 0, 300)
    c = ssr.naive_counters(log, 2)
    for key in ("episodes", "illegal"):
        with pytest.raises(AssertionError):
            ssr.check(dict(c, **{key: c[key] + 1}), log, 2)
    # a reward that is no multiple of 2^-10 does not belong in the exact regime: refused, not compared
    e = log.entries[0]
    bad = log.with_entries([e._replace(rewards=(e.rewards[0] + 2.0 ** -30, e.rewards[1]))] + log.entries[1:])
    with pytest.raises(AssertionError, match="exact regime"):
        ssr.check(ssr.naive_counters(bad, 2), bad, 2, exact=True)


# ----------------------------------------------------------------------------------------------------------------- 3. + 4. the cases
def _assert_budget(log, N):
    """The exact regime's bit budget, from the log: max |x| and the count per sum kind."""
    assert log.exact
    for kind, (multiple, need) in ssr.exact_budget(log, N).items():
        assert multiple and need < 2.0 ** 53, (kind, multiple, need)
    add = ssr.addends(log, N)
    biggest = max(abs(x) for xs in add["sum_reward"] for x in xs)
    count = max(len(xs) for xs in add["sum_reward"])
    assert biggest < 2.0 ** 10 and count * biggest ** 2 * 2.0 ** 20 < 2.0 ** 53, (biggest, count)  # the docstring's a-priori bounds


@pytest.mark.parametrize("N", sc.PLAYERS)
def test_fused_rollout_cases_meet_their_conditions(N):
    for rng_mode in (0, 1):
        log = sc.rollout_log(N, rng_mode, sc.ITERS[N])
        _report(f"fused rollout N={N} {'philox' if rng_mode else 'mt19937'}", log, N, ssr.conditions(log, N, sc.B))
        assert ssr.counts(log)[1] == 0  # the on-device policy makes no illegal move
        a, b = sc.slicing_a(sc.ITERS[N]), sc.slicing_b(sc.ITERS[N])
        assert sum(a) == sum(b) == sc.ITERS[N] and a[0] % 32 == 0 and a[1] % 32 != 0
        assert sc.ends_in_last_iteration_of_short_launches(log, a) >= 1
        if log.exact:
            _assert_budget(log, N)
    assert log.exact == (N in (1, 2, 4, 8))


@pytest.mark.parametrize("N", [2, 3])
def test_dry_bank_cases_meet_their_conditions(N):
    for rng_mode in (0, 1):
        log = sc.rollout_log(N, rng_mode, sc.DRY_ITERS[N])
        _report(f"banks run dry N={N} {'philox' if rng_mode else 'mt19937'}", log, N, ssr.conditions(log, N, sc.B))
        per_game = np.bincount([e.game for e in log.entries], minlength=sc.B)
        assert len(log.entries) >= 5 * sc.B and per_game.max() > 4  # more episodes than the seeding deals ahead: a game deals in place
        if log.exact:
            _assert_budget(log, N)


@pytest.mark.parametrize("auto_reset", [True, False], ids=["auto_reset", "no_auto_reset"])
@pytest.mark.parametrize("N", sc.PLAYERS)
def test_caller_action_cases_meet_their_conditions(N, auto_reset):
    for ind in (True, False):
        log, acts = sc.caller_log(N, ind, auto_reset)
        figures = ssr.conditions(log, N, sc.B, auto_reset=auto_reset, caller=True)
        _report(f"caller actions N={N} {'indirect' if ind else 'direct'} auto_reset={auto_reset}", log, N, figures)
        skip = acts == ssr.so.ACTION_SKIP
        assert skip.any() and (((acts < 0) | (acts > 25)) & ~skip).any()  # skips, and actions out of range among the illegal ones
        if not auto_reset:  # steps and skips of finished games
            assert (log.ora.status == ssr.so.ST_NOOP_DONE).any() and log.ora.dones.all()
        if log.exact:
            _assert_budget(log, N)


@pytest.mark.parametrize("N", [2, 3])
def test_reduction_geometry_cases_meet_their_conditions(N):
    log = sc.rollout_log(N, (N + 1) % 2, sc.GEOM_ITERS[N], num_envs=sc.GEOM_B, seed=sc.GEOM_SEED[N], threads=8)
    _report(f"reduction geometry N={N}", log, N, ssr.conditions(log, N, sc.GEOM_B))
    assert (sc.GEOM_B + 63) // 64 == 258 and sc.GEOM_B % 64 == 52 and sc.GEOM_ITERS[N] % 128 == 0
    assert np.bincount([e.game for e in log.entries], minlength=sc.GEOM_B).min() >= 2
    if log.exact:
        _assert_budget(log, N)
