"""The cases of tests/test_gpu_seat_stats.py as the CPU sees them (TEST INFRASTRUCTURE): settings, tables, launch slicings and the
oracle's episode logs.  tests/test_seat_stats_ref.py asserts - with the oracle alone - that every case meets the conditions the GPU
module relies on (seat_stats_ref.conditions); tools/dev/seat_stats_tables.py computes the tables.

Regimes (tests/seat_stats_ref.py).  N in {1, 2, 4, 8} runs under the EXACT settings and is compared with ``==``; every other N runs under
the inexact settings of tests/test_gpu_scoring_geometry.py and a non-default illegal reward, and is held to the derived bound.
B = 130 games: two full tiles and a tile of two lanes.  Generator: ``(N + indirect) % 2``, as in test_gpu_scoring_geometry.py - both
generators and both observations occur at every N; the observation does not change the play, so a log serves both.
"""
import functools

import numpy as np

from oracle import skyjo_oracle as so
from tests import seat_stats_ref as ssr

B = 130
POLICY_SEED = 77
PLAYERS = list(range(1, 13))
BOUND_SETTINGS = dict(score_penalty=1.0 / 3.0, mean_reward=0.1, reward_refunded=0.007, illegal_reward=-0.3)

# Fused rollout.  ITERS[N]: lockstep iterations (base seed SEED[N]) after which, under EITHER generator, the oracle has seen at least
# 3 B ended episodes, every seat as a finisher and every seat penalised - plus the 72 iterations of the stretch of launches of one
# and two iterations at the end of slicing_a, rounded up to a multiple of 8.  tools/dev/seat_stats_tables.py.
SEED = {N: 1 for N in PLAYERS}
ITERS = {1: 240, 2: 344, 3: 440, 4: 544, 5: 640, 6: 736, 7: 824, 8: 920, 9: 1032, 10: 1096, 11: 1192, 12: 1256}
# Banks run dry (deal interval 1000: nothing is dealt ahead after the seeding): iterations for 5 B ended episodes - more than the
# three episodes a game's bank holds.
DRY_ITERS = {2: 500, 3: 600}
# Caller actions (seed 40 + N, action stream 1000 + N as in test_gpu_scoring_geometry.py).  SHARE[N]: the share of arbitrary actions
# from -2 .. 28 (mostly illegal) per step - 0.2 % there, raised for up to four players so that every seat commits an illegal action.
# STEPS_ON[N] / STEPS_OFF[N]: steps with / without auto-reset after which the conditions hold (without: every game has ended, and
# twenty more steps on finished games), rounded up to a multiple of 10.
SHARE = {1: 0.004, 2: 0.004, 3: 0.004, 4: 0.004, 5: 0.002, 6: 0.002, 7: 0.002, 8: 0.002, 9: 0.002, 10: 0.002, 11: 0.002, 12: 0.002}
STEPS_ON = {1: 160, 2: 260, 3: 340, 4: 390, 5: 510, 6: 580, 7: 660, 8: 730, 9: 810, 10: 870, 11: 930, 12: 1000}
STEPS_OFF = {1: 160, 2: 170, 3: 210, 4: 230, 5: 280, 6: 300, 7: 370, 8: 370, 9: 440, 10: 420, 11: 430, 12: 480}
# Reduction geometry: 16 500 games = 258 tiles (more than one 256-thread workgroup of k_reduce_stats), the last of 52 games, with two
# (exact regime) and three players.  GEOM_ITERS[N]: iterations after which EVERY game has ended at least two episodes, rounded up to a
# multiple of 128.
GEOM_B, GEOM_SEED = 16500, {2: 2, 3: 1}  # (two players, base seed 1: both seats' refunded cards sum to 1 953 - a seat exchange would not show)
GEOM_ITERS = {2: 384, 3: 384}


def settings(N):
    return dict(ssr.EXACT_SETTINGS) if N in ssr.EXACT_PLAYERS else dict(BOUND_SETTINGS)


def config(N, ind, auto_reset=True, rng_mode=None, **over):
    """Keyword arguments of SkyjoVecEnv for a case."""
    cfg = dict(num_players=N, observe_other_player_indirect=bool(ind), rng_mode=(N + int(ind)) % 2 if rng_mode is None else rng_mode,
               auto_reset=auto_reset, **settings(N))
    cfg.update(over)
    return cfg


def new_log(num_envs, cfg, seed):
    """A seeded oracle for ``cfg`` (``config``'s result) behind an empty episode log."""
    cfg = dict(cfg)
    illegal_reward = cfg.pop("illegal_reward")
    ora = so.OracleVec(num_envs=num_envs, **cfg)
    ora.seed(None, seed)
    return ssr.EpisodeLog(ora, illegal_reward=illegal_reward)


@functools.lru_cache(maxsize=4)  # (the forms and slicings of one (N, generator) follow each other)
def rollout_log(N, rng_mode, iters, num_envs=B, seed=None, threads=1, auto_reset=True):
    log = new_log(num_envs, config(N, True, auto_reset, rng_mode), SEED[N] if seed is None else seed)
    log.rollout(iters, POLICY_SEED, threads=threads)
    return log


def slicing_a(total):
    """Launch lengths: two whole SK_SCORE_EVERY = 32 periods in one launch; a length that is no multiple of 32; launches of 96; then 24
    pairs of launches of ONE and TWO iterations, where every episode end of a one-iteration launch falls into a launch's last
    iteration (the deferred scoring's ``it == iters - 1`` service point)."""
    assert total >= 64 + 37 + 72, total
    out, rest = [64, 37], total - 64 - 37 - 72
    while rest > 0:
        out.append(min(96, rest))
        rest -= out[-1]
    return out + [1, 2] * 24


def slicing_b(total):
    """The same run cut elsewhere: 29 iterations, then launches of 160."""
    out, rest = [29], total - 29
    while rest > 0:
        out.append(min(160, rest))
        rest -= out[-1]
    return out


def ends_in_last_iteration_of_short_launches(log, slicing):
    """Episodes of ``log`` that ended in the LAST iteration of a launch of one or two iterations of ``slicing``."""
    last, at = set(), 0
    for k in slicing:
        at += k
        if k <= 2:
            last.add(at - 1)
    return sum(e.iteration in last for e in log.entries)


def caller_actions(rng, mask, n, share):
    from tests.test_gpu_scoring_geometry import caller_actions as ca

    return ca(rng, mask, n, share)


@functools.lru_cache(maxsize=2)
def caller_log(N, ind, auto_reset, steps=None):
    """The caller-action run of (N, observation, auto-reset) on the oracle: (log, the actions of every step [steps, B])."""
    log = new_log(B, config(N, ind, auto_reset), 40 + N)
    rng = np.random.default_rng(1000 + N)
    steps = (STEPS_ON if auto_reset else STEPS_OFF)[N] if steps is None else steps
    acts = np.zeros((steps, B), dtype=np.int32)
    for t in range(steps):
        _, mask, _, _ = log.ora.observe()
        acts[t] = caller_actions(rng, mask, B, SHARE[N])
        log.step(acts[t])
    return log, acts
