#!/usr/bin/env python3
"""The tables of tests/seat_stats_cases.py, computed with the CPU oracle alone (no GPU):

    python tools/dev/seat_stats_tables.py

ITERS (fused rollout), DRY_ITERS (banks run dry), STEPS_ON / STEPS_OFF (caller actions), GEOM_ITERS (reduction geometry) as that file
defines them, printed as Python dicts, and per case the counts of natural and illegal ends the choice rests on."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from tests import seat_stats_cases as sc  # noqa: E402
from tests import seat_stats_ref as ssr  # noqa: E402


def _met(log, N, num_envs, **kw):
    try:
        return ssr.conditions(log, N, num_envs, **kw)
    except AssertionError:
        return None


def rollout_iters(N, factor=3, limit=40000):
    need = 0
    for rng_mode in (0, 1):
        log = sc.new_log(sc.B, sc.config(N, True, True, rng_mode), sc.SEED[N])
        while log.iteration < limit:
            log.rollout(8, sc.POLICY_SEED)
            if len(log.entries) >= factor * sc.B and _met(log, N, sc.B):
                break
        need = max(need, log.iteration)
    return need


def caller_steps(N, auto_reset, limit=40000):
    need = 0
    for ind in (True, False):
        log = sc.new_log(sc.B, sc.config(N, ind, auto_reset), 40 + N)
        rng = np.random.default_rng(1000 + N)
        while log.iteration < limit:
            for _ in range(10):
                _, mask, _, _ = log.ora.observe()
                log.step(sc.caller_actions(rng, mask, sc.B, sc.SHARE[N]))
            if _met(log, N, sc.B, auto_reset=auto_reset, caller=True):
                break
        else:
            raise SystemExit(f"caller actions N={N} auto_reset={auto_reset} indirect={ind}: conditions not met in {limit} steps")
        need = max(need, log.iteration)
    return need + (0 if auto_reset else 20)


def geometry_iters(N, limit=4000):
    log = sc.new_log(sc.GEOM_B, sc.config(N, True), sc.GEOM_SEED[N])
    per_game = np.zeros(sc.GEOM_B, dtype=np.int64)
    seen = 0
    while log.iteration < limit:
        log.rollout(128, sc.POLICY_SEED, threads=8)
        for e in log.entries[seen:]:
            per_game[e.game] += 1
        seen = len(log.entries)
        if per_game.min() >= 2:
            return log.iteration, seen
    raise SystemExit("reduction geometry: not every game ended twice")


def main():
    iters, dry, on, off = {}, {}, {}, {}
    for N in sc.PLAYERS:
        iters[N] = (rollout_iters(N) + 72 + 7) // 8 * 8
        on[N], off[N] = caller_steps(N, True), caller_steps(N, False)
        print(f"N={N}: ITERS {iters[N]}, STEPS_ON {on[N]}, STEPS_OFF {off[N]}", flush=True)
    for N in (2, 3):
        dry[N] = (rollout_iters(N, factor=5) + 99) // 100 * 100
    geom = {}
    for N in (2, 3):
        geom[N], episodes = geometry_iters(N)
        print(f"reduction geometry N={N}: {geom[N]} iterations, {episodes} episodes")
    print("ITERS =", iters)
    print("DRY_ITERS =", dry)
    print("STEPS_ON =", on)
    print("STEPS_OFF =", off)
    print("GEOM_ITERS =", geom)


if __name__ == "__main__":
    main()
