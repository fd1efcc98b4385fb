#!/usr/bin/env python3
"""The tables of tests/test_gpu_scoring_geometry.py, computed with the CPU oracle alone (no GPU):

    python tools/dev/scoring_geometry_tables.py

SEED / T (case 2), K_END (case 3), STEPS (case 4) as that file defines them, printed as Python dicts, and per N the counts the
choice rests on (finished games and order-sensitive means by T under either generator)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from oracle import skyjo_oracle as so  # noqa: E402
from tests import scoring_order_ref as ref  # noqa: E402
from tests import test_gpu_scoring_geometry as tg  # noqa: E402


def by_iteration(N, rng_mode, seed, auto_reset, limit):
    """Per iteration (one, then two at a time): finished episodes so far, order-sensitive means among them, games standing done."""
    ora = tg._oracle(tg.B, **tg._cfg(N, True, rng_mode, auto_reset))
    ora.seed(None, seed)
    total = sensitive = 0
    seen = np.zeros(tg.B, dtype=bool)
    while total < limit:
        k = 1 if total == 0 else 2
        ora.rollout(k, tg.POLICY_SEED)
        total += k
        done = ora.dones.astype(bool)
        new = done & ~seen if not auto_reset else done
        sensitive += sum(ref.order_sensitive(s) for s in tg._oracle_scores(ora, np.flatnonzero(new)))
        seen |= done
        yield total, ora.counters()["episodes"], sensitive, int(done.sum())


def case2(N):
    for seed in range(1, 200):
        t_need, sens = 0, []
        for rng_mode in (0, 1):
            for total, episodes, sensitive, _ in by_iteration(N, rng_mode, seed, True, 20000):
                if episodes >= tg.B:
                    break
            t_need = max(t_need, total)
        for rng_mode in (0, 1):
            for total, episodes, sensitive, _ in by_iteration(N, rng_mode, seed, True, t_need):
                pass
            sens.append((episodes, sensitive))
        if N < 8 or min(s for _, s in sens) >= 5:
            return seed, t_need, sens


def case3(N, seed):
    need, sens = 0, []
    for rng_mode in (0, 1):
        for total, episodes, sensitive, standing in by_iteration(N, rng_mode, seed, False, 100000):
            if standing == tg.B:
                break
        need = max(need, total)
        sens.append(sensitive)
    return (need + 63) // 64 * 64, sens


def case4(N, num_envs, min_scored=10, limit=20000):
    rng_mode_of = lambda ind: (N + int(ind)) % 2
    out = []
    for ind in (True, False):
        ora = tg._oracle(num_envs, **tg._cfg(N, ind, rng_mode_of(ind)))
        ora.seed(None, 40 + N)
        rng = np.random.default_rng(1000 + N)
        scored, per_step = 0, []
        for t in range(limit):
            _, mask, _, _ = ora.observe()
            acts = tg.caller_actions(rng, mask, num_envs)
            before = ora.counters()["episodes"]
            ora.step(acts)
            scored += ora.counters()["episodes"] - before
            per_step.append(scored)
            if scored >= min_scored and (t + 1) % 50 == 0:
                break
        out.append(per_step)
    return out


def main():
    seeds, T, K, S = {}, {}, {}, {}
    for N in tg.PLAYERS:
        seeds[N], T[N], sens = case2(N)
        K[N], sens3 = case3(N, seeds[N])
        per = case4(N, tg.B)
        S[N] = max(len(p) for p in per)
        print(f"N={N}: seed {seeds[N]}, T {T[N]}, (episodes, order-sensitive) by T under mt19937 / philox {sens}; K_END {K[N]} "
              f"(order-sensitive among the B games {sens3}); STEPS {S[N]}", flush=True)
    for N in (7, 11):
        per = case4(N, 321, limit=S[N])
        print(f"N={N}, 321 games, {S[N]} steps: scored ends {[p[-1] for p in per]}")
    print("SEED =", seeds)
    print("T =", T)
    print("K_END =", K)
    print("STEPS =", S)


if __name__ == "__main__":
    main()
