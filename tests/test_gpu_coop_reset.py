"""The fused rollouts' cooperative reset (csrc/skyjo_record.h: spare_issue_coop / spare_commit_coop): a finished game's next episode
is fetched by the WAVEFRONT - lane chunks * k + j takes piece j of the k-th resetting game, 64 / chunks games at a time, the games
beyond that group by LDS-DMA - and written into the game's column of the tile at commit time.  Every record of every iteration and
the counters against the oracle, at the smallest shapes at which that can go wrong:

  * many resets in one iteration (64 freshly seeded games end their first episodes within a few iterations of each other: several
    games in the group, and more than a group serves - asserted on the oracle's own records),
  * partial last tiles whose lanes without a game are fetch lanes (70 x 3); 130 x 2: the two-player kernels keep the LDS-DMA
    (EXPERIMENTS.md: the cooperative form loses at their small batches) - the same records are asked of them,
  * four players in both record layouts and the direct observation (other `chunks`, other code below the shared function),
  * an engine that never deals ahead: every reset finds its bank empty, the fetched record is stale and the game deals in place,
  * a reset in the iteration right after a cycle-end barrier (four dealing cycles in one launch),
  * dealing in line (k_step<.., true, 3>: the same path with one wavefront per workgroup).
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
THREADS = min(16, os.cpu_count() or 1)
SLICE = 64  # iterations the oracle records at a time
ST_RESET = 3

CASES = [
    # name                 B    N  indirect  layout         form         iterations (< 0: that many dealing cycles in ONE launch), calls
    ("many_resets_64x3", 64, 3, True, "row-major", "one kernel", 400, 1),
    ("partial_tile_70x3", 70, 3, True, "row-major", "one kernel", 400, 1),
    ("partial_tile_130x2", 130, 2, True, "tile-planar", "one kernel", 400, 1),
    ("four_players_64x4_tile_planar", 64, 4, True, "tile-planar", "one kernel", 400, 1),
    ("four_players_64x4_row_major", 64, 4, True, "row-major", "one kernel", 400, 1),
    ("direct_obs_64x3", 64, 3, False, "tile-planar", "one kernel", 400, 1),
    ("never_deals_ahead_64x3", 64, 3, True, "row-major", None, 400, 1),
    ("four_cycles_per_launch_64x3", 64, 3, True, "tile-planar", "one kernel", -4, 3),
    ("in_line_64x3", 64, 3, True, "row-major", "in line", 400, 1),
]


@pytest.mark.parametrize("name,B,N,ind,layout,form,K,calls", CASES, ids=[c[0] for c in CASES])
def test_every_record_with_cooperative_resets(name, B, N, ind, layout, form, K, calls):
    from oracle import skyjo_oracle as so
    from skyjo_rl_amd import SkyjoVecEnv

    cfg = dict(num_players=N, score_penalty=2.0, observe_other_player_indirect=ind, mean_reward=1.0, reward_refunded=0.001,
               rng_mode=0, auto_reset=True)
    dry = name.startswith("never_deals_ahead")
    eng = SkyjoVecEnv(B, no_bank=True, **cfg) if dry else SkyjoVecEnv(B, **cfg)
    ora = so.OracleVec(num_envs=B, **cfg)
    if form == "in line":
        eng.set_overlap(0)
    if form is not None:
        assert eng.dealing_form() == form, (name, eng.dealing_form())
    if K < 0:
        eng.set_deal_interval(eng.deal_interval())  # (pinned: a launch of whole cycles is what the case is about)
        K = -K * eng.deal_interval()
    eng.seed(None, 11)
    ora.seed(None, 11)
    planar = layout == "tile-planar"
    if planar:
        eng.set_record_layout("tile-planar")
    rec = eng.new_planar_records(K) if planar else eng.new_records(K)
    most = 0  # most resets of one tile in one iteration (the oracle's records)
    for r in range(calls):
        eng.rollout(K, policy_seed=3, records=rec)
        for s0 in range(0, K, SLICE):
            n = min(SLICE, K - s0)
            oact, obs, mask, meta, eplen = ora.rollout(n, 3, threads=THREADS, record_obs=True)
            v = eng.split(eng.rows_from_planar(rec[s0:s0 + n]) if planar else rec[s0:s0 + n])
            at = f"{name}: call {r}, iterations {s0}..{s0 + n - 1}"
            np.testing.assert_array_equal(v.action.cpu().numpy(), oact.astype(np.int8), err_msg=f"action bytes, {at}")
            np.testing.assert_array_equal(v.observations.cpu().numpy(), obs, err_msg=f"observations, {at}")
            np.testing.assert_array_equal(v.action_mask.cpu().numpy(), mask, err_msg=f"action masks, {at}")
            np.testing.assert_array_equal(v.agent.cpu().numpy(), meta[..., 0], err_msg=f"agent, {at}")
            np.testing.assert_array_equal(v.phase.cpu().numpy(), meta[..., 1], err_msg=f"phase, {at}")
            np.testing.assert_array_equal(v.done.cpu().numpy(), meta[..., 2], err_msg=f"done, {at}")
            np.testing.assert_array_equal(v.status.cpu().numpy(), meta[..., 3], err_msg=f"status, {at}")
            np.testing.assert_array_equal(v.episode_steps.cpu().numpy().astype(np.uint16), eplen, err_msg=f"episode steps, {at}")
            resets = meta[..., 3] == ST_RESET  # [iteration][game]
            for t0 in range(0, B, 64):
                most = max(most, int(resets[:, t0:t0 + 64].sum(axis=1).max()))
    c, oc = eng.counters(), ora.counters()
    print(f"{name}: {c['resets']} resets, at most {most} of one tile in one iteration, {c['waits']} dealt in place")
    for k in ("steps", "episodes", "illegal", "resets", "sum_len"):
        assert c[k] == oc[k], (name, k, c[k], oc[k])
    assert c["steps"] + c["resets"] == calls * K * B and c["illegal"] == 0
    assert c["resets"] > B
    if N >= 3:
        # (freshly seeded: on the oracle's records) more games in one iteration than one group of three serves - several games in
        # the group, and the games beyond it by LDS-DMA - in every case that takes the cooperative form
        assert most > 64 // (12 + 2 * N), (name, most)
    if dry:
        assert c["waits"] == c["resets"], (c["waits"], c["resets"])  # every reset fetched a stale record and dealt in place
    eng.close()
