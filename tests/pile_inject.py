"""Pile injection: mid-game reshuffles at two to four players, where random play never reaches one (TEST INFRASTRUCTURE; numpy only,
nothing from the package - an engine and an oracle come in as arguments).

A random game of two to four players ends long before its 100+ card draw pile is used up, so the reshuffle of skyjo.py:361-365 -
in MT19937 mode a wait for the deal in flight, a roll-back of that deal and of every banked one, a shuffle through a 16-word ring
that aliases the record staging area - only runs there when somebody takes the draw pile away.  Two families of `set_state`
injections do that to a freshly dealt game (the hands stay as dealt):

  near_empty  the draw pile keeps its top 0 .. 6 cards, every other card goes UNDER the discard pile (the old top stays on top).
              Cards are conserved (150); the first reshuffle takes 100 .. 126 cards: that many rng_interval draws, several refills of
              the ring, wraps of the 624-word state.
  thin        3, 4 or 6 pile cards in all, 0 .. 2 of them on the draw pile; the other cards leave the game (set_state does not ask
              for conservation).  A reshuffle every second or third pile draw: the in-episode count runs up (Philox sessions
              (episode, 1), (episode, 2), ...), roll-backs hit banks that are being refilled.

`inject` applies one family to an oracle and - after asserting that both stand on the same dealt state - to an engine.  `play` is
the script both test files run (tests/test_pile_inject.py on the oracle alone, tests/test_gpu_reshuffle_forms.py with an engine
beside it): warm-up, then twice reset of all games -> inject -> a compared segment.  `differences` compares two segments field by
field and says where they first differ; `assert_same` raises on any.
"""
import numpy as np

SEED, POLICY_SEED, WARMUP = 31, 9, 100
INJECT_SEEDS = (1, 8)  # numpy.random.default_rng of the two rounds (tests/test_pile_inject.py: every game then reshuffles inside its segment)
ST_RESET = 3
FIELDS = ("actions", "action_byte", "observations", "action_mask", "agent", "phase", "done", "status", "episode_steps")
COUNTERS = ("steps", "episodes", "resets", "sum_len", "reshuffles")
MIN_PILE = 2  # a reshuffle of a one-card pile: the reference pops from an empty list (skyjo.py:137, 366)


# ------------------------------------------------------------------------------------------ the two families
def _check(state, draw, disc):
    assert len(state["disc"]) >= 1 and state["hand"] == 15 and state["phase"] == 0, "inject into a freshly dealt game"
    assert len(draw) + len(disc) >= MIN_PILE and len(disc) >= 1
    return np.ascontiguousarray(draw, dtype=np.int8), np.ascontiguousarray(disc, dtype=np.int8)


def near_empty(state, rng):
    """(draw, disc): the top `keep` in 0 .. 6 cards stay (the pile is drawn from its end: skyjo.py:366), the rest goes under the discard pile."""
    draw, disc = np.asarray(state["draw"], dtype=np.int8), np.asarray(state["disc"], dtype=np.int8)
    keep = int(rng.integers(0, 7))
    cut = len(draw) - keep
    return _check(state, draw[cut:], np.concatenate([draw[:cut], disc]))


def thin(state, rng):
    """(draw, disc): T in {3, 4, 6} pile cards in all - the top `keep` in 0 .. 2 of the draw pile stay, the T - keep - 1 below them go
    under the old discard top; every other pile card leaves the game."""
    draw, disc = np.asarray(state["draw"], dtype=np.int8), np.asarray(state["disc"], dtype=np.int8)
    total = int(rng.choice([3, 4, 6]))
    keep = int(rng.integers(0, 3))
    cut = len(draw) - keep
    under = total - keep - 1
    assert total >= MIN_PILE and 0 <= under <= cut
    return _check(state, draw[cut:], np.concatenate([draw[cut - under:cut], disc[-1:]]))


FAMILIES = {"near-empty": (near_empty, 48), "thin": (thin, 96)}  # name -> (function, compared iterations)


# ------------------------------------------------------------------------------------------ states
def oracle_state(ora, g):
    """One game of an OracleVec in the terms of SkyjoVecEnv.get_state."""
    s, N = ora.game(g), ora.num_players
    return dict(cards=np.array([list(s.players_cards[p]) for p in range(N)], dtype=np.int8),
                masked=np.array([list(s.players_masked[p]) for p in range(N)], dtype=np.int8),
                draw=np.array(s.drawpile[:s.n_draw], dtype=np.int8), disc=np.array(s.discard_pile[:s.n_disc], dtype=np.int8),
                hand=int(s.hand_card), player=int(s.exp_player), phase=int(s.exp_phase), reshuffles=int(s.reshuffles),
                episode_steps=int(ora.v.contents.ep_len[g]), done=bool(ora.v.contents.done[g]))


def _same_state(a, b, tag):
    for k in ("cards", "masked", "draw", "disc"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{tag}: {k}")
    for k in ("hand", "player", "phase", "reshuffles", "episode_steps", "done"):
        assert a[k] == b[k], (tag, k, a[k], b[k])


def inject(family, rng, ora, eng=None, games=None):
    """Apply `family` to `games` (default: all) of the oracle and, when given, of the engine.  Only directly after a reset of those
    games: at episode step 0 with no reshuffle yet - the one point where both set_state agree on what they zero (the oracle's keeps
    `reshuffles` and the episode length, the engine's zeroes H_RESH and the step count).  Returns {game: (n_draw, n_disc)}."""
    fn = FAMILIES[family][0] if isinstance(family, str) else family
    out = {}
    for g in (range(ora.num_envs) if games is None else games):
        g = int(g)
        so = oracle_state(ora, g)
        assert so["episode_steps"] == 0 and so["reshuffles"] == 0 and not so["done"], (g, so)
        episode = 0
        if eng is not None:
            se = eng.get_state(g)
            _same_state(se, so, f"dealt state of game {g}")
            episode = se["episode"]  # (the counter-based reshuffle session is keyed by it)
        if getattr(fn, "whole_state", False):  # tests/board_inject.py: the boards, the hand and the turn as well as the piles
            cards, masked, draw, disc, hand, player, phase = fn(so, rng, ora.num_players)
        else:
            (draw, disc), cards, masked, hand, player, phase = fn(so, rng), so["cards"], so["masked"], so["hand"], so["player"], so["phase"]
        ora.set_state(g, cards, masked, draw, disc, hand, player, phase)
        if eng is not None:
            eng.set_state(g, cards, masked, draw, disc, hand, player, phase, episode=episode)
        out[g] = (len(draw), len(disc))
    return out


# ------------------------------------------------------------------------------------------ segments
def oracle_segment(ora, iters, policy_seed, games, tail=1, probe=None):
    """`iters` iterations of the on-device policy's restatement, every record; then `tail` more (episodes end on one iteration parity
    and a segment is even: only then do games stand finished) and what stands: piles of `games`, counters, rewards and scores.  Also,
    not for comparison: `resh` uint64 [iters, B], every game's reshuffles so far after each iteration, `resh_episode` (inside the
    running episode) and `resh_sizes`, (iteration, game, cards) of every pile that was reshuffled."""
    B, N = ora.num_envs, ora.num_players
    parts, resh, resh_ep, sizes = [], np.zeros((iters, B), np.uint64), np.zeros((iters, B), np.uint32), []
    before = ora.reshuffles()[0]
    for t in range(iters):
        parts.append(ora.rollout(1, policy_seed, record_obs=True))
        resh[t], resh_ep[t] = ora.reshuffles()
        if probe is not None:
            probe(t)  # (tests/board_inject.py looks at the oracle's games after every iteration)
        for g in np.flatnonzero(resh[t] != (resh[t - 1] if t else before)):
            sizes.append((t, int(g), int(ora.game(int(g)).n_draw) + 2))  # n cards -> n - 1 on the draw pile, one of them drawn (skyjo.py:135-138, 366)
    act, obs, mask, meta, eplen = (np.concatenate([p[k] for p in parts]) for k in range(5))
    seg = dict(actions=act, action_byte=act.astype(np.int8), observations=obs, action_mask=mask, agent=meta[..., 0], phase=meta[..., 1],
               done=meta[..., 2], status=meta[..., 3], episode_steps=eplen, resh=resh, resh_before=before, resh_episode=resh_ep,
               resh_sizes=sizes, error=None)
    if tail:
        ora.rollout(tail, policy_seed)
    seg["piles"] = {int(g): (oracle_state(ora, int(g))["draw"], oracle_state(ora, int(g))["disc"]) for g in games}
    c = ora.counters()
    seg["counters"] = {k: int(c[k]) for k in COUNTERS}
    dn = ora.dones.astype(bool)
    seg["finished"] = dn
    seg["rewards"] = ora.rewards
    seg["scores"] = np.array([[ora.game(i).final_score[p] for p in range(N)] if dn[i] else [0.0] * N for i in range(B)])
    return seg


def engine_segment(eng, iters, policy_seed, games, tail=1):
    """The same from a SkyjoVecEnv: ONE rollout call of `iters` iterations (in the one-kernel form the reshuffles then fall inside a
    launch of several dealing cycles), records in the engine's layout."""
    import torch

    B = eng.num_envs
    planar = eng.record_layout != "row-major"
    rec = eng.new_planar_records(iters) if planar else eng.new_records(iters)
    act = torch.empty((iters, B), dtype=torch.int32, device=rec.device)
    eng.rollout(iters, policy_seed=policy_seed, records=rec, actions=act)
    v = eng.split(eng.rows_from_planar(rec) if planar else rec)
    seg = {k: getattr(v, k).cpu().numpy() for k in ("observations", "action_mask", "agent", "phase", "done", "status")}
    seg.update(actions=act.cpu().numpy(), action_byte=v.action.cpu().numpy(), episode_steps=v.episode_steps.cpu().numpy().astype(np.uint16))
    if planar:  # the dense arrays skyjo_vec_unpack_tiles makes of the same blocks are what goes into the comparison
        obs, mask = eng.unpack_tiles(rec)
        seg["observations"] = obs.view(iters, eng.tiles * 64, eng.obs_dim)[:, :B].cpu().numpy()
        seg["action_mask"] = mask.view(iters, eng.tiles * 64, 26)[:, :B].cpu().numpy()
        np.testing.assert_array_equal(seg["observations"], v.observations.cpu().numpy(), err_msg="unpack_tiles against the row-major copy")
    if tail:
        eng.rollout(tail, policy_seed=policy_seed)
    rew, sc, done = eng.rewards_host()
    seg["piles"] = {}
    for g in games:
        s = eng.get_state(int(g))
        seg["piles"][int(g)] = (s["draw"], s["disc"])
    c = eng.counters()
    seg["counters"] = {k: int(c[k]) for k in COUNTERS}
    seg["waits"] = int(c["waits"])
    seg["finished"], seg["rewards"], seg["scores"] = done.astype(bool), rew, np.where(done.astype(bool)[:, None], sc, 0.0)
    try:
        eng.check_error()
        seg["error"] = None
    except Exception as e:  # the sticky device error (include/skyjo_vec.h: skyjo_vec_check_error)
        seg["error"] = str(e)
    return seg


def differences(a, b):
    """Where two segments differ: {"records": {game: (iteration, field)} - the first differing record of each game -, "piles": games whose
    draw or discard pile differs after the segment, "counters": names, "finished": games whose done flag, rewards or final scores
    differ (==), "error": the device errors if either side has one}.  Empty dict: the same."""
    out = {}
    K, B = a["actions"].shape
    first = np.full(B, K, dtype=np.int64)
    field = [None] * B
    for k in FIELDS:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape, (k, x.shape, y.shape)
        ne = (x != y).reshape(K, B, -1).any(axis=2)
        t = np.where(ne.any(axis=0), ne.argmax(axis=0), K)
        for g in np.flatnonzero(t < first):
            first[g], field[g] = t[g], k
    if (first < K).any():
        out["records"] = {int(g): (int(first[g]), field[g]) for g in np.flatnonzero(first < K)}
    assert a["piles"].keys() == b["piles"].keys()
    piles = sorted(g for g in a["piles"] if not all(np.array_equal(p, q) for p, q in zip(a["piles"][g], b["piles"][g])))
    if piles:
        out["piles"] = piles
    cn = [k for k in COUNTERS if a["counters"][k] != b["counters"][k]]
    if cn:
        out["counters"] = {k: (a["counters"][k], b["counters"][k]) for k in cn}
    dn = a["finished"] & b["finished"]
    fin = (a["finished"] != b["finished"]) | (dn & ((a["rewards"] != b["rewards"]).any(axis=1) | (a["scores"] != b["scores"]).any(axis=1)))
    if fin.any():
        out["finished"] = [int(g) for g in np.flatnonzero(fin)]
    if a["error"] or b["error"]:
        out["error"] = (a["error"], b["error"])
    return out


def assert_same(a, b, tag):
    d = differences(a, b)
    if d:
        brief = {k: (dict(list(v.items())[:6]) if isinstance(v, dict) else v[:6] if isinstance(v, list) else v) for k, v in d.items()}
        sizes = {k: len(v) for k, v in d.items() if isinstance(v, (dict, list))}
        raise AssertionError(f"{tag}: the segments differ - {sizes} - first of each kind: {brief}")


# ------------------------------------------------------------------------------------------ the script of both test files
def segment_stats(seg, games):
    """What the oracle's side of a compared segment says about the path: reshuffles per injected game, the largest in-episode count,
    the pile sizes, the first iteration by which every game has reshuffled, and how many MT19937 games were dealt again after a
    roll-back had emptied their bank (a RESET record later than the game's first reshuffle)."""
    games = np.asarray(sorted(games), dtype=np.int64)
    resh = seg["resh"][:, games].astype(np.int64) - seg["resh_before"][games].astype(np.int64)
    K = resh.shape[0]
    per_game = resh[-1]
    first = np.where(per_game > 0, (resh > 0).argmax(axis=0), K)
    reset = seg["status"][:, games] == ST_RESET
    after = reset & (np.arange(K)[:, None] > first[None, :])
    return dict(per_game=per_game, total=int(per_game.sum()), min_per_game=int(per_game.min()), max_in_episode=int(seg["resh_episode"][:, games].max()),
                all_by=int(first.max()) + 1 if (per_game > 0).all() else None, sizes=(min(n for _, _, n in seg["resh_sizes"]), max(n for _, _, n in seg["resh_sizes"])) if seg["resh_sizes"] else None,
                redealt_after_rollback=int(after.any(axis=0).sum()), finished=int(seg["finished"].sum()))


def play(ora, family, eng=None, rounds=2, inject_seeds=INJECT_SEEDS, seed=SEED, on_segment=None, iters=None, probe=None):
    """seed -> WARMUP iterations (games then stand at different points, banks are partly used, dealing runs are in flight) -> `rounds` x
    [reset of ALL games (it takes a banked episode of every game: the next dealing run has work for all) -> inject `family` into every
    game -> one segment of the family's length].  With an engine every step is compared with the oracle's (assert_same).  Returns one
    dict per round: segment_stats + `injected` ({game: (n_draw, n_disc)}) + `seg` (the oracle's segment) and, with an engine, `eng`."""
    iters = FAMILIES[family][1] if iters is None else iters  # (a family given as a function brings its own length)
    tag = family if isinstance(family, str) else family.__name__
    games = list(range(ora.num_envs))
    ora.seed(None, seed)
    if eng is not None:
        eng.seed(None, seed)
    warm = oracle_segment(ora, WARMUP, POLICY_SEED, games[:8], tail=0)
    if eng is not None:
        assert_same(engine_segment(eng, WARMUP, POLICY_SEED, games[:8], tail=0), warm, f"{tag}: warm-up")
    out = []
    for r in range(rounds):
        ora.reset()
        if eng is not None:
            o = eng.reset_host()
            obs, mask, agent, phase = ora.observe()
            np.testing.assert_array_equal(o.observations, obs, err_msg=f"round {r}: observations after the reset")
            np.testing.assert_array_equal(o.action_mask, mask, err_msg=f"round {r}: masks after the reset")
            np.testing.assert_array_equal(o.agent, agent, err_msg=f"round {r}: agent after the reset")
        injected = inject(family, np.random.default_rng(inject_seeds[r]), ora, eng, games)
        if probe is not None:
            probe(-1)  # (the games as injected)
        seg = oracle_segment(ora, iters, POLICY_SEED, games, probe=probe)
        st = segment_stats(seg, games)
        st.update(injected=injected, seg=seg)
        if eng is not None:
            st["eng"] = engine_segment(eng, iters, POLICY_SEED, games)
            assert_same(st["eng"], seg, f"{tag}: round {r}")
        if on_segment is not None:
            on_segment(r, st)
        out.append(st)
    return out


def caller_actions(rng, mask, reveal=False):
    """Caller-chosen actions from the oracle's masks: the draw pile (24) whenever it is legal, else a uniformly random legal action -
    with `reveal` one that turns a hidden card over (12 .. 23) while there is one, so that episodes end within ~20 turns per seat."""
    u = rng.random(mask.shape) * (mask != 0)
    if reveal:
        u[:, 12:24] += (mask[:, 12:24] != 0)
    acts = np.argmax(u, axis=1).astype(np.int32)
    acts[mask[:, 24] != 0] = 24
    return acts


def play_caller(ora, family, steps, after_step=None, reveal=False, seed=SEED, inject_seed=INJECT_SEEDS[0], eng=None, actions_seed=5):
    """seed -> reset of all games -> inject -> `steps` steps with caller_actions.  after_step(t, acts, ended): called after the oracle
    has stepped (`ended`: the games whose episode that step ended).  Returns (reshuffles per game, largest in-episode count, episode ends)."""
    ora.seed(None, seed)
    if eng is not None:
        eng.seed(None, seed)
        eng.reset_host()
    ora.reset()
    inject(family, np.random.default_rng(inject_seed), ora, eng)
    rng = np.random.default_rng(actions_seed)
    before, deepest, ends = ora.reshuffles()[0], 0, 0
    for t in range(steps):
        obs, mask, agent, phase = ora.observe()
        acts = caller_actions(rng, mask, reveal)
        done_before = ora.dones.astype(bool)
        ora.step(acts)
        ended = ~done_before & ora.dones.astype(bool)
        ends += int(ended.sum())
        deepest = max(deepest, int(ora.reshuffles()[1].max()))
        if after_step is not None:
            after_step(t, acts, ended)
    return (ora.reshuffles()[0] - before).astype(np.int64), deepest, ends


# ------------------------------------------------------------------------------------------ the cases of tests/test_gpu_reshuffle_forms.py
MT, PHILOX = 0, 1
# id: players, rng mode, indirect observation, games, family, dealing form, dealing interval, options, record layout
#   options: work_list / unpipelined / cycle_s (set before the seed) / max_cycles  (SKYJO_OPT_INLINE_WORK_LIST, _UNPIPELINED, _CYCLE_S,
#   _MAX_CYCLES_PER_LAUNCH); 320 games = 5 tiles, so cycle_s 2 / 4 leave a last workgroup of one tile; 300 games: a last tile of 44
ROLLOUT_CASES = {
    "inline8_N2_mt_ind_near": (2, MT, True, 320, "near-empty", "in line", 8, {}, "row-major"),
    "inline8_N3_px_dir_thin": (3, PHILOX, False, 320, "thin", "in line", 8, {}, "row-major"),
    "inline8_N4_mt_dir_near": (4, MT, False, 320, "near-empty", "in line", 8, {}, "row-major"),
    "inline8_N4_mt_ind_thin_300": (4, MT, True, 300, "thin", "in line", 8, {}, "row-major"),
    "inline1000_N2_mt_ind_thin": (2, MT, True, 320, "thin", "in line", 1000, {}, "row-major"),
    "inline1000_N3_mt_dir_near": (3, MT, False, 320, "near-empty", "in line", 1000, {}, "row-major"),
    "inline1000_N4_mt_ind_thin": (4, MT, True, 320, "thin", "in line", 1000, {}, "row-major"),
    "worklist8_N3_mt_ind_near": (3, MT, True, 320, "near-empty", "in line", 8, {"work_list": 1}, "row-major"),
    "worklist8_N4_px_ind_thin": (4, PHILOX, True, 320, "thin", "in line", 8, {"work_list": 1}, "row-major"),
    "worklist8_N2_mt_dir_thin": (2, MT, False, 320, "thin", "in line", 8, {"work_list": 1}, "row-major"),
    "two8_N2_mt_dir_near": (2, MT, False, 320, "near-empty", "two streams", 8, {}, "row-major"),
    "two8_N3_mt_ind_thin": (3, MT, True, 320, "thin", "two streams", 8, {}, "row-major"),
    "two8_N4_mt_ind_near": (4, MT, True, 320, "near-empty", "two streams", 8, {}, "row-major"),
    "two8_N4_px_dir_thin": (4, PHILOX, False, 320, "thin", "two streams", 8, {}, "row-major"),
    "unpipelined8_N2_mt_ind_thin": (2, MT, True, 320, "thin", "two streams", 8, {"unpipelined": 1}, "row-major"),
    "unpipelined8_N3_mt_dir_near": (3, MT, False, 320, "near-empty", "two streams", 8, {"unpipelined": 1}, "row-major"),
    "unpipelined8_N4_mt_ind_thin": (4, MT, True, 320, "thin", "two streams", 8, {"unpipelined": 1}, "row-major"),
    "one8_S1_N2_mt_ind_near": (2, MT, True, 320, "near-empty", "one kernel", 8, {"cycle_s": 1}, "row-major"),
    "one8_S2_N3_mt_ind_thin": (3, MT, True, 320, "thin", "one kernel", 8, {"cycle_s": 2}, "row-major"),
    "one8_S4_N4_mt_ind_near": (4, MT, True, 320, "near-empty", "one kernel", 8, {"cycle_s": 4}, "row-major"),
    "one8_S2_N2_px_dir_thin": (2, PHILOX, False, 320, "thin", "one kernel", 8, {"cycle_s": 2}, "row-major"),
    "one8_S2_N3_mt_ind_near_300": (3, MT, True, 300, "near-empty", "one kernel", 8, {"cycle_s": 2}, "row-major"),
    "one40_S2_N3_mt_dir_near": (3, MT, False, 320, "near-empty", "one kernel", 40, {"cycle_s": 2}, "row-major"),
    "one40_S4_N2_mt_ind_thin": (2, MT, True, 320, "thin", "one kernel", 40, {"cycle_s": 4}, "row-major"),
    "one40_S1_N4_mt_ind_thin": (4, MT, True, 320, "thin", "one kernel", 40, {"cycle_s": 1}, "row-major"),
    "one8_max1_N3_mt_ind_thin": (3, MT, True, 320, "thin", "one kernel", 8, {"max_cycles": 1}, "row-major"),
    "one8_max16_N4_mt_ind_thin": (4, MT, True, 320, "thin", "one kernel", 8, {"max_cycles": 16}, "row-major"),
    "one8_planar_N3_mt_ind_near": (3, MT, True, 320, "near-empty", "one kernel", 8, {}, "tile-planar"),
    "one8_planar_N4_mt_dir_thin": (4, MT, False, 320, "thin", "one kernel", 8, {"cycle_s": 2}, "tile-planar"),
    "one8_planar_N2_px_ind_thin_300": (2, PHILOX, True, 300, "thin", "one kernel", 8, {}, "tile-planar"),
    "one40_planar_N2_mt_dir_near": (2, MT, False, 320, "near-empty", "one kernel", 40, {"cycle_s": 4}, "tile-planar"),
    "one8_planar_all_N3_mt_ind_thin": (3, MT, True, 320, "thin", "one kernel", 8, {}, "tile-planar-all"),
}
# caller actions through step_host (the POLICY = false kernel with a compile-time player count): players, rng mode, indirect, family, form
CALLER_GAMES, CALLER_STEPS = 192, 40
CALLER_CASES = {
    "N2_mt_ind_inline_near": (2, MT, True, "near-empty", "in line"),
    "N2_px_dir_two_thin": (2, PHILOX, False, "thin", "two streams"),
    "N3_mt_dir_inline_thin": (3, MT, False, "thin", "in line"),
    "N3_mt_ind_two_near": (3, MT, True, "near-empty", "two streams"),
    "N4_mt_ind_inline_thin": (4, MT, True, "thin", "in line"),
    "N4_mt_dir_two_near": (4, MT, False, "near-empty", "two streams"),
}
COLLECT_CASE = (2, MT, True, "thin", 320, 60)  # step_collect in a device loop: players, rng mode, indirect, family, games, steps
SNAPSHOT_CASES = {"two_streams": (3, MT, True, 320, "near-empty", "two streams", 8), "one_kernel": (4, MT, True, 320, "thin", "one kernel", 8)}


def oracle_config(N, rng_mode, indirect):
    """The configuration of every engine and oracle here (score_penalty 2.0, auto_reset on)."""
    return dict(num_players=N, score_penalty=2.0, observe_other_player_indirect=indirect, mean_reward=1.0, reward_refunded=0.001,
                rng_mode=rng_mode, auto_reset=True)
