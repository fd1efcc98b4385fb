"""GPU: the four per-seat float64 sums of ``counters()`` - ``sum_score``, ``sum_reward``, ``sum_reward_sq``, ``sum_refunded`` - and the integer
counters, against an episode log of the CPU oracle, on every path that writes them.

The reference and the rule are tests/seat_stats_ref.py: the oracle is advanced one lockstep iteration at a time and every episode that
ends is logged; ``check(counters, log, N)`` compares with ``==`` in the EXACT regime (dyadic settings, N in {1, 2, 4, 8}: every partial
sum is exact in any order) and holds every other case to  n * 2^-53 * fsum(|x|)  around ``math.fsum`` of the log (the BOUND regime:
penalty 1/3, mean reward 0.1, 0.007 per refunded card, illegal reward -0.3).  ``sum_refunded``, ``episodes`` and ``illegal`` are always
compared with ``==``.  The cases, their tables and the conditions they meet (at least 3 B ended episodes, every seat a finisher, every seat
penalised, the seats' sums different, illegal ends per seat) are tests/seat_stats_cases.py, asserted on the CPU by tests/test_seat_stats_ref.py.  B = 130 unless
stated: two full tiles and a tile of two lanes.  Every test prints ``SEATSTATS <case> <kind> <|got - want| / allowance>``: recorded in
EXPERIMENTS.md, never asserted.

The sites that write the sums (skyjo_transition.h, skyjo_step.h, skyjo_cycle.h), and the cases that reach them - exact / bound:

  a. ``finish_game`` + LDS atomics ``ACC`` (the generic kernels: N = 1 and 5 .. 12), scored in the iteration the game ends:
     fused rollout and caller actions at N = 1, 8 / N = 5, 6, 7, 9 .. 12.
  b. ``finish_game_fixed`` + register accumulators ``racc`` (N = 2, 3, 4), scored on the spot: caller actions at N = 2, 4 / N = 3 (a step
     with caller actions never defers); the one-kernel form WITHOUT deferred scoring (``defer_ok`` false) - bound only: N = 3, the direct
     observation, SKYJO_OPT_CYCLE_S = 4 is the one shape whose four step regions do not fit a CU's LDS with the card chunks
     (skyjo_capi.hip resolve_form; it needs N <= 3 and the wide records, and at N = 2 the four regions fit) - no option reports the
     choice, so that case rests on resolve_form's arithmetic, and the same engine with the indirect observation runs deferred.
  c. the deferred service point (``finish_game_fixed`` on the ``pendp`` copy of the card rows, up to 31 iterations after the end, when
     the tile already holds the next episode): the fused rollout at N = 2, 4 / N = 3 in every dealing form - a launch of two whole
     SK_SCORE_EVERY periods, one of 37 iterations, launches of one and two iterations (``it == iters - 1``: CPU-asserted that an episode
     ends in the last iteration of such a launch), and a second slicing of the same run; SKYJO_OPT_CYCLE_S 1, 2, 4 with four dealing
     cycles per launch (cycle ends inside a launch), the tile-planar layout once.
  d. in-place deals and reshuffles beside waiting card rows (the rare paths' scratch aliases the staging area beside ``pendp``): deal
     interval 1000 at N = 2 / N = 3, in line and in the one-kernel form, ``waits > 0``.
  e. the illegal-action branch unrolled over the seats (``racc``): caller actions at N = 2, 4 / N = 3; the model rollout with
     ``no_masking`` at N = 3 (bound).
  f. the illegal-action branch with one ``acc_add``: caller actions at N = 1, 8 / N = 5, 6, 7, 9 .. 12.
  g. the end-of-launch shuffle tree into ``acc_tile`` (slot ``lane / N``, ``lane % N``; gated on ``__any(episodes | illegal)``): every case -
     N = 12 fills 48 lanes; launches of one iteration in which nothing ends, and steps that end nothing but by illegal actions.
  h. ``k_reduce_stats`` (the four arrays as one, ``kind * 12 + seat``): every ``counters()``; more than one workgroup at 16 500 games = 258
     tiles, the last of 52 games: N = 2 / N = 3.
  i. ``skyjo_vec_step_collect`` (model rollout, arena collect): the sums over a span against the buffer's own ``final_rewards`` where
     ``episode_end`` is set, and ``skyjo_vec_episode_stats`` on the same columns by the same rule (N = 3: bound).
"""
import ctypes as C
import math

import numpy as np
import pytest

from tests import seat_stats_cases as sc
from tests import seat_stats_ref as ssr

pytestmark = pytest.mark.gpu

B = sc.B
INTEGER_KEYS = ("steps", "episodes", "resets", "sum_len", "illegal")
FORMS = {"in_line": 0, "two_streams": 2, "one_kernel": 3}


def _engine(num_envs, cfg, form=None, cycle_s=None):
    from skyjo_rl_amd import SkyjoVecEnv, _lib

    eng = SkyjoVecEnv(num_envs, **cfg)
    if cycle_s is not None:
        eng.set_option(_lib.OPT_CYCLE_S, cycle_s)  # (before the engine is seeded)
    if form is not None:
        eng.set_overlap(FORMS[form])
        assert eng.dealing_form() == form.replace("_", " ")
    return eng


def _held(case, counters, log, N, oracle_counters=None):
    """``check``, the integer counters against the oracle's where the log spans the oracle's whole life, and the recorded figure."""
    used = ssr.check(counters, log, N)
    if oracle_counters is not None:
        for key in INTEGER_KEYS:
            assert counters[key] == oracle_counters[key], (case, key, counters[key], oracle_counters[key])
    for kind in ssr.KINDS:
        print(f"SEATSTATS {case} {'exact' if log.exact else 'bound'} {kind} {used[kind]:.3f}")
    return used


def _bits(c):
    return tuple(np.asarray(c[k], dtype=np.float64).tobytes() for k in ssr.KINDS) + tuple(int(c[k]) for k in INTEGER_KEYS)


# ----------------------------------------------------------------------------------------------------------------- fused rollout
def _rollout_cases():
    for N in sc.PLAYERS:
        for ind in (True, False):
            for form in FORMS:
                if form == "one_kernel" and N not in (2, 3, 4):
                    continue  # the one-kernel form is compiled for two to four players
                yield pytest.param(N, ind, form, id=f"N{N}-{'indirect' if ind else 'direct'}-{form}")


@pytest.mark.parametrize("N,ind,form", list(_rollout_cases()))
def test_fused_rollout_sums_equal_the_episode_log(N, ind, form):
    """Sites a / c, g, h.  Auto-reset: the sums are the only witness of the episodes that end and are re-dealt inside a launch."""
    cfg = sc.config(N, ind)
    log = sc.rollout_log(N, cfg["rng_mode"], sc.ITERS[N])
    slicings = [("a", sc.slicing_a(sc.ITERS[N]))] + ([("b", sc.slicing_b(sc.ITERS[N]))] if form == "in_line" else [])
    got = {}
    for name, slicing in slicings:
        eng = _engine(B, cfg, form)
        eng.seed(None, sc.SEED[N])
        for k in slicing:
            eng.rollout(k, policy_seed=sc.POLICY_SEED)
        got[name] = eng.counters()
        _held(f"fused-N{N}-{'ind' if ind else 'dir'}-{form}-{name}", got[name], log, N, log.ora.counters())
        assert got[name]["illegal"] == 0 and got[name]["episodes"] >= 3 * B
        eng.close()
    if "b" in got and log.exact:  # the two slicings agree by the same rule: bit for bit in the exact regime
        assert _bits(got["a"]) == _bits(got["b"])


# ----------------------------------------------------------------------------------------------------------------- one-kernel form
@pytest.mark.parametrize("N,ind,S,planar", [(2, True, 1, False), (3, True, 2, False), (2, False, 4, False), (4, True, 2, False), (4, False, 3, False), (3, True, 4, False),
                                            (3, False, 4, False), (2, True, 2, True), (3, False, 1, True)],
                         ids=["N2-S1", "N3-S2", "N2-direct-S4", "N4-S2", "N4-direct-S3", "N3-S4-deferred", "N3-direct-S4-not_deferred", "N2-S2-planar", "N3-direct-S1-planar"])
def test_one_kernel_form_sums_equal_the_episode_log(N, ind, S, planar):
    """Sites b / c: SKYJO_OPT_CYCLE_S 1, 2 and 4 (four players: up to 3 - four of their step regions do not fit a CU's LDS and the engine
    lowers the request), four dealing cycles per launch (three cycle ends inside it), the last launch shorter; tile-planar records; three
    players with the direct observation at S = 4: scored in the iteration the game ends."""
    from skyjo_rl_amd import _lib

    cfg = sc.config(N, ind)
    log = sc.rollout_log(N, cfg["rng_mode"], sc.ITERS[N])
    eng = _engine(B, cfg, "one_kernel", cycle_s=S)
    v = C.c_int64()
    _lib.check(eng._L.skyjo_vec_get_option(eng._h, _lib.OPT_CYCLE_S, C.byref(v)))
    assert int(v.value) == S
    eng.set_deal_interval(eng.deal_interval())  # pinned: a launch of whole cycles
    K = 4 * eng.deal_interval()
    if planar:
        eng.set_record_layout("tile-planar")
    eng.seed(None, sc.SEED[N])
    rest = sc.ITERS[N]
    assert rest > K
    while rest > 0:
        k = min(K, rest)
        eng.rollout(k, policy_seed=sc.POLICY_SEED, records=eng.new_planar_records(k) if planar else None)
        rest -= k
    _held(f"cycle-N{N}-{'ind' if ind else 'dir'}-S{S}{'-planar' if planar else ''}", eng.counters(), log, N, log.ora.counters())
    eng.close()


# ----------------------------------------------------------------------------------------------------------------- banks run dry
@pytest.mark.parametrize("form", ["in_line", "one_kernel"])
@pytest.mark.parametrize("N", [2, 3])
def test_sums_when_the_banks_run_dry(N, form):
    """Site d.  Nothing is dealt ahead after the seeding (deal interval 1000): from its fourth or fifth episode on a finished game
    deals in place - in the scratch beside the card rows of the ends that still wait for their service point."""
    cfg = sc.config(N, True)
    log = sc.rollout_log(N, cfg["rng_mode"], sc.DRY_ITERS[N])
    eng = _engine(B, cfg, form)
    eng.set_deal_interval(1000)
    eng.seed(None, sc.SEED[N])
    for _ in range(sc.DRY_ITERS[N] // 100):
        eng.rollout(100, policy_seed=sc.POLICY_SEED)
    c = eng.counters()
    assert c["waits"] > 0, c["waits"]
    print(f"{c['waits']} deals in place")
    _held(f"dry-N{N}-{form}", c, log, N, log.ora.counters())
    eng.close()


# ----------------------------------------------------------------------------------------------------------------- caller actions
@pytest.mark.parametrize("auto_reset", [True, False], ids=["auto_reset", "no_auto_reset"])
@pytest.mark.parametrize("N", sc.PLAYERS)
def test_caller_action_sums_equal_the_episode_log(N, auto_reset):
    """Sites a / b, e / f, g: k_step without the policy - illegal actions, actions out of range, SKYJO_ACTION_SKIP; ``step_host`` and
    ``skyjo_vec_step_collect`` in turn.  The observation alternates with N (with auto-reset: indirect at odd N; without: at even N).
    Without auto-reset every game ends once, and the steps and skips of finished games that follow add nothing."""
    import torch
    from skyjo_rl_amd import _lib

    ind = (N % 2 == 1) == auto_reset
    cfg = sc.config(N, ind, auto_reset)
    log, acts = sc.caller_log(N, ind, auto_reset)
    L = _lib.load()
    eng = _engine(B, cfg)
    eng.seed(None, 40 + N)
    rec_d = eng.new_records()
    act_d = torch.empty(B, dtype=torch.int32, device="cuda")
    fr_d = torch.empty((B, N), dtype=torch.float64, device="cuda")
    ee_d = torch.empty(B, dtype=torch.uint8, device="cuda")
    vp = lambda t: C.c_void_p(t.data_ptr())
    steps = len(acts)
    all_done = None
    for t in range(steps):
        if t % 2 == 0:
            eng.step_host(acts[t])
        else:
            act_d.copy_(torch.from_numpy(acts[t]))
            _lib.check(L.skyjo_vec_step_collect(eng._h, vp(act_d), vp(rec_d), vp(fr_d), vp(ee_d), eng._stream()))
        if not auto_reset and t == steps - 21:
            all_done = eng.counters()
    c = eng.counters()
    _held(f"caller-N{N}-{'ind' if ind else 'dir'}-{'auto' if auto_reset else 'once'}", c, log, N, log.ora.counters())
    np.testing.assert_array_equal(eng.rewards_host()[2], log.ora.dones)
    if not auto_reset:
        # tools/dev/seat_stats_tables.py: every game has ended twenty steps before the last - those steps are SKYJO_ST_NOOP_DONE and skips
        assert all_done["episodes"] + all_done["illegal"] == B
        assert tuple(all_done[k].tobytes() for k in ssr.KINDS) == tuple(c[k].tobytes() for k in ssr.KINDS)
        assert (all_done["episodes"], all_done["illegal"], all_done["steps"]) == (c["episodes"], c["illegal"], c["steps"])
    eng.close()


# ----------------------------------------------------------------------------------------------------------------- model path
def _hold_sums(case, kind, got, columns, exact=False):
    """``got`` [N] against the addends ``columns`` (per seat a list): the rule of seat_stats_ref.check for one kind."""
    for p, xs in enumerate(columns):
        want = math.fsum(xs)
        allowance = 0.0 if exact else len(xs) * 2.0 ** -53 * math.fsum(abs(x) for x in xs)
        err = abs(float(got[p]) - want)
        assert err <= allowance, (case, kind, "seat", p, float(got[p]), want, err, allowance)
        print(f"SEATSTATS {case} bound {kind} {err / allowance if allowance else 0.0:.3f}")


@pytest.mark.parametrize("path", ["collect", "collect_no_masking", "arena_collect"])
def test_model_path_sums_equal_the_buffers_own_columns(path):
    """Site i (and e with ``no_masking``).  256 three-player games, T = 64, after 150 iterations of the fused rollout have spread the
    games over their episodes and the counters were reset: ``sum_reward`` / ``sum_reward_sq`` over the span against ``final_rewards`` where
    ``episode_end`` is set, read to the host; ``skyjo_vec_episode_stats`` on the same columns by the same rule."""
    import torch
    from skyjo_rl_amd import arena
    from skyjo_rl_amd.action_mask_model import ActionMaskModel, FusedNet
    from skyjo_rl_amd.rollout import RolloutBuffer, collect

    torch.manual_seed(3)
    nb, N, T = 256, 3, 64
    eng = _engine(nb, sc.config(N, True))
    eng.seed(None, 6)
    eng.rollout(150, policy_seed=sc.POLICY_SEED)
    eng.reset_counters()
    model = ActionMaskModel(obs_dim=eng.obs_dim).cuda()
    pol, val = FusedNet(model.policy), FusedNet(model.value)
    buf = RolloutBuffer(eng, T)
    if path == "arena_collect":
        arena.collect(eng, [("sample", pol), ("greedy", pol), "random"], [val, None, val], buf, seed=8)
    else:
        collect(eng, pol, val, buf, seed=8, no_masking=path == "collect_no_masking")
    c = eng.counters()
    ends = buf.episode_end.cpu().numpy().astype(bool)
    fr = buf.final_rewards.cpu().numpy()
    assert (fr[~ends] == 0.0).all()
    rows = fr[ends]  # [episodes, N]
    assert len(rows) == c["episodes"] + c["illegal"] and len(rows) >= 10, (len(rows), c["episodes"], c["illegal"])
    assert (c["illegal"] > 0) == (path == "collect_no_masking"), c["illegal"]
    rew = [[float(x) for x in rows[:, p] if x != 0.0] for p in range(N)]  # (an illegal end: the offender alone; a zero adds nothing)
    _hold_sums(path, "sum_reward", c["sum_reward"], rew)
    _hold_sums(path, "sum_reward_sq", c["sum_reward_sq"], [[x * x for x in xs] for xs in rew])
    st = arena.episode_stats(buf)
    sums = buf._stats_out[: 1 + 3 * N].cpu().numpy()
    assert st.episodes == len(rows) == int(sums[0])
    _hold_sums(path + "-episode_stats", "sum_reward", sums[1::3], rew)
    _hold_sums(path + "-episode_stats", "sum_reward_sq", sums[2::3], [[x * x for x in xs] for xs in rew])
    eng.close()


# ----------------------------------------------------------------------------------------------------------------- reduction geometry
@pytest.mark.parametrize("N", [2, 3])
def test_reduction_over_258_tiles(N):
    """Site h.  16 500 games: 258 tiles - two workgroups of k_reduce_stats at work, atomics between them - the last tile of 52 games; the
    one-kernel form, launches of 128 iterations, every game through at least two episodes.  The oracle runs on eight threads, one
    iteration at a time."""
    cfg = sc.config(N, True)
    log = sc.rollout_log(N, cfg["rng_mode"], sc.GEOM_ITERS[N], num_envs=sc.GEOM_B, seed=sc.GEOM_SEED[N], threads=8)
    eng = _engine(sc.GEOM_B, cfg, "one_kernel")
    assert eng.tiles == 258
    eng.seed(None, sc.GEOM_SEED[N])
    for _ in range(sc.GEOM_ITERS[N] // 128):
        eng.rollout(128, policy_seed=sc.POLICY_SEED)
    c = eng.counters()
    _held(f"geometry-N{N}", c, log, N, log.ora.counters())
    assert c["episodes"] >= 2 * sc.GEOM_B
    eng.close()


# ----------------------------------------------------------------------------------------------------------------- bookkeeping
@pytest.mark.parametrize("N", [2, 3])
def test_counter_bookkeeping(N):
    """``counters()`` twice: the same bits.  ``reset_counters()`` mid-run: the sums equal the log's tail.  Snapshot, run on, restore: the
    snapshot's sums come back and a continued run equals the log.  ``distributed``'s means and deviations equal the same expressions on the
    log (exact regime: the same bits).  ``seed()`` zeroes the sums."""
    from skyjo_rl_amd.distributed import combine_stats, stats_record

    cfg = sc.config(N, True)
    log = sc.new_log(B, cfg, 5)
    eng = _engine(B, cfg)
    eng.seed(None, 5)

    def run(k, both=True):
        eng.rollout(k, policy_seed=sc.POLICY_SEED)
        if both:
            log.rollout(k, sc.POLICY_SEED)

    run(250)
    c1, c2 = eng.counters(), eng.counters()
    assert _bits(c1) == _bits(c2)
    _held(f"bookkeeping-N{N}-first", c1, log, N, log.ora.counters())
    assert c1["episodes"] > B
    eng.reset_counters()
    mark = len(log.entries)
    z = eng.counters()
    assert z["episodes"] == 0 and not any(z[k].any() for k in ssr.KINDS)
    run(170)
    _held(f"bookkeeping-N{N}-after_reset", eng.counters(), log.tail(mark), N)
    snap = eng.snapshot()
    cs = eng.counters()
    run(130, both=False)
    assert eng.counters()["episodes"] > cs["episodes"]
    eng.restore(snap)
    assert _bits(eng.counters()) == _bits(cs)
    run(130)
    c = eng.counters()
    tail = log.tail(mark)
    _held(f"bookkeeping-N{N}-after_restore", c, tail, N)
    snap.close()
    if tail.exact:  # the formulas as distributed.py writes them, on the log's sums in numpy float64
        want = ssr.naive_counters(tail, N)
        tot = combine_stats(np.asarray([stats_record(c, N)]), N)
        ep = max(float(want["episodes"] + want["illegal"]), 1.0)
        mean = want["sum_reward"] / ep
        np.testing.assert_array_equal(tot["mean_reward"], mean)
        np.testing.assert_array_equal(tot["std_reward"], np.sqrt(np.maximum(want["sum_reward_sq"] / ep - mean ** 2, 0.0)))
        np.testing.assert_array_equal(tot["mean_score"], want["sum_score"] / max(float(want["episodes"]), 1.0))
        assert (tot["std_reward"] > 0).all()
    eng.seed(None, 5)
    z = eng.counters()
    assert z["episodes"] == 0 and z["steps"] == 0 and not any(z[k].any() for k in ssr.KINDS)
    eng.close()


@pytest.mark.parametrize("N", [2, 3])
def test_reseeding_or_resetting_a_finished_game_adds_nothing(N):
    """Without auto-reset: ``seed_one`` of a game that stands finished and a masked ``reset`` of another add nothing to the sums; both games
    then play - and end - again, and the sums equal the log."""
    import torch

    cfg = sc.config(N, True, auto_reset=False)
    log = sc.new_log(B, cfg, 5)
    eng = _engine(B, cfg)
    eng.seed(None, 5)
    k = 40 + 30 * N
    eng.rollout(k, policy_seed=sc.POLICY_SEED)
    log.rollout(k, sc.POLICY_SEED)
    done = np.flatnonzero(log.ora.dones)
    assert 2 <= len(done) < B, len(done)
    c0 = eng.counters()
    ssr.check(c0, log, N)
    one, other = int(done[0]), int(done[-1])
    eng.seed_one(one, 1234)
    log.ora.seed_one(one, 1234)
    mask = np.zeros(B, dtype=np.uint8)
    mask[other] = 1
    eng.reset(torch.from_numpy(mask))
    log.ora.reset(mask)
    c1 = eng.counters()
    assert tuple(c1[k].tobytes() for k in ssr.KINDS) == tuple(c0[k].tobytes() for k in ssr.KINDS)
    assert (c1["episodes"], c1["illegal"]) == (c0["episodes"], c0["illegal"])
    eng.rollout(300, policy_seed=sc.POLICY_SEED)
    log.rollout(300, sc.POLICY_SEED)
    assert sum(e.game in (one, other) for e in log.entries) == 4  # both ended a second time
    _held(f"reseeded-N{N}", eng.counters(), log, N, log.ora.counters())
    eng.close()
