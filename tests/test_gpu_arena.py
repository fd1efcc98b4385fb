"""Arena rollouts on the GPU (skyjo_rl_amd/arena.py; include/skyjo_vec.h: skyjo_vec_arena_*, skyjo_vec_episode_stats): per-seat nets,
greedy and random seats, and the per-seat results of the episodes that end.

Shapes: engines with the indirect observation and auto_reset, N in {2, 3, 4}, num_envs in {1, 63, 130} - one lane, a partial tile of
k_arena's 256 lanes and of the records' 64, two record tiles plus a partial one - row-major, and tile-planar-all at N = 3 x 130.
The nets are ``FusedNet(model.policy, precision="fp32")`` of seeded ``ActionMaskModel``s.  Expected actions are built from entry points
that existed before the arena (the net's forward, ``skyjo_vec_sample_actions_layout``) and tests/arena_ref.py; every comparison of
actions, records and flags is exact.
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest

from tests import arena_ref
from tests import policy_stats_checks as psc

pytestmark = pytest.mark.gpu

SHAPES = [(N, B, "row-major") for N in (2, 3, 4) for B in (1, 63, 130)] + [(3, 130, "tile-planar-all")]
IDS = ["N%d_B%d_%s" % (N, B, "rows" if lay == "row-major" else "planar") for N, B, lay in SHAPES]
SEED, TICKET0 = 8, 1000
MIXED = {2: ["random", ("greedy", "A")],
         3: [("greedy", "A"), ("sample", "B"), "random"],
         4: [("sample", "A"), ("greedy", "A"), "random", ("greedy", "B")]}  # two distinct nets on three seats


def _engine(N, B, layout="row-major", seed=33):
    from skyjo_rl_amd import SkyjoVecEnv

    env = SkyjoVecEnv(B, num_players=N, observe_other_player_indirect=True, auto_reset=True)
    if layout != "row-major":
        env.set_record_layout(layout)
    env.seed(None, seed)
    return env


@functools.lru_cache(maxsize=None)
def _nets():
    """Policy nets A and B, the value net V of A's model, and Z: a policy net whose parameters are all zero."""
    import torch

    from skyjo_rl_amd.action_mask_model import ActionMaskModel, FusedNet

    out = {}
    for name, seed in (("A", 4), ("B", 5)):
        torch.manual_seed(seed)
        model = ActionMaskModel(obs_dim=31)
        out[name] = FusedNet(model.policy, precision="fp32")
        if name == "A":
            out["V"] = FusedNet(model.value, precision="fp32")
    zero = ActionMaskModel(obs_dim=31)
    with torch.no_grad():
        for p in zero.parameters():
            p.zero_()
    out["Z"] = FusedNet(zero.policy, precision="fp32")
    return out


def _seats(spec):
    nets = _nets()
    return [s if isinstance(s, str) else (s[0], nets[s[1]]) for s in spec]


def _columns(env, buf):
    """The four columns the arena writes, as host tensors; records row-major without the padded lanes of a partial tile."""
    rec = env.rows_from_planar(buf.records) if buf.planar else buf.records
    return [x.cpu().clone() for x in (rec, buf.actions, buf.final_rewards, buf.episode_end)]


@functools.lru_cache(maxsize=None)
def _stepwise_reference(N, B, layout, T):
    """rollout.collect_stepwise with net A on every seat: the training rollout, one launch at a time (computed once per shape)."""
    from skyjo_rl_amd.rollout import RolloutBuffer, collect_stepwise

    nets = _nets()
    env = _engine(N, B, layout)
    buf = RolloutBuffer(env, T)
    collect_stepwise(env, nets["A"], nets["V"], buf, seed=SEED, first_ticket=TICKET0)
    cols = _columns(env, buf)
    assert env.counters()["illegal"] == 0
    env.close()
    return cols


def _play(N, B, layout, T, spec, **kw):
    from skyjo_rl_amd import arena
    from skyjo_rl_amd.rollout import RolloutBuffer

    env = _engine(N, B, layout)
    buf = RolloutBuffer(env, T)
    arena.play(env, _seats(spec), buf, seed=SEED, first_ticket=TICKET0, **kw)
    return env, buf


# ---------------------------------------------------------------- 1. the arena is the training rollout when it should be
@pytest.mark.parametrize("N,B,layout,T", [s + (24,) for s in SHAPES] + [(2, 130, "row-major", 320)], ids=IDS + ["N2_B130_rows_T320"])
def test_all_seats_sampling_one_net_is_the_training_rollout(N, B, layout, T):
    import torch

    ref = _stepwise_reference(N, B, layout, T)
    env, buf = _play(N, B, layout, T, [("sample", "A")] * N)
    got = _columns(env, buf)
    for name, a, b in zip(("records", "actions", "final_rewards", "episode_end"), got, ref):
        assert torch.equal(a, b), name
    if T == 320:  # random-length episodes take about 76 steps at N = 2 (tests/golden/policy_stats.npz): several hundred ends
        assert int(buf.episode_end.sum()) >= 1
    assert env.counters()["illegal"] == 0
    env.close()


# ---------------------------------------------------------------- 2. every row follows its seat's rule
def _expected_actions(env, buf, spec, t):
    """Row t's actions from the entry points that existed before the arena: the net's forward, the masked draw on given logits (on
    zeros for a random seat) and the numpy argmax of tests/arena_ref.py, chosen per game by the record's agent byte."""
    import torch

    nets = _nets()
    B = env.num_envs
    rec = buf.records[t]
    rows = env.rows_from_planar(rec) if buf.planar else rec
    v = env.split(rows)
    seat = v.agent.cpu().numpy().astype(np.int64)
    mask = v.action_mask.cpu().numpy()
    logits = {k: nets[k](rec, out=torch.empty((B, 26), dtype=torch.float32, device=rec.device), planar=buf.planar)
              for k in {s[1] for s in spec if not isinstance(s, str)}}
    zeros = torch.zeros((B, 26), dtype=torch.float32, device=rec.device)
    want = np.full(B, -99, dtype=np.int64)
    for s, entry in enumerate(spec):
        kind, name = (entry, None) if isinstance(entry, str) else entry
        if kind == "greedy":
            a = arena_ref.greedy_actions(logits[name].cpu().numpy(), mask)
        else:
            a = env.sample_actions(zeros if kind == "random" else logits[name], rec, seed=SEED, ticket=TICKET0 + t, planar=buf.planar).cpu().numpy()
        want[seat == s] = a[seat == s]
    return want, mask


@pytest.mark.parametrize("N,B,layout,T", [s + (24,) for s in SHAPES] + [(2, 130, "row-major", 200)], ids=IDS + ["N2_B130_rows_T200"])
def test_every_row_follows_its_seats_rule(N, B, layout, T):
    spec = MIXED[N]
    env, buf = _play(N, B, layout, T, spec)
    got = buf.actions.cpu().numpy()
    valid = buf.valid.cpu().numpy()
    for t in range(T):
        want, mask = _expected_actions(env, buf, spec, t)
        assert np.array_equal(got[t], want), t
        assert mask[np.arange(B), got[t]][valid[t]].all(), "a transition row picked an illegal action"
    if T == 200:
        assert int(buf.episode_end.sum()) >= 1 and not valid.all()  # rows whose record shows done are covered as well
    assert env.counters()["illegal"] == 0
    env.close()


# ---------------------------------------------------------------- 3. ties
@pytest.mark.parametrize("B,layout", [(1, "row-major"), (130, "row-major"), (130, "tile-planar-all")], ids=["B1", "B130", "B130_planar"])
def test_greedy_on_equal_logits_is_the_smallest_legal_index(B, layout):
    N, T = 3, 64
    env, buf = _play(N, B, layout, T, [("greedy", "Z")] * N)
    v = buf.views()
    mask = v.action_mask[:T].cpu().numpy() != 0
    got = buf.actions.cpu().numpy()
    valid = buf.valid.cpu().numpy()
    first_legal = np.argmax(mask, axis=2)   # (0 for an empty mask)
    assert mask[valid].any(axis=1).all()
    assert np.array_equal(got[valid], first_legal[valid])
    empty = ~mask.any(axis=2)
    assert (got[empty] == 0).all()
    assert np.array_equal(got, first_legal)  # both statements at once: every row
    env.close()


# ---------------------------------------------------------------- 4. select and play agree
@pytest.mark.parametrize("N,B,layout", [(4, 130, "row-major"), (2, 63, "row-major"), (3, 130, "tile-planar-all")], ids=["N4_B130", "N2_B63", "N3_B130_planar"])
def test_select_then_step_collect_gives_plays_bits(N, B, layout):
    import torch

    from skyjo_rl_amd import _lib, arena
    from skyjo_rl_amd.rollout import RolloutBuffer

    T, spec = 24, MIXED[N]
    env, buf = _play(N, B, layout, T, spec)
    want = _columns(env, buf)
    env.close()
    L = _lib.load()
    vp = lambda t: C.c_void_p(t.data_ptr())
    env = _engine(N, B, layout)
    buf = RolloutBuffer(env, T)
    sp = arena.seat_policies(env, _seats(spec))
    env.observe(out=buf.records[0])
    for t in range(T):
        arena.select(env, sp, buf.records[t], seed=SEED, ticket=TICKET0 + t, actions=buf.actions[t], planar=buf.planar)
        _lib.check(L.skyjo_vec_step_collect(env._h, vp(buf.actions[t]), vp(buf.records[t + 1]), vp(buf.final_rewards[t]), vp(buf.episode_end[t]),
                                            env._stream()))
    for name, a, b in zip(("records", "actions", "final_rewards", "episode_end"), _columns(env, buf), want):
        assert torch.equal(a, b), name
    env.close()


# ---------------------------------------------------------------- 5. all seats random
def test_all_random_seats_need_no_workspace_and_pick_uniformly():
    """1 024 games x 128 iterations at N = 3 (131 072 rows, ~ 130 000 picks).  Sized on the CPU first: a numpy restatement of policy_ra
    (a uniform rank among the legal actions, numpy's default_rng) stepping tests/oracle_engine.py's engine at this size fills 11 cells
    of at least 2 000 picks (n = 2 and n = 13 .. 22 legal actions; the smallest holds ~ 6 000) and passes check_uniform_ranks, which
    asks for 8; the issue's starting size, 4 096 x 256, fills the same 11."""
    import torch

    from skyjo_rl_amd import _lib, arena
    from skyjo_rl_amd.rollout import RolloutBuffer

    N, B, T = 3, 1024, 128
    env = _engine(N, B)
    assert int(_lib.load().skyjo_vec_arena_workspace_bytes(env._h, 0)) == 0
    buf = RolloutBuffer(env, T)
    arena.play(env, ["random"] * N, buf, seed=SEED, first_ticket=TICKET0)
    assert getattr(buf, "_arena_workspace", None) is None   # a zero-byte workspace: nothing was allocated, NULL was passed
    v = buf.views()
    before = v.action_mask[:T] != 0
    act = buf.actions.to(torch.int64)
    valid = buf.valid
    assert bool(torch.gather(before, 2, act[..., None])[..., 0][valid].all()), "an action outside its mask"
    n_legal = before.sum(dim=2)
    rank = (before & (torch.arange(26, device=act.device)[None, None, :] < act[..., None])).sum(dim=2)
    counts = torch.bincount((n_legal * 26 + rank)[valid], minlength=27 * 26).cpu().numpy().reshape(27, 26)
    assert int(counts.sum()) == int(valid.sum())
    tested = psc.check_uniform_ranks(counts, who="arena, all seats random")
    print("cells tested:", tested, "picks:", int(counts.sum()))
    assert env.counters()["illegal"] == 0
    env.close()


# ---------------------------------------------------------------- 6. statistics on synthetic columns
GUARD = 64


def _device_stats(fr, ee, N, calls=2):
    """skyjo_vec_episode_stats on host columns: the 1 + 3 N doubles of every call, with guard bytes behind stats_out and the scratch."""
    import torch

    from skyjo_rl_amd import _lib

    L = _lib.load()
    dev = torch.device("cuda", 0)
    rows = ee.size
    need = int(L.skyjo_vec_episode_stats_scratch_bytes(rows, N))
    assert need == (rows + 1023) // 1024 * (1 + 3 * N) * 8
    d_fr = torch.from_numpy(np.ascontiguousarray(fr, dtype=np.float64)).to(dev)
    d_ee = torch.from_numpy(np.ascontiguousarray(ee, dtype=np.uint8)).to(dev)
    nout = (1 + 3 * N) * 8
    out = torch.full((nout + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    scratch = torch.full((need + GUARD,), 0x5A, dtype=torch.uint8, device=dev)
    res = []
    for _ in range(calls):
        out[:nout] = 0xA5
        _lib.check(L.skyjo_vec_episode_stats(C.c_void_p(d_fr.data_ptr()), C.c_void_p(d_ee.data_ptr()), rows, N, C.c_void_p(out.data_ptr()),
                                             C.c_void_p(scratch.data_ptr()), need, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        res.append(out[:nout].cpu().numpy().view(np.float64).copy())
        assert bool((out[nout:] == 0xA5).all()) and bool((scratch[need:] == 0x5A).all()), "a guard byte was written"
    return res


def _check_stats(got, fr, ee, N, exact):
    n, sums, squares, wins = arena_ref.episode_sums(fr, ee)
    assert got[0] == float(n)
    x = fr.reshape(-1, N)[ee.reshape(-1) != 0]
    for s in range(N):
        gs, gq, gw = got[1 + 3 * s: 4 + 3 * s]
        assert gw == float(wins[s]), ("wins", s)
        if exact:
            assert gs == sums[s] and gq == squares[s], ("sums", s)
        else:  # any order of n double additions lies within (n - 1) 2^-53 sum |x| of the exact sum
            bs = (n - 1) * 2.0 ** -53 * math.fsum(np.abs(x[:, s]))
            bq = (n - 1) * 2.0 ** -53 * math.fsum(x[:, s] * x[:, s])
            print("seat", s, "sum error", abs(gs - sums[s]), "bound", bs, "squares error", abs(gq - squares[s]), "bound", bq)
            assert abs(gs - sums[s]) <= bs and abs(gq - squares[s]) <= bq, ("sums", s)


@pytest.mark.parametrize("T,B,N", [(1, 1, 2), (3, 65, 3), (7, 130, 4), (5, 257, 12)], ids=["1x1x2", "3x65x3", "7x130x4", "5x257x12"])
def test_episode_stats_on_synthetic_columns(T, B, N):
    rng = np.random.default_rng(100 * T + N)
    rows = T * B
    # no episode end at all: every output is 0, and the rewards - NaN here - are not read
    res = _device_stats(np.full((rows, N), np.nan), np.zeros(rows, dtype=np.uint8), N)
    assert not res[0].any() and np.array_equal(res[0], res[1])
    # every row an end, integer rewards (negative ones included), exact ties of two seats and of all seats planted: all exact
    fr = rng.integers(-20, 21, size=(rows, N)).astype(np.float64)
    two, all_ = np.arange(rows) % 3 == 0, np.arange(rows) % 5 == 1
    top = fr.max(axis=1) + 1.0
    fr[two, 0] = top[two]
    fr[two, N - 1] = top[two]
    fr[all_] = fr[all_, :1]
    ee = np.full(rows, 7, dtype=np.uint8)  # (any non-zero byte is an end)
    res = _device_stats(fr, ee, N)
    assert res[0].tobytes() == res[1].tobytes()
    _check_stats(res[0], fr, ee, N, exact=True)
    assert res[0][0] == rows and res[0][3] >= two.sum()
    # about half the rows end; negative and non-integer rewards, ties of two and of all seats among them; NaN where no episode ended
    fr = rng.normal(size=(rows, N)) * 7.3 - 2.1
    top = fr.max(axis=1)
    fr[two, 0] = top[two]
    fr[two, N - 1] = top[two]
    fr[all_] = fr[all_, :1]
    ee = (rng.random(rows) < 0.5).astype(np.uint8)
    if rows > 1:
        ee[0], ee[-1] = 1, 1
    fr[ee == 0] = np.nan
    res = _device_stats(fr, ee, N)
    assert res[0].tobytes() == res[1].tobytes()
    _check_stats(res[0], fr, ee, N, exact=False)


# ---------------------------------------------------------------- 7. on a played buffer
def test_episode_stats_of_a_played_buffer():
    """``arena.episode_stats`` against the numpy restatement on the columns read back.  Counts and win rates are exact.  A mean is a
    sum within (n - 1) 2^-53 sum |x| of math.fsum, divided by n (one more rounding: 2^-53 relative).  The standard deviation goes
    through q - s^2 / n, whose relative error is at most the condition number (q / (q - s^2 / n), below 10^3 for rewards whose
    spread is no smaller than a thirtieth of their mean) times n 2^-52: rtol 1e-9 leaves orders of magnitude."""
    from skyjo_rl_amd import arena

    N, B, T = 2, 130, 320
    env, buf = _play(N, B, "row-major", T, ["random", ("greedy", "A")])
    st = arena.episode_stats(buf)
    again = arena.episode_stats(buf)
    assert st == again
    fr, ee = buf.final_rewards.cpu().numpy(), buf.episode_end.cpu().numpy()
    n, mean, std, win = arena_ref.episode_stats(fr, ee)
    assert st.episodes == n == int(buf.episode_end.sum()) and n >= 2
    x = fr.reshape(-1, N)[ee.reshape(-1) != 0]
    for s in range(N):
        bound = (n - 1) * 2.0 ** -53 * math.fsum(np.abs(x[:, s])) / n + 2.0 ** -52 * abs(mean[s])
        print("seat", s, "mean", st.mean_reward[s], "error", abs(st.mean_reward[s] - mean[s]), "bound", bound, "std", st.std_reward[s], std[s])
        assert abs(st.mean_reward[s] - mean[s]) <= bound
        assert st.win_rate[s] == win[s]
        assert math.isclose(st.std_reward[s], std[s], rel_tol=1e-9, abs_tol=0.0) and std[s] > 0.0
    # evaluate() is play + episode_stats on a buffer of its own
    env2 = _engine(N, B)
    assert arena.evaluate(env2, _seats(["random", ("greedy", "A")]), T, seed=SEED, first_ticket=TICKET0) == st
    env.close()
    env2.close()


# ---------------------------------------------------------------- 8. validation
def test_invalid_arguments_are_refused_and_leave_engine_and_nets_alone():
    import torch

    from skyjo_rl_amd import _lib, arena
    from skyjo_rl_amd.action_mask_model import ActionMaskModel, FusedNet
    from skyjo_rl_amd.rollout import RolloutBuffer

    L = _lib.load()
    nets = _nets()
    N, B, T = 3, 130, 4
    env = _engine(N, B)
    buf = RolloutBuffer(env, T)
    env.observe(out=buf.records[0])
    exported = {k: nets[k].export().cpu() for k in ("A", "B", "V")}
    torch.manual_seed(1)
    narrow = FusedNet(ActionMaskModel(obs_dim=19).policy, precision="fp32")  # not the engine's observation
    vp = lambda t: C.c_void_p(t.data_ptr())
    stream = env._stream()
    good = arena.seat_policies(env, _seats(MIXED[N]))
    need = int(L.skyjo_vec_arena_workspace_bytes(env._h, 2))
    assert need == 2 * ((B * 26 * 4 + 15) // 16 * 16)
    ws = torch.empty((need + 16,), dtype=torch.uint8, device=buf.actions.device)
    sentinel = torch.full((T, B), -77, dtype=torch.int32, device=buf.actions.device)
    buf.actions.copy_(sentinel)
    rec1 = buf.records[1].clone()

    def seats(*entries):
        arr = (_lib.SeatPolicy * N)()
        for s, (net, kind) in enumerate(entries):
            arr[s].net = net._h.value if net is not None else None
            arr[s].kind = kind
        return arr

    def bufs(**kw):
        f = dict(records=vp(buf.records), actions=vp(buf.actions), logp=None, values=None, final_rewards=vp(buf.final_rewards),
                 episode_end=vp(buf.episode_end))
        f.update(kw)
        return _lib.RolloutBuffers(f["records"], f["actions"], f["logp"], f["values"], f["final_rewards"], f["episode_end"])

    def select(h=env._h, sp=good, rec=vp(buf.records[0]), layout=_lib.REC_ROW_MAJOR, act=vp(buf.actions[0]), w=vp(ws), wb=need):
        return L.skyjo_vec_arena_select(h, sp, rec, layout, SEED, 0, act, w, wb, stream)

    def rollout(h=env._h, sp=good, T_=T, b=None, w=vp(ws), wb=need):
        b = bufs() if b is None else b
        return L.skyjo_vec_arena_rollout(h, sp, T_, SEED, 0, C.byref(b) if b is not False else None, w, wb, stream)

    A, Bn, V = nets["A"], nets["B"], nets["V"]
    S, G, R = _lib.SEAT_SAMPLE, _lib.SEAT_GREEDY, _lib.SEAT_RANDOM
    bad_seats = {"unknown kind": seats((A, S), (A, 3), (None, R)), "negative kind": seats((A, S), (A, -1), (None, R)),
                 "net with random": seats((A, S), (A, G), (A, R)), "no net": seats((A, S), (None, G), (None, R)),
                 "no net, sample": seats((None, S), (A, G), (None, R)), "out_dim": seats((A, S), (V, G), (None, R)),
                 "obs_dim": seats((A, S), (narrow, G), (None, R))}
    if torch.cuda.device_count() > 1:
        torch.manual_seed(2)
        bad_seats["device"] = seats((A, S), (FusedNet(ActionMaskModel(obs_dim=31).policy, device=1), G), (None, R))
    cases = []
    for name, sp in bad_seats.items():
        cases += [("select: " + name, lambda sp=sp: select(sp=sp)), ("rollout: " + name, lambda sp=sp: rollout(sp=sp))]
    cases += [
        ("select: null handle", lambda: select(h=None)), ("select: null seats", lambda: select(sp=None)),
        ("select: null records", lambda: select(rec=None)), ("select: null actions", lambda: select(act=None)),
        ("select: null workspace", lambda: select(w=None)), ("select: small workspace", lambda: select(wb=need - 1)),
        ("select: zero workspace", lambda: select(wb=0)), ("select: misaligned workspace", lambda: select(w=C.c_void_p(ws.data_ptr() + 8))),
        ("select: bad layout", lambda: select(layout=_lib.REC_TILE_PLANAR_ALL)), ("select: negative layout", lambda: select(layout=-1)),
        ("rollout: null handle", lambda: rollout(h=None)), ("rollout: null seats", lambda: rollout(sp=None)),
        ("rollout: null buffers", lambda: rollout(b=False)), ("rollout: null records", lambda: rollout(b=bufs(records=None))),
        ("rollout: null actions", lambda: rollout(b=bufs(actions=None))), ("rollout: null final_rewards", lambda: rollout(b=bufs(final_rewards=None))),
        ("rollout: null episode_end", lambda: rollout(b=bufs(episode_end=None))), ("rollout: logp set", lambda: rollout(b=bufs(logp=vp(buf.logp)))),
        ("rollout: values set", lambda: rollout(b=bufs(values=vp(buf.values)))), ("rollout: T = 0", lambda: rollout(T_=0)),
        ("rollout: T < 0", lambda: rollout(T_=-3)), ("rollout: null workspace", lambda: rollout(w=None)),
        ("rollout: small workspace", lambda: rollout(wb=need - 1)), ("rollout: misaligned workspace", lambda: rollout(w=C.c_void_p(ws.data_ptr() + 4))),
    ]
    # the statistics
    fr, ee = buf.final_rewards, buf.episode_end
    rows = T * B
    sneed = int(L.skyjo_vec_episode_stats_scratch_bytes(rows, N))
    out = torch.full((1 + 3 * N,), -5.0, dtype=torch.float64, device=fr.device)
    scr = torch.empty((sneed + 8,), dtype=torch.uint8, device=fr.device)

    def stats(f=vp(fr), e=vp(ee), rows_=rows, n=N, o=vp(out), s=vp(scr), sb=sneed):
        return L.skyjo_vec_episode_stats(f, e, rows_, n, o, s, sb, stream)

    cases += [("stats: null final_rewards", lambda: stats(f=None)), ("stats: null episode_end", lambda: stats(e=None)),
              ("stats: null stats_out", lambda: stats(o=None)), ("stats: null scratch", lambda: stats(s=None)),
              ("stats: rows = 0", lambda: stats(rows_=0)), ("stats: rows < 0", lambda: stats(rows_=-1)),
              ("stats: num_players = 0", lambda: stats(n=0)), ("stats: num_players = 13", lambda: stats(n=13)),
              ("stats: small scratch", lambda: stats(sb=sneed - 1)), ("stats: misaligned scratch", lambda: stats(s=C.c_void_p(scr.data_ptr() + 4)))]
    for sz in ((0, N), (-1, N), (rows, 0), (rows, 13)):
        assert int(L.skyjo_vec_episode_stats_scratch_bytes(*sz)) == 0
    assert int(L.skyjo_vec_arena_workspace_bytes(None, 1)) == 0 and int(L.skyjo_vec_arena_workspace_bytes(env._h, -1)) == 0
    assert int(L.skyjo_vec_arena_workspace_bytes(env._h, 13)) == 0
    for name, call in cases:
        rc = call()
        assert rc == -1, (name, rc)   # SKYJO_E_INVALID
        assert L.skyjo_vec_last_error(), name
    env.sync()
    # nothing was launched: no action, record or statistic was written, the nets hold the same bytes
    assert torch.equal(buf.actions, sentinel) and torch.equal(buf.records[1], rec1) and bool((out == -5.0).all())
    for k, b in exported.items():
        assert torch.equal(nets[k].export().cpu(), b), k
    # the good calls still work and the engine still steps
    assert select() == 0 and rollout() == 0 and stats() == 0
    env.step(arena.select(env, good, buf.records[T]))
    assert int(out[0]) == int(buf.episode_end.sum()) and env.counters()["illegal"] == 0
    # the Python layer's own checks
    with pytest.raises(ValueError, match="planar"):
        buf.planar = True
        arena.play(env, good, buf)
    buf.planar = False
    with pytest.raises(ValueError, match="records"):
        arena.select(env, good, buf.records[0][:-1])
    narrow.close()
    env.close()


# ---------------------------------------------------------------- 9. stream
def test_play_on_a_side_stream_gives_the_same_bits():
    """play and the read of its columns are queued on one non-default stream; only that stream is waited for."""
    import torch

    from skyjo_rl_amd import arena
    from skyjo_rl_amd.rollout import RolloutBuffer

    N, B, layout, T = 3, 130, "row-major", 24
    ref = _stepwise_reference(N, B, layout, T)
    env = _engine(N, B, layout)
    side = torch.cuda.Stream(device=env.device_index)
    with torch.cuda.stream(side):
        buf = RolloutBuffer(env, T)
        arena.play(env, _seats([("sample", "A")] * N), buf, seed=SEED, first_ticket=TICKET0)
        got = [x.clone() for x in (buf.records, buf.actions, buf.final_rewards, buf.episode_end)]
        host = [torch.empty(x.shape, dtype=x.dtype, pin_memory=True) for x in got]
        for h, x in zip(host, got):
            h.copy_(x, non_blocking=True)
    side.synchronize()
    for name, a, b in zip(("records", "actions", "final_rewards", "episode_end"), host, ref):
        assert torch.equal(a, b), name
    env.close()


# ---------------------------------------------------------------- the example's evaluation
def test_evaluate_vs_random_is_greedy_against_random_seats():
    from examples.ppo import evaluate_vs_random
    from skyjo_rl_amd import arena

    N, B, T = 3, 130, 400
    nets = _nets()
    env, twin = _engine(N, B), _engine(N, B)
    got = evaluate_vs_random(env, nets["A"], T, seat=1, seed=SEED, first_ticket=TICKET0)
    want = arena.evaluate(twin, ["random", ("greedy", nets["A"]), "random"], T, seed=SEED, first_ticket=TICKET0)
    assert isinstance(got, arena.EpisodeStats) and got == want and got.episodes >= 1
    assert len(got.mean_reward) == len(got.std_reward) == len(got.win_rate) == N
    assert 1.0 - 1e-12 <= sum(got.win_rate) <= N   # every episode has a winner; ties count for each tied seat
    env.close()
    twin.close()
