"""The kernels that read the engine's records on the caller's side - ``k_episode_ends``, ``k_unpack``, ``k_sample`` (csrc/skyjo_callers.h),
the pair draw in the net's epilogue and ``k_arena`` - on the synthetic records of tests/record_ref.py: every record geometry (the
indirect observation, the direct one with 1 .. 12 players), both layouts, every planar input with dirty padding, against the numpy
restatements of the header's contracts.  Every comparison is bit for bit, but the draw against float64, which is
``net_ref.check_draw`` as tests/test_gpu_net_synthetic.py uses it.  Every output lies between guard bytes that must stay untouched
and is prefilled with the same sentinel: a zero of the restatement must be a zero the kernel wrote.  What the cases reach, and that
the comparisons reject a restated wrong kernel, is asserted without a GPU in tests/test_record_ref.py.

The last section holds the hand-off checks of the Python wrappers around the same buffers (a caller's ``out``, a rollout buffer of
the other layout, the net's output for several planar iterations).  Their wrong-sized tensors are views into allocations large
enough for either layout: no refusal is needed to stay in bounds."""
import ctypes as C

import numpy as np
import pytest

from tests import arena_ref, net_ref
from tests import record_ref as ref
from tests.test_gpu_net_synthetic import HIGH_ID0, SEED_TICKET, _net

pytestmark = pytest.mark.gpu

GUARD = 256                   # bytes before and after every output (a multiple of 16: the outputs stay aligned)
FILL = 0xA5
ENGINE_WARMUP = 512           # unrecorded iterations before the engine-written case records: its games are then of every age
DRAW_ROWS = 6553              # tests/test_net_ref.py: 104 rows of every (mask family, logit family) pair
GEOMETRY_IDS = [ref.gid(N, ind) for N, ind in ref.GEOMETRIES]
NAMES = ref.UNPACK_NAMES


def _vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _guarded(shape, dtype):
    """(whole uint8 allocation, view of ``shape`` / ``dtype`` inside it), every byte FILL."""
    import torch

    shape = tuple(shape)
    nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    whole = torch.full((nbytes + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda:0")
    return whole, whole[GUARD:GUARD + nbytes].view(dtype).view(shape)


def _intact(*bufs):
    for whole, view in bufs:
        nbytes = view.numel() * view.element_size()
        assert bool((whole[:GUARD] == FILL).all()) and bool((whole[GUARD + nbytes:] == FILL).all()), "a guard byte was written"


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


@pytest.fixture(scope="module")
def handles():
    """SkyjoVecEnv per (B, N, indirect, auto_reset, game_id0), made on first use and closed with the module.  Most tests use one as
    the handle only: never seeded, no game played."""
    from skyjo_rl_amd import SkyjoVecEnv

    made = {}

    def get(B, N, indirect, auto_reset=True, game_id0=0):
        key = (B, N, indirect, auto_reset, game_id0)
        if key not in made:
            env = made[key] = SkyjoVecEnv(B, num_players=N, observe_other_player_indirect=indirect, auto_reset=auto_reset, game_id0=game_id0,
                                          mean_reward=1.0, reward_refunded=0.001, score_penalty=2.0)
            g = ref.geometry(N, indirect)
            assert (env.num_envs, env.num_players, env.obs_dim, env.mask_offset, env.record_bytes, env.tiles) == \
                (B, N, g["obs_dim"], g["mask_offset"], g["record_bytes"], (B + 63) // 64)
        return made[key]

    yield get
    for env in made.values():
        env.close()


# ---------------------------------------------------------------- episode ends
_PLAYED = {}


def _played(handles, B, N, indirect):
    """The engine (no auto-reset) with every game played to its end, and its rewards float64 [B, N] as the host call gives them."""
    env = handles(B, N, indirect, auto_reset=False)
    if id(env) not in _PLAYED:
        env.seed(None, 5)
        done = np.zeros(B, dtype=np.uint8)
        for _ in range(16):                                   # (the reference side's condition: rewards for every game)
            env.rollout_host(256)
            rew, _, done = env.rewards_host()
            if done.all():
                break
        assert done.all(), "%d of %d games still run after 16 x 256 iterations" % (int((done == 0).sum()), B)
        assert (rew != 0).any(axis=1).all()                   # the rows of a table sum to N x mean_reward (+ the refunds): no zero row
        _PLAYED[id(env)] = rew
    return env, _PLAYED[id(env)]


def _episode_ends(L, env, which, rec):
    import torch

    from skyjo_rl_amd import _lib

    fr, ee = _guarded((env.num_envs, env.num_players), torch.float64), _guarded((env.num_envs,), torch.uint8)
    if which == "plain":
        rc = L.skyjo_vec_episode_ends(env._h, _vp(rec), _vp(fr[1]), _vp(ee[1]), env._stream())
    else:
        rc = L.skyjo_vec_episode_ends_layout(env._h, _vp(rec), _lib.REC_TILE_PLANAR if which == "planar" else _lib.REC_ROW_MAJOR, _vp(fr[1]),
                                             _vp(ee[1]), env._stream())
    assert rc == 0
    _intact(fr, ee)
    return fr[1].cpu().numpy(), ee[1].cpu().numpy()


@pytest.mark.parametrize("B,N,indirect", ref.EPISODE_CASES, ids=["B%d-%s" % (B, ref.gid(N, ind)) for B, N, ind in ref.EPISODE_CASES])
def test_episode_ends_on_synthetic_records(handles, B, N, indirect):
    """skyjo_vec_episode_ends_layout in both layouts and skyjo_vec_episode_ends against ``episode_ends_ref`` with the engine's own
    rewards: final_rewards as int64 bits (+ 0.0 where no episode ended), episode_end byte for byte."""
    from skyjo_rl_amd import _lib

    L = _lib.load()
    env, rew_host = _played(handles, B, N, indirect)
    g = ref.geometry(N, indirect)
    rewards = env.rewards_tensor().cpu().numpy()
    assert np.array_equal(rewards.view(np.int64), rew_host.view(np.int64))
    for seed in ref.case_seeds(B, N, indirect):
        case = ref.consumer_case(B, N, indirect, seed)
        want = ref.episode_ends_ref(case["rows"], g, rewards)
        rows, planar = _dev(case["rows"]), _dev(case["planar"])
        for which, rec in (("plain", rows), ("row-major", rows), ("planar", planar)):
            got = _episode_ends(L, env, which, rec)
            bad = int((got[1] != want[1]).sum())
            print("%s seed %d: %d of %d rows with another episode_end (%d ends)" % (which, seed, bad, B, int(want[1].sum())))
            assert ref.same_episode_ends(got, want), (which, seed, bad)


def test_episode_ends_on_engine_written_planar_records_direct_N4():
    """The direct observation with four players (agent and done in different 16-byte pieces) as a caller meets it: the last iteration's
    block of a tile-planar rollout read in place == the same records row-major == the restatement on the unpacked bytes."""
    import torch

    from skyjo_rl_amd import SkyjoVecEnv

    B, N = 4106, 4
    g = ref.geometry(N, False)
    env = SkyjoVecEnv(B, num_players=N, observe_other_player_indirect=False, auto_reset=True)
    assert (env.obs_dim, env.mask_offset, env.record_bytes) == (g["obs_dim"], g["mask_offset"], g["record_bytes"])
    env.set_record_layout("tile-planar")
    assert env.record_layout == "tile-planar"
    K = env.deal_interval()
    env.set_deal_interval(K)
    env.seed(None, 23)
    # Unrecorded iterations first: the games are then of every age.  Under the on-device policy a draw and a place alternate and an
    # episode ends on an EVEN lockstep iteration counted from seeding, in every game at once (measured: EXPERIMENTS.md), so the last
    # recorded iteration, warm-up + K - 1, has to be even to show an end at all.
    env.rollout_host(ENGINE_WARMUP + (K + 1) % 2)
    rp = env.new_planar_records(K)
    rp.fill_(0xEE)                                            # (the padding slots of the last tile are never written)
    env.rollout(K, policy_seed=9, records=rp)
    last = rp[K - 1]
    rows = env.rows_from_planar(last).contiguous()
    assert rows.shape == (B, g["record_bytes"])
    out = {}
    for planar, rec in ((True, last), (False, rows)):
        fr, ee = _guarded((B, N), torch.float64), _guarded((B,), torch.uint8)
        env.episode_ends(rec, final_rewards=fr[1], episode_end=ee[1], planar=planar)
        _intact(fr, ee)
        out[planar] = (fr[1].cpu().numpy(), ee[1].cpu().numpy())
    want = ref.episode_ends_ref(rows.cpu().numpy(), g, env.rewards_tensor().cpu().numpy())
    print("deal interval %d, %d of %d games ended in the last iteration; planar differs in %d rows" % (K, int(want[1].sum()), B, int((out[True][1] != want[1]).sum())))
    assert int(want[1].sum()) >= 1
    assert ref.same_episode_ends(out[False], want), "row-major"
    assert ref.same_episode_ends(out[True], want), "tile-planar"
    assert ref.same_episode_ends(out[True], out[False])
    env.close()


# ---------------------------------------------------------------- unpack
UNPACK_PATTERNS = (NAMES, ("obs",), ("mask",), NAMES[2:])


def _unpack_cases():
    cases = []
    for N, ind in ref.GEOMETRIES:
        cases += [(N, ind, "rows", ref.UNPACK_ROWS), (N, ind, "tiles", ref.UNPACK_TILES)]
    cases += [(4, False, "rows", n) for n in ref.UNPACK_EXTRA["rows"]] + [(4, False, "tiles", t) for t in ref.UNPACK_EXTRA["tiles"]]
    for N, ind, tiles in ref.UNPACK_SECOND_ROUND:
        cases += [(N, ind, "rows", tiles * 64), (N, ind, "tiles", tiles)]
    return cases


def _unpack(L, env, kind, rec, count, n, g, which):
    import torch

    shapes = dict(obs=((n, g["obs_dim"]), torch.int8), mask=((n, 26), torch.int8), **{k: ((n,), torch.uint8) for k in NAMES[2:]})
    outs = {k: _guarded(*shapes[k]) for k in which}
    fn = L.skyjo_vec_unpack if kind == "rows" else L.skyjo_vec_unpack_tiles
    rc = fn(env._h, _vp(rec), count, *[_vp(outs[k][1]) if k in outs else None for k in NAMES], env._stream())
    assert rc == 0
    _intact(*outs.values())
    return {k: v[1].cpu().numpy() for k, v in outs.items()}


@pytest.mark.parametrize("N,indirect,kind,count", _unpack_cases(), ids=["%s-%s%d" % (ref.gid(N, ind), k, c) for N, ind, k, c in _unpack_cases()])
def test_unpack_all_six_outputs_and_null_patterns(handles, N, indirect, kind, count):
    """skyjo_vec_unpack on ``count`` row-major records / skyjo_vec_unpack_tiles on ``count`` tile-planar blocks (the last one partial,
    its padding dirty: the padding rows come out as the bytes the block holds) with all six outputs, and with obs only, mask only and
    the four meta arrays only - what is given is written, the guards around it are not."""
    from skyjo_rl_amd import _lib

    L = _lib.load()
    env = handles(ref.EPISODE_B, N, indirect)
    g = ref.geometry(N, indirect)
    second_round = (N, indirect, count if kind == "tiles" else count / 64) in ref.UNPACK_SECOND_ROUND
    if kind == "rows":
        n = count
        case = ref.consumer_case(n, N, indirect, 300 + N + count)
        rec, rows = _dev(case["rows"]), case["rows"]
    else:
        filled = count * 64 if second_round else (count - 1) * 64 + 1
        case = ref.consumer_case(filled, N, indirect, 400 + N + count)
        n = count * 64
        assert case["planar"].shape[0] == count
        rec, rows = _dev(case["planar"]), ref.rows_from_planar(case["planar"], n)
        assert np.array_equal(rows[:filled], case["rows"])
    assert (n * (g["obs_dim"] + 26) > ref.UNPACK_GRID_ELEMENTS) == second_round
    want = ref.unpack_ref(rows, g)
    for which in UNPACK_PATTERNS:
        got = _unpack(L, env, kind, rec, count, n, g, which)
        assert sorted(got) == sorted(which) and ref.unpack_mismatches(got, want) == [], which


# ---------------------------------------------------------------- the one-lane draw
def _sample(L, env, case, n, planar, rec):
    import torch

    from skyjo_rl_amd import _lib

    lg = _dev(case["logits"])
    a, lp, u = _guarded((n,), torch.int32), _guarded((n,), torch.float32), _guarded((n,), torch.float32)
    rc = L.skyjo_vec_sample_actions_layout(env._h, _vp(rec), _lib.REC_TILE_PLANAR if planar else _lib.REC_ROW_MAJOR, _vp(lg), n, case["seed"],
                                           case["ticket"], 1 if case["no_masking"] else 0, _vp(a[1]), _vp(lp[1]), _vp(u[1]), env._stream())
    assert rc == 0
    _intact(a, lp, u)
    return a[1].cpu().numpy(), lp[1].cpu().numpy(), u[1].cpu().numpy()


def _check_one_lane_draw(L, env, g, n, seed, ticket, game_id0):
    case = ref.draw_case(n, seed, ticket, g, game_id0=game_id0)
    assert case["records"].shape == (n, g["record_bytes"])
    planar = ref.to_planar(case["records"], np.random.default_rng(n + g["record_bytes"]))
    got = {p: _sample(L, env, case, n, p, _dev(planar if p else case["records"])) for p in (False, True)}
    for p in (False, True):
        a, lp, u = got[p]
        assert np.array_equal(u.view(np.uint32), case["u"].view(np.uint32)), ("uniform", p)
        assert net_ref.check_draw(a, lp, u, case) == [], p
    for x, y in zip(got[False], got[True]):
        assert np.array_equal(x.view(np.int32), y.view(np.int32))
    return case


@pytest.mark.parametrize("N,indirect", ref.GEOMETRIES, ids=GEOMETRY_IDS)
def test_one_lane_draw_at_every_geometry(handles, N, indirect):
    from skyjo_rl_amd import _lib

    g = ref.geometry(N, indirect)
    seed, ticket = SEED_TICKET[1]
    case = _check_one_lane_draw(_lib.load(), handles(ref.EPISODE_B, N, indirect), g, DRAW_ROWS, seed, ticket, 0)
    print("ambiguous rows", int(case["ref"]["ambiguous"].sum()))


def test_one_lane_draw_with_a_game_id_whose_high_word_changes(handles):
    from skyjo_rl_amd import _lib

    N, indirect = 4, False
    seed, ticket = SEED_TICKET[2]
    env = handles(ref.EPISODE_B, N, indirect, game_id0=HIGH_ID0)
    _check_one_lane_draw(_lib.load(), env, ref.geometry(N, indirect), DRAW_ROWS, seed, ticket, HIGH_ID0)


@pytest.mark.parametrize("n", ref.DRAW_EDGE_ROWS)
def test_one_lane_draw_at_the_block_edges_direct_N4(handles, n):
    """A partial block, and an odd number of rows in the last block: 26 n is no multiple of four floats and the logits' copy ends in
    its tail loop."""
    from skyjo_rl_amd import _lib

    seed, ticket = SEED_TICKET[1]
    _check_one_lane_draw(_lib.load(), handles(ref.EPISODE_B, 4, False), ref.geometry(4, False), n, seed, ticket, 0)


# ---------------------------------------------------------------- the pair draw away from 31 / 32 / 64
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["ties", "ramp"])
@pytest.mark.parametrize("N", [N for N, _ in ref.PAIR_GEOMETRIES])
def test_pair_draw_on_direct_observation_records(handles, N, kind, precision):
    """A net of 31 inputs on the records of a direct-observation engine (the ABI allows it): the draw in the net's epilogue reads the
    mask at the ENGINE's offset (44 / 56 / 68) out of 5 / 6 / 7 pieces.  ``FusedNet.act`` == ``sample_actions`` on the logits it wrote ==
    the single-net forward, planar == row-major, and the float64 reference's draw."""
    import torch

    n = DRAW_ROWS
    g = ref.geometry(N, False)
    env = handles(n, N, False)
    net = _net(net_ref.steered(kind), precision, key=("steered", kind))
    seed, ticket = SEED_TICKET[2]
    case = ref.draw_case(n, seed, ticket, g, rng_seed=1)
    planar = ref.to_planar(case["records"], np.random.default_rng(N))
    got = {}
    for p, rec in ((False, _dev(case["records"])), (True, _dev(planar))):
        lg, a, lp = _guarded((n, 26), torch.float32), _guarded((n,), torch.int32), _guarded((n,), torch.float32)
        net.act(env, rec, seed=seed, ticket=ticket, actions=a[1], logp=lp[1], logits=lg[1], planar=p)
        _intact(lg, a, lp)
        logits = lg[1].clone()
        lp1, u1 = torch.empty(n, device="cuda:0"), torch.empty(n, device="cuda:0")
        a1 = env.sample_actions(logits, rec, seed=seed, ticket=ticket, logp=lp1, uniform=u1, planar=p)
        assert torch.equal(a1, a[1]) and torch.equal(lp1.view(torch.int32), lp[1].view(torch.int32)), p
        fwd = _guarded((n, 26), torch.float32)
        net(rec, out=fwd[1], planar=p)
        _intact(fwd)
        assert torch.equal(fwd[1].view(torch.int32), logits.view(torch.int32)), p
        got[p] = (a[1].cpu().numpy(), lp[1].cpu().numpy(), logits.cpu().numpy(), u1.cpu().numpy())
        lgn = got[p][2]
        if kind == "ties":
            assert (lgn == np.float32(1.25)).all()
        else:
            assert np.abs(lgn - np.linspace(0.0, -120.0, 26)).max() < 120 * 2.0 ** -16   # (a bias is the sum of two bf16 values)
        assert net_ref.check_draw(got[p][0], got[p][1], got[p][3], net_ref.with_logits(case, lgn)) == [], p
    for x, y in zip(got[False], got[True]):
        assert np.array_equal(x.view(np.int32), y.view(np.int32))


# ---------------------------------------------------------------- arena select
ARENA_PATTERN = [("sample", "A"), ("greedy", "B"), "random", ("greedy", "A"), ("sample", "B"), "random"]


def _arena_spec(N):
    return [ARENA_PATTERN[s % len(ARENA_PATTERN)] for s in range(N)]   # (two seats: a sampled and a greedy net; from three on a random seat too)


@pytest.mark.parametrize("planar", [False, True], ids=["rows", "planar"])
@pytest.mark.parametrize("N", ref.ARENA_N)
def test_arena_select_on_synthetic_records(handles, N, planar):
    """Every row by the rule of its own seat, on records no game wrote: ``sample`` is ``sample_actions`` on that net's forward logits,
    ``random`` is ``sample_actions`` on zeros, ``greedy`` the rule of tests/arena_ref.py."""
    import torch

    from skyjo_rl_amd import arena

    B = ref.ARENA_B
    seed, ticket = SEED_TICKET[1]
    g = ref.geometry(N, True)
    env = handles(B, N, True)
    nets = {k: _net(net_ref.weights((31, 26), k), "fp32", key=((31, 26), k)) for k in ("A", "B")}
    spec = _arena_spec(N)
    assert {s if isinstance(s, str) else s[0] for s in spec} >= {"sample", "greedy"}
    assert len({s[1] for s in spec if not isinstance(s, str)}) == 2 and (N == 2 or "random" in spec)
    rows, mask, agent = ref.arena_records(B, g, np.random.default_rng(600 + N))
    rec = _dev(ref.to_planar(rows, np.random.default_rng(N)) if planar else rows)
    acts = _guarded((B,), torch.int32)
    seats = [s if isinstance(s, str) else (s[0], nets[s[1]]) for s in spec]
    assert arena.select(env, seats, rec, seed=seed, ticket=ticket, actions=acts[1], planar=planar) is acts[1]
    _intact(acts)
    got = acts[1].cpu().numpy().astype(np.int64)
    logits = {k: nets[k](rec, out=torch.empty((B, 26), dtype=torch.float32, device="cuda:0"), planar=planar) for k in {s[1] for s in spec if not isinstance(s, str)}}
    zeros = torch.zeros((B, 26), dtype=torch.float32, device="cuda:0")
    want = np.full(B, -99, dtype=np.int64)
    for s, entry in enumerate(spec):
        kind, name = (entry, None) if isinstance(entry, str) else entry
        if kind == "greedy":
            a = arena_ref.greedy_actions(logits[name].cpu().numpy(), mask)
        else:
            a = env.sample_actions(zeros if kind == "random" else logits[name], rec, seed=seed, ticket=ticket, planar=planar).cpu().numpy()
        want[agent == s] = a[agent == s]
    assert (want >= 0).all() and np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    legal = mask.sum(1) > 0
    assert (mask[legal, got[legal]] == 1).all()


# ---------------------------------------------------------------- hand-off checks of the wrappers
def _seeded(B, N, layout):
    from skyjo_rl_amd import SkyjoVecEnv

    env = SkyjoVecEnv(B, num_players=N, auto_reset=True)
    env.set_record_layout(layout)
    assert env.record_layout == layout
    env.seed(None, 41)
    return env


@pytest.mark.parametrize("layout", ["row-major", "tile-planar-all"])
def test_reset_step_observe_refuse_an_out_of_another_size(layout):
    import torch

    B, N = 130, 3
    env = _seeded(B, N, layout)
    rb = env.record_bytes
    sizes = {"row-major": B * rb, "tile-planar-all": env.tiles * 64 * rb}
    assert sizes["row-major"] != sizes["tile-planar-all"]
    big = torch.empty((2 * max(sizes.values()),), dtype=torch.uint8, device="cuda:0")   # either layout fits wherever a view starts
    right = big[:sizes[layout]]
    other = big[:sizes["row-major" if layout != "row-major" else "tile-planar-all"]]
    wrong = [other, other.view(-1, rb), big[:sizes[layout] + 16], big[:sizes[layout] - 16], big.view(-1, 2)[:sizes[layout], 0], right.view(torch.int8)]
    assert not wrong[4].is_contiguous() and wrong[4].numel() == right.numel()
    actions = torch.full((B,), 24, dtype=torch.int32, device="cuda:0")
    calls = (lambda out: env.reset(out=out), lambda out: env.observe(out=out), lambda out: env.step(actions, out=out))
    for call in calls:
        for out in wrong:
            with pytest.raises(ValueError):
                call(out)
    env.sync()

    def games(t):                                             # (the padding slots of a partial last tile are never written)
        return t.view(B, rb) if layout == "row-major" else env.rows_from_planar(t.view(env.tiles, rb // 16, 64, 16))

    for shaped in (right, right.view(-1, rb), env._new_step_records()):
        assert env.observe(out=shaped) is shaped
        assert torch.equal(games(shaped), games(env.observe()))
    assert env.reset(out=right) is right and env.step(actions, out=right) is right
    env.check_error()
    env.close()


def test_collect_refuses_a_buffer_of_the_other_layout_or_size():
    import torch

    from skyjo_rl_amd import SkyjoVecEnv
    from skyjo_rl_amd.rollout import RolloutBuffer, collect, collect_stepwise

    B, N, T = 130, 3, 2
    pol = _net(net_ref.weights((31, 26), "A"), "fp32", key=((31, 26), "A"))
    val = _net(net_ref.weights((31, 1), "A"), "fp32", key=((31, 1), "A"))
    env = SkyjoVecEnv(B, num_players=N, auto_reset=True)
    rb = env.record_bytes
    rows_bytes, planar_bytes = (T + 1) * B * rb, (T + 1) * env.tiles * 64 * rb
    big = torch.zeros((2 * planar_bytes,), dtype=torch.uint8, device="cuda:0")          # either layout fits
    early = RolloutBuffer(env, T)                                                      # made before the layout is chosen: row-major
    early.records = big[:rows_bytes].view(T + 1, B, rb)
    env.set_record_layout("tile-planar-all")
    env.seed(None, 41)
    assert not early.planar and env.record_layout == "tile-planar-all"
    short = RolloutBuffer(env, T)                                                      # the right layout, records of the other size
    assert short.planar
    short.records = big[:rows_bytes].view(T + 1, B, rb)
    for fn in (collect, collect_stepwise):
        for buf in (early, short):
            with pytest.raises(ValueError):
                fn(env, pol, val, buf, seed=3)
    env.sync()
    good = RolloutBuffer(env, T)                                                       # (and a buffer that fits is taken)
    first = env.reset()
    for fn in (collect, collect_stepwise):
        acts = fn(env, pol, val, good, seed=3, first_records=first).actions
        assert bool(((acts >= 0) & (acts < 26)).all())
    env.close()


def test_net_refuses_an_out_that_counts_padding_slots_as_games():
    """Several planar iterations of 130 games: rows are (iteration, tile, lane), so an ``out`` of iters x 130 rows would shift every
    iteration but the first.  Without ``out`` every iteration's first 130 rows are the row-major result."""
    import torch

    iters, B = 3, 130
    tiles = (B + 63) // 64
    net = _net(net_ref.weights((31, 26), "A"), "fp32", key=((31, 26), "A"))
    rng = np.random.default_rng(77)
    rows = rng.integers(0, 256, size=(iters, B, 64), dtype=np.uint8)
    from tests import learner_synth

    planar = _dev(learner_synth.to_planar_dirty(rows, rng))
    assert tuple(planar.shape) == (iters, tiles, 4, 64, 16)
    want = net(_dev(rows).view(iters * B, 64)).view(iters, B, 26)
    full = net(planar, planar=True)
    assert tuple(full.shape) == (iters * tiles * 64, 26)
    assert torch.equal(full.view(iters, tiles * 64, 26)[:, :B].view(torch.int32), want.view(torch.int32))
    big = torch.empty((iters * tiles * 64, 26), dtype=torch.float32, device="cuda:0")   # (every wrong-sized out is a view into it)
    for rows_out in (iters * B, B, iters * tiles * 64 - 1):
        with pytest.raises(ValueError):
            net(planar, out=big[:rows_out], planar=True)
    assert torch.equal(net(planar, out=big, planar=True).view(torch.int32), full.view(torch.int32))
    # one iteration's blocks: the output tells the game count
    for one in (planar[1], planar[1:2]):
        out = _guarded((B, 26), torch.float32)
        net(one, out=out[1], planar=True)
        _intact(out)
        assert torch.equal(out[1].view(torch.int32), want[1].view(torch.int32))
