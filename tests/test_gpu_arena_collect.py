"""Arena rollouts that record learner columns, on the GPU (skyjo_rl_amd/arena.py: ``act`` / ``collect``; include/skyjo_vec.h:
skyjo_vec_arena_act, skyjo_vec_arena_collect, skyjo_vec_rollout_select_seats) and their hand-off to the per-seat learner
(``rollout.select_rows`` / ``minibatches`` with ``seats``, ``examples.ppo.ppo_update_per_seat``).

Shapes: those of tests/test_gpu_arena.py (N in {2, 3, 4} x num_envs in {1, 63, 130} row-major, N = 3 x 130 tile-planar-all: one lane,
a partial workgroup of k_arena's 256 lanes, a partial record tile) and the synthetic records of tests/record_ref.py (321 games: a
second, partial workgroup).  Actions, values, records and flags are compared bit for bit; ``logp`` of a seat that is not the training
rollout's against float64 within ``net_ref.check_draw``'s bound, 1e-5 + 4 x 2^-24 |logp_ref|.

The direct observation has 43 / 67 / 163 features and a packed net at most 31 inputs (skyjo_vec_mlp_create), so no net can sit at such
a table: on the direct geometries of test 2 every seat is ``"random"`` and no seat has a value net - the mask words and the agent byte are
still read through the straddling pieces, the log-probability is - log(legal count) and every value 0.0.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import arena_collect_ref as acr
from tests import learner_synth, net_ref
from tests import record_ref as ref
from tests.test_gpu_arena import IDS, SEED, SHAPES, TICKET0, _engine, _nets
from tests.test_gpu_net_synthetic import SEED_TICKET, _net
from tests.test_gpu_record_consumers import _dev, _guarded, _intact, _vp, handles  # noqa: F401  (handles: a fixture)

pytestmark = pytest.mark.gpu


def _bits(t):
    """A tensor's bytes on the host: floats are compared as bits (-0.0 is not 0.0, a NaN equals itself)."""
    import torch

    t = t.detach().contiguous().cpu()
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int64) if t.dtype == torch.float64 else t


@functools.lru_cache(maxsize=None)
def _second_value_net():
    """W: the value branch of net B's model (tests/test_gpu_arena.py seeds it with 5 and keeps its policy branch only)."""
    import torch

    from skyjo_rl_amd.action_mask_model import ActionMaskModel, FusedNet

    torch.manual_seed(5)
    return FusedNet(ActionMaskModel(obs_dim=31).value, precision="fp32")


def _all_columns(env, buf):
    rec = env.rows_from_planar(buf.records) if buf.planar else buf.records
    return dict(records=rec, actions=buf.actions, logp=buf.logp, values=buf.values, final_rewards=buf.final_rewards, episode_end=buf.episode_end)


# ---------------------------------------------------------------- 1. the arena is the training rollout when it should be
@pytest.mark.parametrize("N,B,layout", SHAPES, ids=IDS)
def test_all_seats_sampling_one_net_gives_the_training_rollouts_six_columns(N, B, layout):
    import torch

    from skyjo_rl_amd import arena
    from skyjo_rl_amd.rollout import RolloutBuffer, collect

    T = 24
    nets = _nets()
    env, twin = _engine(N, B, layout), _engine(N, B, layout)
    want, got = RolloutBuffer(twin, T), RolloutBuffer(env, T)
    for b in (want, got):                                       # (every byte the calls must write starts out different)
        b.logp.fill_(7.0), b.values.fill_(-7.0), b.actions.fill_(-5)
    collect(twin, nets["A"], nets["V"], want, seed=SEED, first_ticket=TICKET0)
    assert arena.collect(env, [("sample", nets["A"])] * N, [nets["V"]] * N, got, seed=SEED, first_ticket=TICKET0) is got
    for (name, a), b in zip(_all_columns(env, got).items(), _all_columns(twin, want).values()):
        assert a.shape == b.shape and torch.equal(_bits(a), _bits(b)), name
    c, w = env.counters(), twin.counters()
    assert tuple(got.values.shape) == (T + 1, B, 1) and all(c[k] == w[k] for k in ("steps", "episodes", "resets")) and c["illegal"] == 0
    env.close()
    twin.close()


# ---------------------------------------------------------------- 2. synthetic records, mixed seats, one iteration
PATTERN = [("sample", "A"), ("greedy", "B"), "random", ("greedy", "A"), ("sample", "B"), "random"]
VALUE_PATTERN = ["V", "W", None, "W", "V", "V"]
ACT_CASES = [(N, indirect, planar) for N in ref.ARENA_N for indirect in (True, False) for planar in (False, True)]


def _act_specs(N, indirect):
    """[(seats, values)] of one geometry: names of the nets, resolved by ``_synthetic_nets``.  Two seats cannot hold two value nets AND
    a seat without one: N = 2 has a second assignment."""
    if not indirect:
        return [(["random"] * N, [None] * N)]
    if N == 2:
        return [([("sample", "A"), ("greedy", "B")], ["V", None]), ([("greedy", "A"), ("sample", "B")], ["W", "V"])]
    return [([PATTERN[s % 6] for s in range(N)], [VALUE_PATTERN[s % 6] for s in range(N)])]


def _synthetic_nets():
    w = net_ref.weights
    nets = {k: _net(w((31, 26), k), "fp32", key=((31, 26), k)) for k in ("A", "B")}
    nets["V"] = _net(w((31, 1), "A"), "fp32", key=((31, 1), "A"))
    nets["W"] = _net(w((31, 1), "B"), "fp32", key=((31, 1), "B"))
    return nets


def _act(env, seats, values, rec, planar, seed, ticket, values_only=False):
    """arena.act into guarded, prefilled outputs: (actions, logp, values) as numpy - float columns as uint32 bits as well."""
    import torch

    from skyjo_rl_amd import arena

    B = env.num_envs
    a, lp, v = _guarded((B,), torch.int32), _guarded((B,), torch.float32), _guarded((B,), torch.float32)
    if values_only:
        out = arena.act(env, seats, values, rec, seed=seed, ticket=ticket, values_out=v[1], planar=planar, values_only=True)
        assert out[0] is None and out[1] is None and out[2] is v[1]
        assert bool((a[0] == 0xA5).all()) and bool((lp[0] == 0xA5).all())
    else:
        out = arena.act(env, seats, values, rec, seed=seed, ticket=ticket, actions=a[1], logp=lp[1], values_out=v[1], planar=planar)
        assert out[0] is a[1] and out[1] is lp[1] and out[2] is v[1]
    _intact(a, lp, v)
    return a[1].cpu().numpy(), lp[1].cpu().numpy(), v[1].cpu().numpy()


@pytest.mark.parametrize("N,indirect,planar", ACT_CASES, ids=["%s-%s" % (ref.gid(N, ind), "planar" if p else "rows") for N, ind, p in ACT_CASES])
def test_act_on_synthetic_records_with_mixed_seats(handles, N, indirect, planar):
    import torch

    from skyjo_rl_amd import arena

    B = ref.ARENA_B
    seed, ticket = SEED_TICKET[1]
    g = ref.geometry(N, indirect)
    env = handles(B, N, indirect)
    nets = _synthetic_nets()
    rows, mask, agent = ref.arena_records(B, g, np.random.default_rng(700 + N + 50 * indirect))
    assert set(agent.tolist()) == set(range(N))
    rec = _dev(ref.to_planar(rows, np.random.default_rng(N)) if planar else rows)
    fwd = lambda name, width: nets[name](rec, out=torch.empty((B, width), dtype=torch.float32, device="cuda:0"), planar=planar).cpu().numpy()
    for spec, vspec in _act_specs(N, indirect):
        seats = [s if isinstance(s, str) else (s[0], nets[s[1]]) for s in spec]
        values = [None if v is None else nets[v] for v in vspec]
        act, lp, val = _act(env, seats, values, rec, planar, seed, ticket)
        # actions: arena.select's bits
        want_act = arena.select(env, seats, rec, seed=seed, ticket=ticket, planar=planar).cpu().numpy()
        assert np.array_equal(act, want_act), np.flatnonzero(act != want_act)[:8]
        # values: the seat's value net as FusedNet.__call__ evaluates it on the same records, 0.0 for the seat without one
        cols = [None if v is None else fwd(v, 1) for v in vspec]
        want_val = acr.value_by_seat(cols, agent)
        assert np.array_equal(val.view(np.uint32), want_val.view(np.uint32)), np.flatnonzero(val.view(np.uint32) != want_val.view(np.uint32))[:8]
        if None in vspec:
            assert (val.view(np.uint32)[agent == vspec.index(None)] == 0).all()
        # logp: float64 at the chosen action, from the seat's logits as its net's forward wrote them (zeros for a random seat)
        logits = {name: fwd(name, 26) for name in {s[1] for s in spec if not isinstance(s, str)}}
        want_lp = np.full(B, np.nan)
        for s, entry in enumerate(spec):
            lg = np.zeros((B, 26), dtype=np.float32) if isinstance(entry, str) else logits[entry[1]]
            here = agent == s
            want_lp[here] = acr.logp_at(lg, mask, act)[here]
        bad = acr.logp_failures(lp, want_lp)
        print("logp: largest |got - ref| %.3e" % float(np.abs(lp.astype(np.float64) - want_lp).max()))
        assert bad.size == 0, (bad[:8], lp[bad[:8]], want_lp[bad[:8]])
        for s, entry in enumerate(spec):
            if entry == "random":
                here = (agent == s) & (mask.sum(1) > 0)
                assert np.abs(lp[here] + np.log(mask[here].sum(1))).max() <= 1e-5 + 4 * 2.0 ** -24 * np.log(26)
        # a second call gives the same bits
        act2, lp2, val2 = _act(env, seats, values, rec, planar, seed, ticket)
        assert np.array_equal(act, act2) and np.array_equal(lp.view(np.uint32), lp2.view(np.uint32)) and np.array_equal(val.view(np.uint32), val2.view(np.uint32))
        # values only: the same values, no action, no logp
        _, _, val3 = _act(env, seats, values, rec, planar, seed, ticket, values_only=True)
        assert np.array_equal(val.view(np.uint32), val3.view(np.uint32))
    if indirect:
        # a greedy and a sampled seat of the same net on identical records: where they choose the same action, the same logp bits
        for name in ("A", "B"):
            s_act, s_lp, _ = _act(env, [("sample", nets[name])] * N, [None] * N, rec, planar, seed, ticket)
            g_act, g_lp, _ = _act(env, [("greedy", nets[name])] * N, [None] * N, rec, planar, seed, ticket)
            same = s_act == g_act
            assert same.sum() >= B // 8 and (~same).any()
            assert np.array_equal(s_lp.view(np.uint32)[same], g_lp.view(np.uint32)[same])
    else:
        sp, vn = arena.seat_policies(env, seats), arena.value_nets(env, values)   # no net of either kind: no workspace is allocated
        arena.act(env, sp, vn, rec, seed=seed, ticket=ticket, planar=planar)
        assert getattr(sp, "_arena_workspace", None) is None


# ---------------------------------------------------------------- 3. the bootstrap row (and every other row's value)
@functools.lru_cache(maxsize=None)
def _collected(N, B, layout, T, spec, vspec):
    """One collected buffer per shape, shared and left unchanged: (env, buf, nets by name)."""
    from skyjo_rl_amd import arena
    from skyjo_rl_amd.rollout import RolloutBuffer

    nets = dict(_nets(), W=_second_value_net())
    env = _engine(N, B, layout)
    buf = RolloutBuffer(env, T)
    buf.logp.fill_(7.0), buf.values.fill_(-7.0)
    arena.collect(env, [s if isinstance(s, str) else (s[0], nets[s[1]]) for s in spec], [None if v is None else nets[v] for v in vspec], buf,
                  seed=SEED, first_ticket=TICKET0)
    return env, buf, nets


def test_values_are_the_acting_seats_net_and_the_bootstrap_row_the_expected_seats():
    import torch

    N, B, T = 4, 130, 8
    vspec = ("V", "W", "V", "W")
    env, buf, nets = _collected(N, B, "row-major", T, (("sample", "A"), ("sample", "B"), ("greedy", "A"), "random"), vspec)
    agent = buf.views().agent.cpu().numpy()
    got = buf.values.cpu().numpy()
    for t in range(T + 1):
        cols = {k: nets[k](buf.records[t], out=torch.empty((B, 1), dtype=torch.float32, device="cuda:0")).cpu().numpy() for k in ("V", "W")}
        want = acr.value_by_seat([cols[k] for k in vspec], agent[t])
        assert np.array_equal(got[t, :, 0].view(np.uint32), want.view(np.uint32)), t
    last = agent[T]
    assert (np.isin(last, (0, 2)).any() and np.isin(last, (1, 3)).any()), "records[T] expects seats of one value net only"
    assert not np.array_equal(cols["V"], cols["W"])


# ---------------------------------------------------------------- 4. targets on a collected buffer
HANDOFF = (3, 130, "row-major", 48, (("sample", "A"), ("sample", "B"), "random"), ("V", "W", None))


def test_compute_targets_on_a_collected_buffer_is_the_recursion():
    import torch

    from skyjo_rl_amd.rollout import compute_targets
    from tests import rollout_targets_ref as tref

    env, buf, _ = _collected(*HANDOFF)
    cols = tref.columns_from_buffer(buf)
    assert len(set(cols["agent"][: buf.T].reshape(-1).tolist())) == 3
    for gamma, lam in ((0.99, 0.95), (1.0, 1.0)):
        compute_targets(buf, gamma=gamma, lam=lam)
        want = tref.targets_f32(gamma=gamma, lam=lam, **cols)
        for name, got, w in zip(("advantages", "value_targets", "returns", "flags"), (buf.advantages, buf.value_targets, buf.returns, buf.target_flags), want):
            assert torch.equal(_bits(got), _bits(torch.from_numpy(w))), (name, gamma, lam)
    assert int((buf.target_flags & 1).sum()) > 0


# ---------------------------------------------------------------- 5. select by seat on synthetic flags and records
# (T, B, N, indirect, planar): T * B = 1, 4095, 4096, 4097 around k_select_pass' 4 096 rows, and 3 x 130 with padding slots
SELECT_CASES = [(1, 1, 3, True, False), (3, 1365, 4, False, False), (2, 2048, 3, True, True), (17, 241, 4, False, True), (3, 130, 4, False, True),
                (3, 130, 3, True, False)]


def _select_seats(L, env, rec, planar, T, flags, require, mask, adv):
    import torch

    from skyjo_rl_amd import _lib

    n = flags.numel()
    index = torch.full((n + 8,), -7, dtype=torch.int64, device="cuda")
    out = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    rc = L.skyjo_vec_rollout_select_seats(env._h, rec.data_ptr(), _lib.REC_TILE_PLANAR if planar else _lib.REC_ROW_MAJOR, T, flags.data_ptr(), require, mask,
                                          adv.data_ptr() if adv is not None else None, index.data_ptr(), out.data_ptr(),
                                          out[1:].data_ptr() if adv is not None else None, env._stream())
    assert rc == 0, L.skyjo_vec_last_error()
    count = int(out[0])
    assert bool((index[count:] == -7).all())                    # only the first count entries are written
    return index[:count].cpu().numpy(), count, out[1:].view(torch.float64).cpu().numpy().copy()


@pytest.mark.parametrize("T,B,N,indirect,planar", SELECT_CASES, ids=["T%d_B%d_%s_%s" % (T, B, ref.gid(N, ind), "planar" if p else "rows") for T, B, N, ind, p in SELECT_CASES])
def test_select_seats_on_synthetic_flags_and_records(handles, T, B, N, indirect, planar):
    import torch

    from skyjo_rl_amd import _lib

    L = _lib.load()
    env = handles(B, N, indirect)
    g = ref.geometry(N, indirect)
    rng = np.random.default_rng(1000 * T + B + N)
    rows = learner_synth.records(T, B, g, rng)
    rows[..., g["mask_offset"] + 26] = rng.integers(0, N, size=(T, B))        # a random seat in every row
    agent = rows[..., g["mask_offset"] + 26].reshape(-1).copy()
    rec = _dev(learner_synth.to_planar_dirty(rows, rng) if planar else rows)
    n = T * B
    flags = learner_synth.select_flags(n, "random", rng)
    adv = learner_synth.select_advantages(n, rng)
    d_flags, d_adv = _dev(flags), _dev(adv)
    a64 = adv.astype(np.float64)
    masks = [(s,) for s in range(N)] + [tuple(range(N)), (0, N - 1) if N > 2 else (1,)]
    total = {1: 0, 3: 0}
    for require in (1, 3):
        for seats in masks:
            want, want_n, _ = acr.select_by_seat(flags, require, agent, seats)
            index, count, mom = _select_seats(L, env, rec, planar, T, d_flags, require, acr.seat_mask(seats), d_adv)
            assert count == want_n and np.array_equal(index, want), (require, seats)
            x = a64[want]
            for got, ref_sum, mag in ((mom[0], x.sum(), np.abs(x).sum()), (mom[1], (x * x).sum(), (x * x).sum())):
                bound = 2 * count * 2.0 ** -53 * mag
                print(f"n={n} require={require} seats={seats}: count={count} sum={got!r} numpy={ref_sum!r} |diff|={abs(got - ref_sum):.3e} bound={bound:.3e}")
                assert abs(got - ref_sum) <= bound
            if count == 0:
                assert mom.tolist() == [0.0, 0.0]
            index2, count2, mom2 = _select_seats(L, env, rec, planar, T, d_flags, require, acr.seat_mask(seats), d_adv)
            assert count2 == count and np.array_equal(index2, index) and mom2.tobytes() == mom.tobytes()
            if len(seats) == 1:
                total[require] += count
            if len(seats) == N:                                 # every seat: the bits of skyjo_vec_rollout_select
                idx = torch.full((n,), -7, dtype=torch.int64, device="cuda")
                out = torch.full((3,), -1, dtype=torch.int64, device="cuda")
                assert L.skyjo_vec_rollout_select(env._h, d_flags.data_ptr(), n, require, d_adv.data_ptr(), idx.data_ptr(), out.data_ptr(), out[1:].data_ptr(),
                                                  env._stream()) == 0
                assert int(out[0]) == count and np.array_equal(idx[:count].cpu().numpy(), index)
                assert out[1:].view(torch.float64).cpu().numpy().tobytes() == mom.tobytes()
                assert count == total[require]                  # the single seats' counts add up to it
        # without advantages: the same list, no moments
        index3, count3, _ = _select_seats(L, env, rec, planar, T, d_flags, require, 1, None)
        assert np.array_equal(index3, acr.select_by_seat(flags, require, agent, (0,))[0]) and count3 == index3.size
    if (T, B) == (3, 130):
        # agent bytes at and above num_players (a record the engine never writes) belong to no seat
        rows[0, ::3, g["mask_offset"] + 26] = np.array([N, 31, 32, 200, 255], dtype=np.uint8)[np.arange(len(rows[0, ::3])) % 5]
        agent = rows[..., g["mask_offset"] + 26].reshape(-1).copy()
        rec = _dev(learner_synth.to_planar_dirty(rows, rng) if planar else rows)
        want, want_n, _ = acr.select_by_seat(flags, 1, agent, range(N))
        index, count, _ = _select_seats(L, env, rec, planar, T, d_flags, 1, (1 << N) - 1, d_adv)
        assert count == want_n < int((flags & 1).sum()) and np.array_equal(index, want)


# ---------------------------------------------------------------- 6. hand-off to the per-seat learner
def test_minibatches_of_one_seat_hold_that_seats_rows():
    import torch

    from skyjo_rl_amd.rollout import compute_targets, minibatches, select_rows

    env, buf, _ = _collected(*HANDOFF)
    compute_targets(buf, gamma=0.99, lam=0.95)
    everything = select_rows(buf)
    all_rows, all_moments = everything.index.clone(), (everything.count, everything.mean, everything.std)
    sel = select_rows(buf, seats=(1,))
    index = sel.index.clone()
    agent = buf.views().agent[: buf.T].reshape(-1)
    flags = buf.target_flags.reshape(-1)
    assert torch.equal(index, (((flags & 1) != 0) & (agent == 1)).nonzero().squeeze(1)) and 256 < sel.count < everything.count
    x = buf.advantages.reshape(-1)[index].double()
    assert abs(sel.mean - float(x.mean())) <= 1e-9 and abs(sel.std - float(x.std())) <= 1e-9
    # the row ids ride through the gather in the logp column (a row id below 2^24 is a float32)
    keep = buf.logp.clone()
    buf.logp.copy_(torch.arange(buf.T * buf.B, device=keep.device, dtype=torch.float32).view(buf.T, buf.B))
    try:
        seen = []
        gen = torch.Generator(device=keep.device).manual_seed(3)
        for mb in minibatches(buf, 256, generator=gen, seats=(1,)):
            assert bool((mb.seats == 1).all()) and mb.seats.numel() <= 256
            seen.append(mb.logp.clone())
    finally:
        buf.logp.copy_(keep)
    seen = torch.cat(seen).long()
    assert seen.numel() == sel.count and torch.equal(seen.sort().values, index) and not torch.equal(seen, index)
    # seats=None is the old call: the same selection as before
    again = select_rows(buf)
    assert torch.equal(again.index, all_rows) and (again.count, again.mean, again.std) == all_moments
    with pytest.raises(ValueError, match="seat"):
        select_rows(buf, seats=(3,))
    with pytest.raises(ValueError, match="seat"):
        select_rows(buf, seats=())
    with pytest.raises(ValueError, match="selection"):
        next(minibatches(buf, 256, selection=sel, seats=(1,)))


def test_one_per_seat_update_changes_each_learners_nets_and_nobody_elses():
    import torch

    from examples.ppo import ppo_update, ppo_update_per_seat
    from skyjo_rl_amd import arena
    from skyjo_rl_amd.action_mask_model import ActionMaskModel, FusedNet
    from skyjo_rl_amd.learner import NativeAdam
    from skyjo_rl_amd.rollout import RolloutBuffer

    N, B, T = 3, 130, 48
    env = _engine(N, B)
    models, pol, val = [], [], []
    for s in range(N):
        torch.manual_seed(20 + s)
        m = ActionMaskModel(obs_dim=31).cuda()
        models.append(m), pol.append(FusedNet(m.policy)), val.append(FusedNet(m.value))
    buf = RolloutBuffer(env, T)
    arena.collect(env, [("sample", p) for p in pol], val, buf, seed=SEED, first_ticket=TICKET0)
    learners = [models[0], models[1], None]                    # seat 2 is a frozen opponent
    opts = [NativeAdam(models[s], pol[s], val[s], lr=1e-3) if learners[s] is not None else None for s in range(N)]
    params = [[p.detach().clone() for p in m.parameters()] for m in models]
    blobs = [(pol[s].export().cpu(), val[s].export().cpu()) for s in range(N)]
    res = ppo_update_per_seat(learners, buf, opts, gae=(0.99, 0.95), epochs=1, native_nets=True)
    assert res[2] is None and all(r["transitions"] > 0 for r in res[:2])
    counts = [int((((buf.target_flags & 1) != 0) & (buf.views().agent[:T] == s)).sum()) for s in range(N)]
    assert [r["transitions"] for r in res[:2]] == counts[:2]
    for s in range(N):
        changed = [not torch.equal(a, b) for a, b in zip(params[s], [p.detach() for p in models[s].parameters()])]
        now = (pol[s].export().cpu(), val[s].export().cpu())
        if learners[s] is not None:
            assert all(changed), s
            assert not torch.equal(now[0], blobs[s][0]) and not torch.equal(now[1], blobs[s][1]), s
            assert opts[s].steps == 1
        else:
            assert not any(changed) and torch.equal(now[0], blobs[s][0]) and torch.equal(now[1], blobs[s][1])
    with pytest.raises(ValueError, match="native_batches"):
        ppo_update(models[0], buf, opts[0], gae=(0.99, 0.95), seats=(0,))
    with pytest.raises(ValueError, match="entries"):
        ppo_update_per_seat(learners[:2], buf, opts[:2])
    with pytest.raises(ValueError, match="share"):
        ppo_update_per_seat([models[0], models[0], None], buf, [opts[0], opts[0], None])
    for n in pol + val:
        n.close()
    env.close()


# ---------------------------------------------------------------- 7. validation
def test_invalid_arguments_are_refused_and_leave_buffers_and_nets_alone():
    import torch

    from skyjo_rl_amd import _lib, arena
    from skyjo_rl_amd.action_mask_model import ActionMaskModel, FusedNet
    from skyjo_rl_amd.rollout import RolloutBuffer

    L = _lib.load()
    nets = dict(_nets(), W=_second_value_net())
    N, B, T = 3, 130, 4
    env = _engine(N, B)
    buf = RolloutBuffer(env, T)
    env.observe(out=buf.records[0])
    exported = {k: nets[k].export().cpu() for k in ("A", "B", "V", "W")}
    torch.manual_seed(1)
    narrow = FusedNet(ActionMaskModel(obs_dim=19).value, precision="fp32")   # a value net of another observation
    vp = lambda t: C.c_void_p(t.data_ptr())
    stream = env._stream()
    seats = arena.seat_policies(env, [("sample", nets["A"]), ("greedy", nets["B"]), "random"])
    need = int(L.skyjo_vec_arena_act_workspace_bytes(env._h, 2, 2))
    assert need == 2 * ((B * 26 * 4 + 15) // 16 * 16) + 2 * ((B * 4 + 15) // 16 * 16)
    assert int(L.skyjo_vec_arena_act_workspace_bytes(env._h, 2, 0)) == int(L.skyjo_vec_arena_workspace_bytes(env._h, 2))
    for bad in ((None, 1, 1), (env._h, -1, 0), (env._h, 13, 0), (env._h, 0, -1), (env._h, 0, 13)):
        assert int(L.skyjo_vec_arena_act_workspace_bytes(*bad)) == 0
    ws = torch.empty((need + 16,), dtype=torch.uint8, device=buf.actions.device)
    dev = buf.actions.device
    sent_a = torch.full((T, B), -77, dtype=torch.int32, device=dev)
    sent_f = torch.full((T + 1, B, 1), -77.0, dtype=torch.float32, device=dev)
    buf.actions.copy_(sent_a), buf.logp.copy_(sent_f[:T, :, 0]), buf.values.copy_(sent_f)
    rec1 = buf.records[1].clone()
    index = torch.full((T * B,), -7, dtype=torch.int64, device=dev)
    out = torch.full((3,), -1, dtype=torch.int64, device=dev)
    flags = torch.ones((T, B), dtype=torch.uint8, device=dev)
    adv = torch.zeros((T, B), dtype=torch.float32, device=dev)

    def vnets(*entries):
        arr = (C.c_void_p * N)()
        for s, net in enumerate(entries):
            arr[s] = net._h.value if net is not None else None
        return arr

    good_v = vnets(nets["V"], nets["W"], None)

    def bufs(**kw):
        f = dict(records=vp(buf.records), actions=vp(buf.actions), logp=vp(buf.logp), values=vp(buf.values), final_rewards=vp(buf.final_rewards),
                 episode_end=vp(buf.episode_end))
        f.update(kw)
        return _lib.RolloutBuffers(f["records"], f["actions"], f["logp"], f["values"], f["final_rewards"], f["episode_end"])

    def act(h=env._h, sp=seats, vn=good_v, rec=vp(buf.records[0]), layout=_lib.REC_ROW_MAJOR, a=vp(buf.actions[0]), lp=vp(buf.logp[0]), v=vp(buf.values[0]),
            w=vp(ws), wb=need):
        return L.skyjo_vec_arena_act(h, sp, vn, rec, layout, SEED, 0, a, lp, v, w, wb, stream)

    def collect(h=env._h, sp=seats, vn=good_v, T_=T, b=None, w=vp(ws), wb=need):
        b = bufs() if b is None else b
        return L.skyjo_vec_arena_collect(h, sp, vn, T_, SEED, 0, C.byref(b) if b is not False else None, w, wb, stream)

    def select(h=env._h, rec=vp(buf.records), layout=_lib.REC_ROW_MAJOR, T_=T, f=vp(flags), req=1, mask=1, a=vp(adv), idx=vp(index), cnt=vp(out), mom=vp(out[1:])):
        return L.skyjo_vec_rollout_select_seats(h, rec, layout, T_, f, req, mask, a, idx, cnt, mom, stream)

    bad_seat = (_lib.SeatPolicy * N)()
    bad_seat[0].net, bad_seat[0].kind = nets["V"]._h.value, _lib.SEAT_SAMPLE   # a policy seat whose net has one output
    bad_seat[1].kind = bad_seat[2].kind = _lib.SEAT_RANDOM
    bad_values = {"26 outputs": vnets(nets["A"], None, None), "wrong observation": vnets(nets["V"], narrow, None)}
    if torch.cuda.device_count() > 1:
        torch.manual_seed(2)
        bad_values["device"] = vnets(FusedNet(ActionMaskModel(obs_dim=31).value, device=1), None, None)
    cases = []
    for name, vn in bad_values.items():
        cases += [("act: value net, " + name, lambda vn=vn: act(vn=vn)), ("collect: value net, " + name, lambda vn=vn: collect(vn=vn))]
    cases += [
        ("act: null handle", lambda: act(h=None)), ("act: null seats", lambda: act(sp=None)), ("act: null value_nets", lambda: act(vn=None)),
        ("act: null records", lambda: act(rec=None)), ("act: null values_out", lambda: act(v=None)), ("act: a bad seat", lambda: act(sp=bad_seat)),
        ("act: actions without logp", lambda: act(lp=None)), ("act: logp without actions", lambda: act(a=None)),
        ("act: null workspace", lambda: act(w=None)), ("act: small workspace", lambda: act(wb=need - 1)), ("act: zero workspace", lambda: act(wb=0)),
        ("act: the select workspace", lambda: act(wb=int(L.skyjo_vec_arena_workspace_bytes(env._h, 2)))),
        ("act: misaligned workspace", lambda: act(w=C.c_void_p(ws.data_ptr() + 8))), ("act: bad layout", lambda: act(layout=_lib.REC_TILE_PLANAR_ALL)),
        ("act: negative layout", lambda: act(layout=-1)),
        ("act: values only, small workspace", lambda: act(a=None, lp=None, wb=need - 1)),
        ("collect: null handle", lambda: collect(h=None)), ("collect: null seats", lambda: collect(sp=None)), ("collect: null value_nets", lambda: collect(vn=None)),
        ("collect: null buffers", lambda: collect(b=False)), ("collect: a bad seat", lambda: collect(sp=bad_seat)),
        ("collect: null records", lambda: collect(b=bufs(records=None))), ("collect: null actions", lambda: collect(b=bufs(actions=None))),
        ("collect: logp missing", lambda: collect(b=bufs(logp=None))), ("collect: values missing", lambda: collect(b=bufs(values=None))),
        ("collect: null final_rewards", lambda: collect(b=bufs(final_rewards=None))), ("collect: null episode_end", lambda: collect(b=bufs(episode_end=None))),
        ("collect: T = 0", lambda: collect(T_=0)), ("collect: T < 0", lambda: collect(T_=-3)), ("collect: null workspace", lambda: collect(w=None)),
        ("collect: small workspace", lambda: collect(wb=need - 1)), ("collect: misaligned workspace", lambda: collect(w=C.c_void_p(ws.data_ptr() + 4))),
        ("select: null handle", lambda: select(h=None)), ("select: null records", lambda: select(rec=None)), ("select: null flags", lambda: select(f=None)),
        ("select: null index", lambda: select(idx=None)), ("select: null count", lambda: select(cnt=None)),
        ("select: advantages without moments", lambda: select(mom=None)), ("select: moments without advantages", lambda: select(a=None)),
        ("select: seat_mask = 0", lambda: select(mask=0)), ("select: a bit at num_players", lambda: select(mask=1 << N)),
        ("select: bits above num_players", lambda: select(mask=(1 << 12) | 1)), ("select: the top bit", lambda: select(mask=(1 << 31) | 1)),
        ("select: T = 0", lambda: select(T_=0)), ("select: T < 0", lambda: select(T_=-1)), ("select: require = 0", lambda: select(req=0)),
        ("select: require = 256", lambda: select(req=256)), ("select: bad layout", lambda: select(layout=_lib.REC_TILE_PLANAR_ALL)),
        ("select: negative layout", lambda: select(layout=-1)),
    ]
    for name, call in cases:
        rc = call()
        assert rc == -1, (name, rc)                             # SKYJO_E_INVALID
        assert L.skyjo_vec_last_error(), name
    env.sync()
    # nothing was launched: no column, record, index or count was written, the nets hold the same bytes
    assert torch.equal(buf.actions, sent_a) and torch.equal(buf.logp, sent_f[:T, :, 0]) and torch.equal(buf.values, sent_f)
    assert torch.equal(buf.records[1], rec1) and bool((index == -7).all()) and bool((out == -1).all())
    for k, b in exported.items():
        assert torch.equal(nets[k].export().cpu(), b), k
    # the good calls still work, and the engine still steps
    assert act() == 0 and act(a=None, lp=None) == 0 and collect() == 0 and select() == 0
    a, lp, v = arena.act(env, seats, good_v, buf.records[T])
    env.step(a)
    assert env.counters()["illegal"] == 0 and int(out[0]) == int((buf.views().agent[:T] == 0).sum())
    # the Python layer's own checks
    with pytest.raises(ValueError, match="planar"):
        buf.planar = True
        arena.collect(env, seats, good_v, buf)
    buf.planar = False
    with pytest.raises(ValueError, match="records"):
        arena.act(env, seats, good_v, buf.records[0][:-1])
    with pytest.raises(ValueError, match="values has"):
        arena.collect(env, seats, [nets["V"]], buf)
    with pytest.raises(ValueError, match="FusedNet or None"):
        arena.collect(env, seats, [nets["V"], "W", None], buf)
    with pytest.raises(ValueError, match="values_only"):
        arena.act(env, seats, good_v, buf.records[0], actions=buf.actions[0], values_only=True)
    narrow.close()
    env.close()


# ---------------------------------------------------------------- 8. stream
def test_collect_on_a_side_stream_gives_the_same_bits():
    """collect and the read of its columns are queued on one non-default stream; only that stream is waited for."""
    import torch

    from skyjo_rl_amd import arena
    from skyjo_rl_amd.rollout import RolloutBuffer

    N, B, layout, T, spec, vspec = HANDOFF
    _, ref_buf, nets = _collected(*HANDOFF)
    want = [ref_buf.records, ref_buf.actions, ref_buf.logp, ref_buf.values, ref_buf.final_rewards, ref_buf.episode_end]
    env = _engine(N, B, layout)
    side = torch.cuda.Stream(device=env.device_index)
    with torch.cuda.stream(side):
        buf = RolloutBuffer(env, T)
        arena.collect(env, [s if isinstance(s, str) else (s[0], nets[s[1]]) for s in spec], [None if v is None else nets[v] for v in vspec], buf,
                      seed=SEED, first_ticket=TICKET0)
        got = [x.clone() for x in (buf.records, buf.actions, buf.logp, buf.values, buf.final_rewards, buf.episode_end)]
        host = [torch.empty(x.shape, dtype=x.dtype, pin_memory=True) for x in got]
        for h, x in zip(host, got):
            h.copy_(x, non_blocking=True)
    side.synchronize()
    for name, a, b in zip(("records", "actions", "logp", "values", "final_rewards", "episode_end"), host, want):
        assert torch.equal(_bits(a), _bits(b)), name
    env.close()
