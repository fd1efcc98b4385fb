"""The three learner kernels (``k_rollout_targets``, ``k_select_pass`` / ``k_select_scan``, ``k_gather_rows``) on the synthetic buffers
of tests/learner_synth.py, through the C ABI alone: the edges a rollout never reaches.  A ``SkyjoVecEnv`` per (B, N, observation mode)
serves as the handle only - no rollout, no model.  What the inputs reach is asserted without a GPU in tests/test_learner_synth.py.

Every output is allocated with a guard tail of GUARD elements and prefilled - floats with a NaN that carries a payload, integers
with a sentinel, bytes with 0xA5.  After the call the tail must be untouched and the head must hold the restatement's bits: a zero
of the restatement must be a zero that the kernel wrote, never a sentinel it left."""
import types

import numpy as np
import pytest

from tests import learner_synth as synth
from tests import rollout_batches_ref as bref
from tests import rollout_targets_ref as tref

pytestmark = pytest.mark.gpu

GUARD = 64
NAN_BITS = 0x7FC0BEEF                 # a quiet NaN with a payload
INT_SENTINEL = -0x0123456789ABCDEF
BYTE_SENTINEL = 0xA5


@pytest.fixture(scope="module")
def handles():
    """SkyjoVecEnv per (B, N, indirect), made on first use and closed with the module."""
    from skyjo_rl_amd import SkyjoVecEnv

    made = {}

    def get(B, N, indirect=True):
        key = (B, N, indirect)
        if key not in made:
            env = made[key] = SkyjoVecEnv(B, num_players=N, observe_other_player_indirect=indirect)
            g = synth.geometry(N, indirect)
            assert (env.num_envs, env.num_players, env.obs_dim, env.mask_offset, env.record_bytes, env.tiles) == \
                (B, N, g["obs_dim"], g["mask_offset"], g["record_bytes"], (B + 63) // 64)
        return made[key]

    yield get
    for env in made.values():
        env.close()


def _guarded(n, dtype):
    """A prefilled device tensor of n + GUARD elements."""
    import torch

    if dtype == torch.float32:
        return torch.full((n + GUARD,), NAN_BITS, dtype=torch.int32, device="cuda").view(torch.float32)
    return torch.full((n + GUARD,), BYTE_SENTINEL if dtype == torch.uint8 else INT_SENTINEL, dtype=dtype, device="cuda")


def _bits(t):
    import torch

    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _assert_guarded(got, n, want, what):
    """Head == the restatement bit for bit (``want``: numpy, any shape of n elements), tail untouched."""
    import torch

    w = torch.from_numpy(np.ascontiguousarray(want).reshape(-1))
    assert w.numel() == n and w.dtype == got.dtype, (what, w.dtype, got.dtype)
    assert torch.equal(_bits(got[:n]).cpu(), _bits(w)), what
    tail = _bits(got[n:]).cpu()
    fill = NAN_BITS if got.dtype == torch.float32 else BYTE_SENTINEL if got.dtype == torch.uint8 else INT_SENTINEL
    assert tail.numel() == GUARD and bool((tail == fill).all()), (what, "guard tail written")


def _strided(col, stride):
    """float32 [..., stride] on the device: component 0 = col, the others the NaN sentinel."""
    import torch

    out = torch.full((col.size, stride), NAN_BITS, dtype=torch.int32).view(torch.float32)
    out[:, 0] = torch.from_numpy(np.ascontiguousarray(col).reshape(-1))
    return out.cuda()


# ---------------------------------------------------------------------------------------------------------------- targets
def _run_targets(L, env, rec, layout, T, values, stride, rewards, end, gamma, lam):
    import torch

    n = T * env.num_envs
    out = [_guarded(n, torch.float32) for _ in range(3)] + [_guarded(n, torch.uint8)]
    rc = L.skyjo_vec_rollout_targets(env._h, rec.data_ptr(), layout, T, values.data_ptr(), stride, rewards.data_ptr(), end.data_ptr(),
                                     gamma, lam, *(o.data_ptr() for o in out), env._stream())
    assert rc == 0
    return out


@pytest.mark.parametrize("T,B,N", synth.TARGET_CASES)
def test_targets_bitwise(handles, T, B, N):
    """All four columns bit for bit ``targets_f32``'s, in both layouts (the planar one with dirty padding), with value_stride 1 and
    3, for the five (gamma, lambda) pairs: T on both sides of the 16-step block and of its multiples, B on both sides of the
    wavefront (B = 1 included: the engine refuses only num_envs <= 0), every player count - the register forms 2 .. 4 and the LDS form."""
    import torch

    from skyjo_rl_amd import _lib

    L = _lib.load()
    env = handles(B, N)
    for seed in synth.target_seeds(T, B, N):
        case = synth.targets_case(T, B, N, seed)
        c = case["cols"]
        recs = ((_lib.REC_ROW_MAJOR, torch.from_numpy(case["records"]).cuda()), (_lib.REC_TILE_PLANAR, torch.from_numpy(case["planar"]).cuda()))
        values = {s: _strided(c["values"], s) for s in (1, 3)}
        rewards, end = torch.from_numpy(c["final_rewards"]).cuda(), torch.from_numpy(c["episode_end"]).cuda()
        for gamma, lam in synth.PARAMS:
            want = tref.targets_f32(gamma=gamma, lam=lam, **c)
            for layout, rec in recs:
                for stride in (1, 3):
                    got = _run_targets(L, env, rec, layout, T, values[stride], stride, rewards, end, gamma, lam)
                    for name, g, w in zip(("advantages", "value_targets", "returns", "flags"), got, want):
                        _assert_guarded(g, T * B, w, (T, B, N, seed, gamma, lam, layout, stride, name))


def test_targets_within_textbook_bound(handles):
    """One synthetic case (T = 48, B = 65, N = 3, dirty planar, value_stride 3) against the float64 textbook GAE, within the bound
    tests/test_rollout_targets_ref.py derives: 4 L 2^-24 M."""
    import torch

    from skyjo_rl_amd import _lib

    T, B, N = 48, 65, 3
    case = synth.targets_case(T, B, N, synth.target_seeds(T, B, N)[0])
    c = case["cols"]
    adv, tgt, _, flags = _run_targets(_lib.load(), handles(B, N), torch.from_numpy(case["planar"]).cuda(), _lib.REC_TILE_PLANAR, T,
                                      _strided(c["values"], 3), 3, torch.from_numpy(c["final_rewards"]).cuda(),
                                      torch.from_numpy(c["episode_end"]).cuda(), 0.99, 0.95)
    adv64, tgt64, has64, info = tref.targets_f64(gamma=0.99, lam=0.95, **c)
    M = max(float(np.abs(c["values"]).max()), float(np.abs(c["final_rewards"]).max()))
    bound = 4 * info["longest"] * 2.0 ** -24 * M
    a, v, f = (x[:T * B].cpu().numpy().reshape(T, B) for x in (adv, tgt, flags))
    err = max(float(np.abs(a - adv64).max()), float(np.abs(v - tgt64).max()))
    print(f"textbook on synthetic columns: L={info['longest']} M={M:.4f} bound={bound:.3e} max error={err:.3e}")
    assert np.array_equal((f & 1) != 0, has64) and int(has64.sum()) > 0 and err <= bound


# ---------------------------------------------------------------------------------------------------------------- select
def _select(L, env, flags, require, adv, index):
    """One native selection into ``index`` (guarded, prefilled by the caller): count, moments (float64 [2]), and the raw out words."""
    import torch

    out = _guarded(3, torch.int64)
    rc = L.skyjo_vec_rollout_select(env._h, flags.data_ptr(), flags.numel(), require, adv.data_ptr() if adv is not None else None,
                                    index.data_ptr(), out.data_ptr(), out[1:].data_ptr() if adv is not None else None, env._stream())
    assert rc == 0
    host = out.cpu()
    assert bool((host[3:] == INT_SENTINEL).all()) and (adv is not None or bool((host[1:] == INT_SENTINEL).all()))
    return int(host[0]), host[1:3].view(torch.float64).numpy().copy()


def _check_select(L, env, n, pattern, requires, with_adv=True):
    """Index and count are ``torch.nonzero``'s, ``index[count:]`` and the guard keep their prefill; the sums lie within
    2 count 2^-53 sum|x| of numpy's float64 sums (the bound of test_gpu_rollout_batches.py); a second call gives the same bits."""
    import torch

    rng = np.random.default_rng(n % 1000 + len(pattern))
    f_np = synth.select_flags(n, pattern, rng)
    a_np = synth.select_advantages(n, rng)
    flags = torch.from_numpy(f_np).cuda()
    adv = torch.from_numpy(a_np).cuda() if with_adv else None
    for require in requires:
        index = _guarded(n, torch.int64)
        count, mom = _select(L, env, flags, require, adv, index)
        want = ((flags & require) == require).nonzero().squeeze(1)
        assert count == want.numel(), (n, pattern, require, count, want.numel())
        assert torch.equal(index[:count], want), (n, pattern, require)
        assert bool((index[count:] == INT_SENTINEL).all()), (n, pattern, require, "index[count:] written")
        if with_adv:
            x = a_np[want.cpu().numpy()].astype(np.float64)
            for got, ref_sum, mag in ((mom[0], x.sum(), np.abs(x).sum()), (mom[1], (x * x).sum(), (x * x).sum())):
                bound = 2 * count * 2.0 ** -53 * mag
                print(f"n={n} {pattern} require={require}: count={count} sum={got!r} numpy={ref_sum!r} |diff|={abs(got - ref_sum):.3e} bound={bound:.3e}")
                assert abs(got - ref_sum) <= bound
            if count == 0:
                assert mom.tolist() == [0.0, 0.0]
        index2 = _guarded(n, torch.int64)
        count2, mom2 = _select(L, env, flags, require, adv, index2)
        assert count2 == count and torch.equal(index2, index) and (not with_adv or mom2.tobytes() == mom.tobytes())
    return flags, adv


@pytest.fixture(scope="module")
def select_env():
    """ONE handle for the select tests below, which run in ascending and then descending size: the block scratch of the handle is
    allocated, grown three times and then reused."""
    from skyjo_rl_amd import SkyjoVecEnv

    env = SkyjoVecEnv(64)
    yield env
    env.close()


@pytest.mark.parametrize("n", sorted(synth.SELECT_SIZES))
def test_select_beyond_1024_blocks_ascending(select_env, n):
    """1 024 blocks (every thread of the scan owns one, the last block one row or full), 1 025 and 2 049 (threads own two or
    three blocks, trailing threads none): all six flag patterns, require 1, 2 and 3."""
    from skyjo_rl_amd import _lib

    for pattern in synth.SELECT_PATTERNS:
        _check_select(_lib.load(), select_env, n, pattern, (1, 2, 3))


def test_select_workload_shape(select_env):
    """65 536 x 320 rows: 5 120 blocks, five per thread of the scan - the shape the benchmarks quote."""
    from skyjo_rl_amd import _lib

    _check_select(_lib.load(), select_env, synth.WORKLOAD_ROWS, "random", (1,))


class _StandInBuffer:
    """What ``rollout.select_rows`` asks of a buffer, around synthetic columns: T x B rows of 64-byte records that are never read."""

    def __init__(self, env, T, B, flags, adv):
        import torch

        self.T, self.B, self._env, self.planar = T, B, env, False
        self.records = torch.empty((T + 1, B, env.record_bytes), dtype=torch.uint8, device="cuda")
        self.actions = torch.empty((1,), dtype=torch.int32, device="cuda")
        self.target_flags, self.advantages = flags.view(T, B), adv.view(T, B)


@pytest.mark.parametrize("n", sorted(synth.SELECT_SIZES, reverse=True)[1:])
def test_select_descending_reuses_scratch(select_env, n):
    """The same handle at shrinking sizes (the scratch is reused, its tail is stale): the random pattern, with and without
    advantages; and at 1 024 x 4 096 rows through ``rollout.select_rows`` on a stand-in buffer, whose mean / std must be
    ``mean_std`` of numpy's float64 sums within the bound of the sums, propagated: with es, eq the bounds of the two sums,
    |mean - mean'| <= es / n + 2^-53 |mean'|, and since std^2 - std'^2 is the difference of the variances,
    |std - std'| <= dvar / (std + std') + 2^-52 std' with dvar = (eq + (2 |s| es + es^2) / n + 4 2^-53 q) / (n - 1)."""
    import torch

    from skyjo_rl_amd import _lib
    from skyjo_rl_amd.rollout import select_rows

    L = _lib.load()
    flags, adv = _check_select(L, select_env, n, "random", (1,))
    _check_select(L, select_env, n, "random", (2,), with_adv=False)
    if n % synth.SEL_ROWS:
        return
    B = 4096
    buf = _StandInBuffer(select_env, n // B, B, flags, adv)
    for require in (1, 3):
        sel = select_rows(buf, require=require)
        want = ((flags & require) == require).nonzero().squeeze(1)
        assert sel.count == want.numel() > 1 and torch.equal(sel.index, want) and sel.index.data_ptr() == buf.row_index.data_ptr()
        x = adv.cpu().numpy()[want.cpu().numpy()].astype(np.float64)
        s, q, c = float(x.sum()), float((x * x).sum()), sel.count
        mean, std = bref.mean_std(s, q, c)
        es, eq = 2 * c * 2.0 ** -53 * float(np.abs(x).sum()), 2 * c * 2.0 ** -53 * q
        dvar = (eq + (2 * abs(s) * es + es * es) / c + 4 * 2.0 ** -53 * q) / (c - 1)
        bm, bs = es / c + 2.0 ** -53 * abs(mean), dvar / (sel.std + std) + 2.0 ** -52 * std
        print(f"select_rows require={require}: mean={sel.mean!r} numpy={mean!r} bound={bm:.3e}; std={sel.std!r} numpy={std!r} bound={bs:.3e}")
        assert abs(sel.mean - mean) <= bm and abs(sel.std - std) <= bs


# ---------------------------------------------------------------------------------------------------------------- gather
NAMES = ("observations", "log_mask", "actions", "logp", "advantages", "value_targets", "values", "seats")


@pytest.mark.parametrize("N,indirect", synth.GATHER_GEOMETRIES)
def test_gather_bitwise(handles, N, indirect):
    """All eight outputs bit for bit ``rollout_batches_ref.gather``'s at B = 200, T = 3: every record size, both layouts (dirty
    planar), value_stride 1 and 2, m on both sides of the 64-row workgroup, permuted / partial-tile / out-of-range / interleaved /
    repeated row ids, the identity normalisation and one that rounds; no store past m * D, m * 26 or m."""
    import torch

    from skyjo_rl_amd import _lib

    L = _lib.load()
    B, T = synth.GATHER_B, synth.GATHER_T
    env = handles(B, N, indirect)
    case = synth.gather_case(N, indirect)
    g, cols = case["geometry"], case["cols"]
    D, rb = g["obs_dim"], g["record_bytes"]
    recs = ((_lib.REC_ROW_MAJOR, torch.from_numpy(case["records"]).cuda()), (_lib.REC_TILE_PLANAR, torch.from_numpy(case["planar"]).cuda()))
    dev = {k: torch.from_numpy(v).cuda() for k, v in cols.items() if k != "values"}
    values = {s: _strided(cols["values"], s) for s in (1, 2)}
    dtypes = (torch.float32, torch.float32, torch.int64, torch.float32, torch.float32, torch.float32, torch.float32, torch.uint8)
    for what, index_np in case["lists"].items():
        m = index_np.size
        index = torch.from_numpy(index_np).cuda()
        sizes = (m * D, m * 26, m, m, m, m, m, m)
        for mean, std in synth.GATHER_NORMS:
            want = bref.gather(case["records"], False, rb, D, B, T, B, index_np, mean=mean, std=std, **cols)
            for layout, rec in recs:
                for stride in (1, 2):
                    out = [_guarded(n, dt) for n, dt in zip(sizes, dtypes)]
                    rc = L.skyjo_vec_rollout_gather(env._h, rec.data_ptr(), layout, T, index.data_ptr(), m, dev["actions"].data_ptr(),
                                                    dev["logp"].data_ptr(), values[stride].data_ptr(), stride, dev["advantages"].data_ptr(),
                                                    dev["value_targets"].data_ptr(), mean, std, *(o.data_ptr() for o in out), env._stream())
                    assert rc == 0
                    for name, o, n in zip(NAMES, out, sizes):
                        _assert_guarded(o, n, want[name], (N, indirect, what, mean, std, layout, stride, name))


def test_gather_cases_reach_every_piece_count(handles):
    """The handles of the gather cases have every record size the engine offers: record_bytes / 16 from 4 to 13."""
    reached = set(handles(synth.GATHER_B, N, ind).record_bytes // 16 for N, ind in synth.GATHER_GEOMETRIES)
    offered = set(synth.geometry(N, ind)["record_bytes"] // 16 for N in range(1, 13) for ind in (True, False))
    assert reached == offered, (sorted(reached), sorted(offered))
