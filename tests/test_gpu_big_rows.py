"""Every row-count kernel of the caller's and the learner's side past 2^31 and 2^32: include/skyjo_vec.h takes row counts as int64_t, and
here each call is made ONCE at the smallest row count that carries one of its arrays across byte 2^31, byte 2^32 or element 2^31
(tests/big_rows.py has the plans, tests/test_big_rows.py holds them and the checks without a GPU).  Content is periodic with the prime
period 4099; a kernel whose output row depends on its input row alone is compared on its first period with the CPU reference the
kernel's own test uses, and then WHOLE, on the device, with its own first period tiled; what depends on the row id (the draws, the
selection, the gathers, the episode ends) is compared with the reference in the windows around every mark.  Outputs lie between guard
bytes and are prefilled with the guard's byte.  Every test stays below 16 GiB of device memory and frees what it took.

References: record_ref.unpack_ref, net_ref.check_forward / check_draw, rollout_targets_ref, rollout_batches_ref.gather, ppo_loss_ref /
ppo_loss_kl_ref, arena_ref.episode_sums, and the definitions of skyjo_vec_rollout_select / _gather_logits restated in two lines of
numpy.  Nothing is compared with the kernel under test at another size, but for the one case named at the end.

Left out on purpose:
  skyjo_vec_mlp_train_* and skyjo_vec_ppo_update   their 256-wide float32 workspaces reach 2^32 bytes only with four arrays of 4.3 GB
                                                   each, over the cap; minibatches are at most 32 768 rows everywhere in the project
  skyjo_vec_rollout_shuffle                        capped at 2^30 rows (SKE_MAX_COUNT), which tests/test_gpu_ppo_update_native.py holds
  kernels sized by num_envs alone                  (episode_ends, the arena) skyjo_vec_create bounds them

``rollout.collect`` is the one case whose reference is the product itself, at low offsets (tests/big_rows.py: SELF_REFERENCED)."""
import ctypes as C
import gc
import time

import numpy as np
import pytest

from tests import arena_ref, learner_synth, net_ref, ppo_loss_kl_synth, ppo_loss_synth
from tests import rollout_batches_ref as bref
from tests import big_rows as br
from tests import record_ref as ref
from tests.test_gpu_net_synthetic import HIGH_ID0, SEED_TICKET, _net
from tests.test_gpu_ppo_loss import F32_DEVIATION, MARGIN
from tests.test_gpu_ppo_loss_kl import F32_DEVIATION as F32_DEVIATION_KL

pytestmark = pytest.mark.gpu

POOL, GUARD, FILL = br.POOL, br.GUARD, br.FILL
FILL32 = int(np.array([FILL] * 4, dtype=np.uint8).view(np.int32)[0])
FILL64 = int(np.array([FILL] * 8, dtype=np.uint8).view(np.int64)[0])


@pytest.fixture(autouse=True)
def memory_and_time(request):
    """The cap is a condition: peak allocation of the test <= 16 GiB, everything freed afterwards.  Wall time and peak are printed."""
    import torch

    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    peak = torch.cuda.max_memory_allocated()
    gc.collect()
    torch.cuda.empty_cache()
    print("BIG_ROWS %s: wall %.2f s, max_memory_allocated %.2f GiB" % (request.node.name, wall, peak / br.GIB))
    assert peak <= br.CAP, "%.2f GiB allocated" % (peak / br.GIB)


def _vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _guarded(shape, dtype):
    """(whole uint8 allocation, view of ``shape`` / ``dtype`` inside it), every byte FILL."""
    import torch

    shape = tuple(shape)
    nbytes = int(np.prod(shape, dtype=np.int64)) * torch.empty((), dtype=dtype).element_size()
    whole = torch.full((nbytes + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda:0")
    return whole, whole[GUARD:GUARD + nbytes].view(dtype).view(shape)


def _intact(*bufs):
    for whole, view in bufs:
        nbytes = view.numel() * view.element_size()
        assert bool((whole[:GUARD] == FILL).all()) and bool((whole[GUARD + nbytes:] == FILL).all()), "a guard byte was written"


def _filled(n, pool):
    """A device array of n rows, row r = pool[r % POOL] (pool: numpy [POOL, ...])."""
    import torch

    p = _dev(pool)
    assert p.shape[0] == POOL
    return br.fill_periodic(torch.empty((n,) + tuple(p.shape[1:]), dtype=p.dtype, device="cuda:0"), p)


def _filled_planar(n, pool):
    """Tile-planar blocks uint8 [ceil(n / 64), P, 64, 16] whose record r is pool[r % POOL]; the slots of the last tile beyond n hold
    the pool's next rows (dirty padding).  One super-period is POOL tiles - 64 POOL rows - laid out on the host."""
    import torch

    rb = pool.shape[1]
    rows = pool[np.arange(64 * POOL) % POOL]
    period = np.ascontiguousarray(rows.reshape(POOL, 64, rb // 16, 16).transpose(0, 2, 1, 3))
    assert np.array_equal(ref.rows_from_planar(period[:3], 130), rows[:130])         # record_ref's address formula
    assert period.nbytes <= br.CHUNK_BYTES
    tiles = (n + 63) // 64
    return br.fill_periodic(torch.empty((tiles, rb // 16, 64, 16), dtype=torch.uint8, device="cuda:0"), _dev(period))


def _periodic(name, out, first=None):
    bad, where = br.periodic_mismatches(out, first=first)
    assert bad == 0, "%s: %d rows differ from their row of the first period, first at row %d" % (name, bad, where)


def _marks(name):
    case = br.CASES[name]
    wins = br.windows(case["n"], case["arrays"])
    print("BIG_ROWS %s: n = %d, marks %s, windows %s" % (name, case["n"], ", ".join("%s %s row %d" % m for m in br.mark_rows(case["n"], case["arrays"])),
                                                        " ".join("[%d, %d)" % w for w in wins)))
    assert all(a[1] <= b[0] for a, b in zip(wins, wins[1:])), "windows overlap"
    return case["n"], wins


# ---------------------------------------------------------------- 1. unpack
@pytest.mark.parametrize("kind", ["rows", "tiles"])
def test_unpack_past_4_gib(kind):
    """skyjo_vec_unpack / _unpack_tiles, direct observation with 12 players (208-byte records, 163 observation bytes): the records cross
    byte 2^31 and 2^32, obs crosses element 2^31 and byte 2^32.  Bit for bit against ``record_ref.unpack_ref``."""
    import torch

    from skyjo_rl_amd import SkyjoVecEnv, _lib

    L = _lib.load()
    n, _ = _marks("unpack-" + kind)
    g = ref.geometry(12, False)
    D, rb = g["obs_dim"], g["record_bytes"]
    assert (D, rb) == (163, 208)
    pool = ref.consumer_records(POOL, g, np.random.default_rng(1201))
    assert np.unique(pool, axis=0).shape[0] == POOL
    env = SkyjoVecEnv(64, num_players=12, observe_other_player_indirect=False)
    try:
        assert (env.obs_dim, env.record_bytes) == (D, rb)
        rec = _filled(n, pool) if kind == "rows" else _filled_planar(n, pool)
        shapes = dict(obs=((n, D), torch.int8), mask=((n, 26), torch.int8), **{k: ((n,), torch.uint8) for k in ref.UNPACK_NAMES[2:]})
        outs = {k: _guarded(*shapes[k]) for k in ref.UNPACK_NAMES}
        fn, count = (L.skyjo_vec_unpack, n) if kind == "rows" else (L.skyjo_vec_unpack_tiles, n // 64)
        assert fn(env._h, _vp(rec), count, *[_vp(outs[k][1]) for k in ref.UNPACK_NAMES], env._stream()) == 0
        torch.cuda.synchronize()
        _intact(*outs.values())
        got = {k: v[1][:POOL].cpu().numpy() for k, v in outs.items()}
        assert ref.unpack_mismatches(got, ref.unpack_ref(pool, g)) == []
        for k, v in outs.items():
            _periodic(k, v[1])
    finally:
        env.close()


# ---------------------------------------------------------------- 2. the net's forward
@pytest.mark.parametrize("precision,planar", [("fp32", False), ("bf16", True)], ids=["rows-fp32", "planar-bf16"])
def test_forward_past_4_gib(precision, planar):
    """skyjo_vec_mlp_forward_layout on 2^26 + 4099 indirect records (4 GiB) with 26 outputs (the output crosses byte 2^32 near row
    41.3 M): ``net_ref.check_forward`` on the first period, the whole output against that period."""
    import torch

    n, _ = _marks("forward-planar-bf16" if planar else "forward-rows-fp32")
    case = net_ref.forward_case((31, 26), "A")
    net = _net(case["params"], precision, key=((31, 26), "A"))
    pool = np.array(case["pool"])
    rec = _filled_planar(n, pool) if planar else _filled(n, pool)
    out = _guarded((n, 26), torch.float32)
    assert net(rec, out=out[1], planar=planar) is out[1]
    torch.cuda.synchronize()
    _intact(out)
    assert net_ref.check_forward(out[1][:POOL].cpu().numpy(), case, precision) == []
    _periodic("out", out[1])


# ---------------------------------------------------------------- 3. the one-lane draw
def _draw_subcase(pool_case, rows, seed, ticket, game_id0):
    """``pool_case`` (net_ref.draw_case of POOL rows) restated for the rows ``rows`` of the periodic buffer: their uniforms are those of
    the ids game_id0 + row."""
    idx = rows % POOL
    with np.errstate(over="ignore"):
        gid = np.uint64(game_id0) + rows.astype(np.uint64)
    u = net_ref.uniform(seed, ticket, gid)
    c = dict(n=rows.size, seed=seed, ticket=ticket, game_id0=game_id0, no_masking=False, mask=pool_case["mask"][idx],
             mask_family=pool_case["mask_family"][idx], logits=pool_case["logits"][idx], logit_family=pool_case["logit_family"][idx], u=u)
    c["ref"] = net_ref.draw_reference(c["logits"], c["mask"], u, False)
    return c


@pytest.mark.parametrize("planar", [False, True], ids=["rows", "planar"])
def test_sample_actions_past_element_2_31(planar):
    """skyjo_vec_sample_actions_layout: row-major at the smallest n whose logits cross ELEMENT 2^31 (82.6 M rows; the records cross byte
    2^32 on the way), tile-planar at 2^26 + 4099.  game_id0 = 2^32 - 100: the ids' high word changes inside the first window.  In the
    windows ``net_ref.check_draw`` with the uniforms of the rows' own ids, bit for bit; everywhere: no sentinel left, every action in
    0 .. 25, every uniform in [0, 1)."""
    import torch

    from skyjo_rl_amd import SkyjoVecEnv, _lib

    L = _lib.load()
    n, wins = _marks("sample-planar" if planar else "sample-rows")
    seed, ticket = SEED_TICKET[2]
    pc = net_ref.draw_case(POOL, seed, ticket)
    env = SkyjoVecEnv(64, game_id0=HIGH_ID0)
    try:
        assert (env.mask_offset, env.record_bytes) == (pc["mask_offset"], 64)
        rec = _filled_planar(n, pc["records"]) if planar else _filled(n, pc["records"])
        logits = _filled(n, pc["logits"])
        a, lp, u = _guarded((n,), torch.int32), _guarded((n,), torch.float32), _guarded((n,), torch.float32)
        rc = L.skyjo_vec_sample_actions_layout(env._h, _vp(rec), _lib.REC_TILE_PLANAR if planar else _lib.REC_ROW_MAJOR, _vp(logits), n, seed, ticket,
                                               0, _vp(a[1]), _vp(lp[1]), _vp(u[1]), env._stream())
        assert rc == 0
        torch.cuda.synchronize()
        _intact(a, lp, u)
        for name, t in (("actions", a[1]), ("logp", lp[1]), ("uniform", u[1])):
            assert br.window_mismatches(t.view(torch.int32), [], None, sentinel=FILL32)[1] == 0, name + " has elements the kernel did not write"
        assert int(a[1].min()) >= 0 and int(a[1].max()) <= 25 and float(u[1].min()) >= 0.0 and float(u[1].max()) < 1.0
        rows = br.window_rows(wins)
        idx = _dev(rows)
        sub = _draw_subcase(pc, rows, seed, ticket, HIGH_ID0)
        assert (sub["u"] != net_ref.uniform(seed, ticket, rows.astype(np.uint64))).any()      # (game_id0 matters)
        assert net_ref.check_draw(a[1][idx].cpu().numpy(), lp[1][idx].cpu().numpy(), u[1][idx].cpu().numpy(), sub) == []
    finally:
        env.close()


# ---------------------------------------------------------------- 6. select
def test_select_row_ids_past_2_31():
    """skyjo_vec_rollout_select over 2^31 + 4099 one-byte flags with the advantages beside them (8.6 GB: they cross byte 2^32 and element
    2^31): islands in the windows - the first and the last block and around rows 2^30 and 2^31 - so the index stays small.  Row ids from
    2^31 on come out exact and in order, the count is ==, the moments lie within the bound of tests/test_gpu_rollout_batches.py."""
    import torch

    from skyjo_rl_amd import SkyjoVecEnv, _lib

    L = _lib.load()
    n, wins = _marks("select")
    rng = np.random.default_rng(631)
    flag_pool = (rng.integers(0, 256, size=POOL, dtype=np.uint8) & 0xFC)[:, None]       # bits 0 / 1 clear outside the islands
    adv_pool = (rng.standard_normal(POOL).astype(np.float32) * np.float32(25.0))[:, None]
    env = SkyjoVecEnv(64)
    try:
        flags, adv = _filled(n, flag_pool).view(n), _filled(n, adv_pool).view(n)
        islands = {}
        for lo, hi in wins:
            islands[lo] = rng.integers(0, 256, size=hi - lo, dtype=np.uint8)
            islands[lo][0] |= 3
            flags[lo:hi] = _dev(islands[lo])
        assert any(lo >= 2 ** 31 for lo, _ in wins) and any(lo < 2 ** 31 < hi for lo, hi in wins)
        room = sum(hi - lo for lo, hi in wins)
        for require in (1, 3):
            want = np.concatenate([lo + np.flatnonzero((islands[lo] & require) == require) for lo, _ in wins]).astype(np.int64)
            assert want.size < room and (np.diff(want) > 0).all() and (want >= 2 ** 31).any()
            index, out = _guarded((room,), torch.int64), _guarded((3,), torch.int64)
            rc = L.skyjo_vec_rollout_select(env._h, _vp(flags), n, require, _vp(adv), _vp(index[1]), _vp(out[1]), _vp(out[1][1:]), env._stream())
            assert rc == 0
            torch.cuda.synchronize()
            _intact(index, out)
            count = int(out[1][0])
            assert count == want.size, (require, count, want.size)
            got = index[1].cpu().numpy()
            assert np.array_equal(got[:count], want), (require, np.flatnonzero(got[:count] != want)[:4])
            assert (got[count:] == FILL64).all(), "index[count:] written"
            mom = out[1][1:3].view(torch.float64).cpu().numpy()
            x = adv_pool[want % POOL, 0].astype(np.float64)
            for got_sum, ref_sum, mag in ((mom[0], x.sum(), np.abs(x).sum()), (mom[1], (x * x).sum(), (x * x).sum())):
                bound = 2 * count * 2.0 ** -53 * mag
                print("require %d: count %d sum %r numpy %r |diff| %.3e bound %.3e" % (require, count, got_sum, ref_sum, abs(got_sum - ref_sum), bound))
                assert abs(got_sum - ref_sum) <= bound
    finally:
        env.close()


# ---------------------------------------------------------------- 8. gather_logits
def _gather_logits(L, column, n_rows, index, m, out):
    import torch

    rc = L.skyjo_vec_rollout_gather_logits(_vp(column), n_rows, _vp(index), m, _vp(out), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.skyjo_vec_last_error()
    torch.cuda.synchronize()


def _gather_logits_ref(col_pool, n_rows, index):
    """A row id outside [0, n_rows) gives zeros; row r of the column is pool row r % POOL."""
    ok = (index >= 0) & (index < n_rows)
    return np.where(ok[:, None], col_pool[np.where(ok, index, 0) % POOL], np.float32(0.0)).astype(np.float32)


def test_gather_logits_from_a_column_past_4_gib():
    """skyjo_vec_rollout_gather_logits, m = 600 rows out of a column of 41.3 M rows x 104 bytes: ids in every window - either side of byte
    2^32 and the last rows - and the out-of-range ids of tests/learner_synth.py (2^31, 2^32, +-2^63)."""
    import torch

    from skyjo_rl_amd import _lib

    L = _lib.load()
    n, wins = _marks("gather-logits-column")
    rng = np.random.default_rng(811)
    col_pool = rng.standard_normal((POOL, 26)).astype(np.float32)
    column = _filled(n, col_pool)
    bad = np.array([-1, n, 2 ** 63 - 1, -2 ** 63, n + 1, -n, 2 ** 32, -2 ** 32 + 5, 2 ** 31, 2 ** 31 + 7], dtype=np.int64)
    rows = br.window_rows(wins)
    mark = 2 ** 32 // 104
    index = np.concatenate([rng.choice(rows, size=586, replace=True), [0, n - 1, mark - 1, mark], bad])
    index = index[rng.permutation(index.size)].astype(np.int64)
    assert index.size == 600 and ((index >= 0) & (index < n) & (index * 104 >= 2 ** 32)).sum() > 50
    out = _guarded((600, 26), torch.float32)
    _gather_logits(L, column, n, _dev(index), 600, out[1])
    _intact(out)
    got, want = out[1].cpu().numpy(), _gather_logits_ref(col_pool, n, index)
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), np.flatnonzero((got != want).any(1))[:8]


def test_gather_logits_into_an_output_past_4_gib():
    """The same call with m as large as the column (index int64 [m], periodic; out crosses byte 2^32): first period against the
    definition, the whole output against that period."""
    import torch

    from skyjo_rl_amd import _lib

    L = _lib.load()
    n, _ = _marks("gather-logits-index")
    rng = np.random.default_rng(812)
    col_pool = rng.standard_normal((POOL, 26)).astype(np.float32)
    idx_pool = rng.integers(0, n, size=POOL, dtype=np.int64)
    idx_pool[:6] = [0, n - 1, 2 ** 32 // 104 - 1, 2 ** 32 // 104, -1, n]
    idx_pool[6:606] = rng.integers(2 ** 32 // 104, n, size=600)                          # (the last 4099 rows lie past byte 2^32)
    assert ((idx_pool < n) & (idx_pool * 104 >= 2 ** 32)).sum() > 600
    column, index = _filled(n, col_pool), _filled(n, idx_pool[:, None]).view(n)
    out = _guarded((n, 26), torch.float32)
    _gather_logits(L, column, n, index, n, out[1])
    _intact(out)
    got, want = out[1][:POOL].cpu().numpy(), _gather_logits_ref(col_pool, n, idx_pool)
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), np.flatnonzero((got != want).any(1))[:8]
    _periodic("out", out[1])


# ---------------------------------------------------------------- 9. the loss head
def _scaled_stats(m, whole, part):
    """Means over m periodic rows from the pool's means: m = q POOL + rem rows are q copies of the pool and its first rem rows."""
    q, rem = divmod(m, POOL)
    return (q * POOL * whole + rem * part) / m


def _head_columns(b, m):
    names = ("logits", "log_mask", "value", "actions", "logp", "advantages", "value_targets", "values")
    return {k: _filled(m, getattr(b, k).reshape(POOL, -1)) for k in names}


def _check_head(name, m, stats, gl, gv, want_pool, want_part, T, nstats, clipped_pool):
    scale = POOL / m                                          # the gradients carry 1 / m
    got_l, got_v = gl[:POOL].cpu().numpy().astype(np.float64), gv[:POOL].cpu().numpy().astype(np.float64)
    dl, dv = np.abs(got_l - want_pool["grad_logits"] * scale).max(), np.abs(got_v - want_pool["grad_value"] * scale).max()
    want_stats = _scaled_stats(m, want_pool["stats"], want_part["stats"])
    ds = np.abs(stats - want_stats)
    print("%s m=%d: grad_logits %.3e (x m %.3e) grad_value %.3e (x m %.3e) stats %s" % (name, m, dl, dl * m, dv, dv * m, " ".join("%.3e" % x for x in ds)))
    assert dl <= MARGIN * min(T["grad_logits"], T["grad_logits_times_m"] / m)
    assert dv <= MARGIN * min(T["grad_value"], T["grad_value_times_m"] / m)
    for k in range(nstats):
        key = (ppo_loss_synth.ref.STATS + ("action_kl",))[k]
        assert ds[k] <= MARGIN * T[key], (key, ds[k])
    count = int((br.repeat_counts(m) * clipped_pool).sum())
    assert stats[5] == count / m, (stats[5] * m, count)       # the clipped rows, counted exactly
    _periodic("grad_logits", gl)
    _periodic("grad_value", gv.view(m, 1))


def test_ppo_loss_past_4_gib():
    """skyjo_vec_ppo_loss on 41.3 M rows: logits, log-mask and the logit gradients cross byte 2^32.  Gradients: first period against
    ``ppo_loss_ref`` (scaled by POOL / m), then the whole against that period.  Statistics: the pool's, weighted by the exact repeat
    counts, at the bounds of tests/test_gpu_ppo_loss.py - which hold per row, and a mean over more rows is a mean of the same rows."""
    import torch

    from skyjo_rl_amd import _lib

    L = _lib.load()
    m, _ = _marks("ppo-loss")
    ent_coef, vf_clip = 0.01, ppo_loss_synth.VF_CLIP
    b = ppo_loss_synth.make(POOL)
    part = ppo_loss_synth.Batch(*[x[:m % POOL] if isinstance(x, np.ndarray) else x for x in b])
    want_pool, want_part = ppo_loss_synth.reference(b, ent_coef, vf_clip), ppo_loss_synth.reference(part, ent_coef, vf_clip)
    c = _head_columns(b, m)
    nbytes = int(L.skyjo_vec_ppo_loss_scratch_bytes(m))
    gl, gv, st, sc = _guarded((m, 26), torch.float32), _guarded((m,), torch.float32), _guarded((6,), torch.float64), _guarded((nbytes,), torch.uint8)
    rc = L.skyjo_vec_ppo_loss(_vp(c["logits"]), _vp(c["log_mask"]), _vp(c["value"]), _vp(c["actions"]), _vp(c["logp"]), _vp(c["advantages"]),
                              _vp(c["value_targets"]), _vp(c["values"]), m, ppo_loss_synth.CLIP, 1.0, ent_coef, vf_clip, _vp(gl[1]), _vp(gv[1]), _vp(st[1]),
                              _vp(sc[1]), nbytes, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.skyjo_vec_last_error()
    torch.cuda.synchronize()
    _intact(gl, gv, st, sc)
    _check_head("ppo_loss", m, st[1].cpu().numpy(), gl[1], gv[1], want_pool, want_part, F32_DEVIATION, 6, want_pool["clipped"])


def test_ppo_loss_kl_past_2_gib():
    """skyjo_vec_ppo_loss_kl at the byte-2^31 crossing of its four [m][26] arrays (20.65 M rows; the cap leaves no room for 2^32)."""
    import torch

    from skyjo_rl_amd import _lib

    L = _lib.load()
    m, _ = _marks("ppo-loss-kl")
    ent_coef, vf_clip, kl_coeff = 0.01, ppo_loss_synth.VF_CLIP, 0.2
    b = ppo_loss_kl_synth.make(POOL)
    part = ppo_loss_kl_synth.KLBatch(*[x[:m % POOL] if isinstance(x, np.ndarray) else x for x in b])
    want_pool, want_part = ppo_loss_kl_synth.reference(b, ent_coef, vf_clip, kl_coeff), ppo_loss_kl_synth.reference(part, ent_coef, vf_clip, kl_coeff)
    c = _head_columns(b, m)
    old = _filled(m, b.old_logits)
    nbytes = int(L.skyjo_vec_ppo_loss_kl_scratch_bytes(m))
    gl, gv, st, sc = _guarded((m, 26), torch.float32), _guarded((m,), torch.float32), _guarded((7,), torch.float64), _guarded((nbytes,), torch.uint8)
    rc = L.skyjo_vec_ppo_loss_kl(_vp(c["logits"]), _vp(c["log_mask"]), _vp(old), _vp(c["value"]), _vp(c["actions"]), _vp(c["logp"]), _vp(c["advantages"]),
                                 _vp(c["value_targets"]), _vp(c["values"]), m, ppo_loss_synth.CLIP, 1.0, ent_coef, vf_clip, kl_coeff, _vp(gl[1]), _vp(gv[1]),
                                 _vp(st[1]), _vp(sc[1]), nbytes, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.skyjo_vec_last_error()
    torch.cuda.synchronize()
    _intact(gl, gv, st, sc)
    _check_head("ppo_loss_kl", m, st[1].cpu().numpy(), gl[1], gv[1], want_pool, want_part, F32_DEVIATION_KL, 7, want_pool["clipped"])


# ---------------------------------------------------------------- 10. episode statistics
def test_episode_stats_past_4_gib():
    """skyjo_vec_episode_stats, four seats, 134 M rows: final_rewards (32 bytes a row) crosses byte 2^32.  Episodes end inside the windows
    only; the rewards are multiples of 1 / 8 below 2^10, so every partial sum is exact in double and the comparison is ==."""
    import torch

    from skyjo_rl_amd import _lib

    L = _lib.load()
    N = 4
    rows, wins = _marks("episode-stats")
    rng = np.random.default_rng(1010)
    fr_pool = rng.integers(-8000, 8001, size=(POOL, N)).astype(np.float64) / 8.0
    fr_pool[::3, 0] = fr_pool[::3].max(axis=1)               # ties of two seats, and of all seats
    fr_pool[1::5] = fr_pool[1::5, :1]
    fr = _filled(rows, fr_pool)
    ee = torch.zeros((rows,), dtype=torch.uint8, device="cuda:0")
    ends = np.zeros(0, dtype=np.int64)
    for lo, hi in wins:
        e = (rng.random(hi - lo) < 0.5).astype(np.uint8) * rng.integers(1, 256, size=hi - lo).astype(np.uint8)
        e[0], e[-1] = 1, 0x80
        ee[lo:hi] = _dev(e)
        ends = np.concatenate([ends, lo + np.flatnonzero(e)])
    assert (ends * 32 >= 2 ** 32).any() and (ends * 32 < 2 ** 32).any()
    need = int(L.skyjo_vec_episode_stats_scratch_bytes(rows, N))
    out, scratch = _guarded((1 + 3 * N,), torch.float64), _guarded((need,), torch.uint8)
    _lib.check(L.skyjo_vec_episode_stats(_vp(fr), _vp(ee), rows, N, _vp(out[1]), _vp(scratch[1]), need, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    _intact(out, scratch)
    got = out[1].cpu().numpy()
    count, sums, squares, wins_ = arena_ref.episode_sums(fr_pool[ends % POOL], np.ones(ends.size, dtype=np.uint8))
    assert count == ends.size and got[0] == float(count)
    for s in range(N):
        assert (got[1 + 3 * s], got[2 + 3 * s], got[3 + 3 * s]) == (sums[s], squares[s], float(wins_[s])), s


# ---------------------------------------------------------------- 4. both branches with the draw
@pytest.mark.parametrize("precision,planar", [("fp32", False), ("bf16", True)], ids=["rows-fp32", "planar-bf16"])
def test_act_value_past_4_gib(precision, planar):
    """skyjo_vec_mlp_act_value_layout on 2^26 + 4099 records, policy and value branch with the draw in the launch's epilogue.  Logits and
    values: ``check_forward`` on the first period, then the whole against it.  Actions and log-probabilities: ``check_draw`` in the
    windows, on the logits the launch wrote there (just checked) and the uniforms of the rows' own ids, as
    tests/test_gpu_net_synthetic.py compares a draw made in the net's launch; everywhere: written, and in 0 .. 25."""
    import torch

    from skyjo_rl_amd import SkyjoVecEnv, _lib

    L = _lib.load()
    n, wins = _marks("act-value-planar-bf16" if planar else "act-value-rows-fp32")
    seed, ticket = SEED_TICKET[2]
    pc, vc = net_ref.forward_case((31, 26), "A"), net_ref.forward_case((31, 1), "A")
    assert np.array_equal(pc["pool"], vc["pool"])
    pol, val = _net(pc["params"], precision, key=((31, 26), "A")), _net(vc["params"], precision, key=((31, 1), "A"))
    pool = np.array(pc["pool"])
    env = SkyjoVecEnv(64, game_id0=HIGH_ID0)
    try:
        assert (env.mask_offset, env.record_bytes) == (32, 64)
        rec = _filled_planar(n, pool) if planar else _filled(n, pool)
        lg, v = _guarded((n, 26), torch.float32), _guarded((n, 1), torch.float32)
        a, lp = _guarded((n,), torch.int32), _guarded((n,), torch.float32)
        rc = L.skyjo_vec_mlp_act_value_layout(env._h, pol._h, val._h, _vp(rec), _lib.REC_TILE_PLANAR if planar else _lib.REC_ROW_MAJOR, n, seed, ticket, 0,
                                              _vp(a[1]), _vp(lp[1]), _vp(lg[1]), _vp(v[1]), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, L.skyjo_vec_last_error()
        torch.cuda.synchronize()
        _intact(lg, v, a, lp)
        assert net_ref.check_forward(lg[1][:POOL].cpu().numpy(), pc, precision) == []
        assert net_ref.check_forward(v[1][:POOL].cpu().numpy(), vc, precision) == []
        _periodic("logits", lg[1])
        _periodic("values", v[1])
        for name, t in (("actions", a[1]), ("logp", lp[1])):
            assert br.window_mismatches(t.view(torch.int32), [], None, sentinel=FILL32)[1] == 0, name + " has elements the kernel did not write"
        assert int(a[1].min()) >= 0 and int(a[1].max()) <= 25
        rows = br.window_rows(wins)
        idx = _dev(rows)
        with np.errstate(over="ignore"):
            gid = np.uint64(HIGH_ID0) + rows.astype(np.uint64)
        u = net_ref.uniform(seed, ticket, gid)
        mask = pool[rows % POOL, 32:58]
        logits = lg[1][idx].cpu().numpy()
        sub = dict(n=rows.size, seed=seed, ticket=ticket, game_id0=HIGH_ID0, no_masking=False, mask=mask, mask_family=np.full(rows.size, 8), logits=logits,
                   logit_family=np.full(rows.size, -1), u=u, ref=net_ref.draw_reference(logits, mask, u, False))
        assert net_ref.check_draw(a[1][idx].cpu().numpy(), lp[1][idx].cpu().numpy(), None, sub) == []
    finally:
        env.close()


# ---------------------------------------------------------------- 6 / 7. a buffer whose rows cross byte 2^32
def _window_buffer(planar, steps):
    """``steps`` steps of WINDOW_B indirect three-player records on the device in either layout, slot s (row-major: s = t B + b;
    tile-planar: s = t tiles 64 + b, the padding slots of the last tile included) holding pool row s % POOL; the pool; the slot of a row."""
    B = br.WINDOW_B
    g = learner_synth.geometry(3, True)
    pool = learner_synth.records(1, POOL, g, np.random.default_rng(707))[0]
    stride = (B + 63) // 64 * 64 if planar else B
    rec = _filled_planar(steps * stride, pool) if planar else _filled(steps * stride, pool)
    return g, pool, rec, (lambda r: (r // B) * stride + r % B)


@pytest.mark.parametrize("planar", [False, True], ids=["rows", "planar"])
def test_select_seats_over_records_past_4_gib(planar):
    """skyjo_vec_rollout_select_seats over T x B = 4 090 x 16 411 rows whose records cross byte 2^32: the agent byte of a row far out is
    read where the row's record lies.  Islands of flags in the windows, one seat in the mask."""
    import torch

    from skyjo_rl_amd import SkyjoVecEnv, _lib

    L = _lib.load()
    n, wins = _marks("select-seats")
    B, T = br.WINDOW_B, br.WINDOW_T
    assert n == T * B and B % 64 and B % POOL and (T - 1) * B < 2 ** 26 + POOL <= n
    rng = np.random.default_rng(632)
    flag_pool = (rng.integers(0, 256, size=POOL, dtype=np.uint8) & 0xFC)[:, None]
    adv_pool = (rng.standard_normal(POOL).astype(np.float32) * np.float32(25.0))[:, None]
    env = SkyjoVecEnv(B, num_players=3, observe_other_player_indirect=True)
    try:
        g, pool, rec, slot = _window_buffer(planar, T)
        flags, adv = _filled(n, flag_pool).view(n), _filled(n, adv_pool).view(n)
        islands = {}
        for lo, hi in wins:
            islands[lo] = rng.integers(0, 256, size=hi - lo, dtype=np.uint8) | 1
            flags[lo:hi] = _dev(islands[lo])
        room = sum(hi - lo for lo, hi in wins)
        seat = 1
        parts = []
        for lo, hi in wins:
            r = np.arange(lo, hi, dtype=np.int64)
            agent = pool[slot(r) % POOL, g["mask_offset"] + 26]
            parts.append(r[((islands[lo] & 3) == 3) & (agent == seat)])
        want = np.concatenate(parts)
        assert 50 < want.size < room and (want * 64 >= 2 ** 32).any()
        index, out = _guarded((room,), torch.int64), _guarded((3,), torch.int64)
        rc = L.skyjo_vec_rollout_select_seats(env._h, _vp(rec), _lib.REC_TILE_PLANAR if planar else _lib.REC_ROW_MAJOR, T, _vp(flags), 3, 1 << seat, _vp(adv),
                                              _vp(index[1]), _vp(out[1]), _vp(out[1][1:]), env._stream())
        assert rc == 0, L.skyjo_vec_last_error()
        torch.cuda.synchronize()
        _intact(index, out)
        count = int(out[1][0])
        got = index[1].cpu().numpy()
        assert count == want.size and np.array_equal(got[:count], want) and (got[count:] == FILL64).all()
        mom = out[1][1:3].view(torch.float64).cpu().numpy()
        x = adv_pool[want % POOL, 0].astype(np.float64)
        for got_sum, ref_sum, mag in ((mom[0], x.sum(), np.abs(x).sum()), (mom[1], (x * x).sum(), (x * x).sum())):
            assert abs(got_sum - ref_sum) <= 2 * count * 2.0 ** -53 * mag
    finally:
        env.close()


GATHER_NAMES = ("observations", "log_mask", "actions", "logp", "advantages", "value_targets", "values", "seats")


def _gather_outputs(m, D):
    import torch

    dtypes = (torch.float32, torch.float32, torch.int64, torch.float32, torch.float32, torch.float32, torch.float32, torch.uint8)
    shapes = ((m, D), (m, 26)) + ((m,),) * 6
    return {k: _guarded(s, dt) for k, s, dt in zip(GATHER_NAMES, shapes, dtypes)}


def _same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def _column_pools(rng):
    return dict(actions=rng.integers(-2 ** 31, 2 ** 31, size=POOL).astype(np.int32), logp=-rng.random(POOL, dtype=np.float32),
                values=(rng.standard_normal(POOL) * 30).astype(np.float32), advantages=(rng.standard_normal(POOL) * 9).astype(np.float32),
                value_targets=rng.standard_normal(POOL, dtype=np.float32))


@pytest.mark.parametrize("planar", [False, True], ids=["rows", "planar"])
def test_gather_out_of_a_buffer_past_4_gib(planar):
    """skyjo_vec_rollout_gather, m = 600 row ids in every window of a buffer of 4 090 x 16 411 rows (records past byte 2^32), with the
    out-of-range ids of tests/learner_synth.py.  ``rollout_batches_ref.gather`` on the records and column values those rows hold."""
    import torch

    from skyjo_rl_amd import SkyjoVecEnv, _lib

    L = _lib.load()
    n, wins = _marks("gather-window")
    B, T = br.WINDOW_B, br.WINDOW_T
    rng = np.random.default_rng(711)
    env = SkyjoVecEnv(B, num_players=3, observe_other_player_indirect=True)
    try:
        g, pool, rec, slot = _window_buffer(planar, T + 1)
        D, rb = g["obs_dim"], g["record_bytes"]
        pools = _column_pools(rng)
        cols = {k: _filled((T + 1) * B if k == "values" else n, v[:, None]) for k, v in pools.items()}
        bad = np.array([-1, n, 2 ** 63 - 1, -2 ** 63, n + 1, -n, 2 ** 32, -2 ** 32 + 5, 2 ** 31, (T + 1) * B - 1], dtype=np.int64)
        index = np.concatenate([rng.choice(br.window_rows(wins), size=586), [0, n - 1, 2 ** 26 - 1, 2 ** 26], bad])
        index = index[rng.permutation(index.size)].astype(np.int64)
        m = index.size
        ok = (index >= 0) & (index < n)
        assert m == 600 and (ok & (index * rb >= 2 ** 32)).sum() > 50
        r = np.where(ok, index, 0)
        want = bref.gather(pool[slot(r) % POOL], False, rb, D, m, 1, m, np.where(ok, np.arange(m), -1), mean=0.1, std=0.7,
                           **{k: v[r % POOL] for k, v in pools.items()})
        outs = _gather_outputs(m, D)
        rc = L.skyjo_vec_rollout_gather(env._h, _vp(rec), _lib.REC_TILE_PLANAR if planar else _lib.REC_ROW_MAJOR, T, _vp(_dev(index)), m, _vp(cols["actions"]),
                                        _vp(cols["logp"]), _vp(cols["values"]), 1, _vp(cols["advantages"]), _vp(cols["value_targets"]), 0.1, 0.7,
                                        *[_vp(outs[k][1]) for k in GATHER_NAMES], env._stream())
        assert rc == 0, L.skyjo_vec_last_error()
        torch.cuda.synchronize()
        _intact(*outs.values())
        for k in GATHER_NAMES:
            assert _same_bits(outs[k][1].cpu().numpy(), want[k]), k
    finally:
        env.close()


@pytest.mark.parametrize("planar", [False, True], ids=["rows", "planar"])
def test_gather_into_outputs_past_4_gib(planar):
    """skyjo_vec_rollout_gather with m = 34.6 M: obs_out crosses byte 2^32, lm_out byte 2^31.  The index is periodic into a buffer of one
    step of 4099 games: first period against ``rollout_batches_ref.gather``, every output whole against its first period."""
    import torch

    from skyjo_rl_amd import SkyjoVecEnv, _lib

    L = _lib.load()
    m, _ = _marks("gather-index")
    B, T = POOL, 1
    rng = np.random.default_rng(712)
    g = learner_synth.geometry(3, True)
    D, rb = g["obs_dim"], g["record_bytes"]
    rec_np = learner_synth.records(T + 1, B, g, rng)
    planar_np = learner_synth.to_planar_dirty(rec_np, rng)
    pools = _column_pools(rng)
    pools["values"] = (rng.standard_normal((T + 1) * B) * 30).astype(np.float32)
    idx_pool = rng.permutation(B).astype(np.int64)
    idx_pool[:8] = [-1, B, 2 ** 63 - 1, -2 ** 63, 2 ** 32, 2 ** 31, 0, B - 1]
    stride = planar_np.shape[1] * 64 if planar else B
    want = bref.gather(planar_np if planar else rec_np, planar, rb, D, B, T, stride, idx_pool, mean=0.1, std=0.7, **pools)
    env = SkyjoVecEnv(B, num_players=3, observe_other_player_indirect=True)
    try:
        rec = _dev(planar_np if planar else rec_np)
        cols = {k: _dev(v) for k, v in pools.items()}
        index = _filled(m, idx_pool[:, None]).view(m)
        outs = _gather_outputs(m, D)
        rc = L.skyjo_vec_rollout_gather(env._h, _vp(rec), _lib.REC_TILE_PLANAR if planar else _lib.REC_ROW_MAJOR, T, _vp(index), m, _vp(cols["actions"]),
                                        _vp(cols["logp"]), _vp(cols["values"]), 1, _vp(cols["advantages"]), _vp(cols["value_targets"]), 0.1, 0.7,
                                        *[_vp(outs[k][1]) for k in GATHER_NAMES], env._stream())
        assert rc == 0, L.skyjo_vec_last_error()
        torch.cuda.synchronize()
        _intact(*outs.values())
        for k in GATHER_NAMES:
            assert _same_bits(outs[k][1][:POOL].cpu().numpy(), want[k]), k
            _periodic(k, outs[k][1])
    finally:
        env.close()


# ---------------------------------------------------------------- 5. learner targets
@pytest.mark.parametrize("planar", [False, True], ids=["rows", "planar"])
def test_rollout_targets_over_records_past_4_gib(planar):
    """skyjo_vec_rollout_targets, 65 536 four-player games, T = 1 025: the (T + 1) B records cross byte 2^32 at the turn from game 65 535
    of step 1 023 to game 0 of step 1 024.  The first and the last 512 games carry the columns of tests/learner_synth.py (every byte of
    their records random, ends, invalid rows); all other games are of two classes (game parity) of two-step episodes with values and
    rewards that change from step to step.  Window games bit for bit ``targets_f32``, and within the textbook bound of
    tests/test_gpu_learner_synthetic.py of ``targets_f64``; every other game, on the device, bit for bit its class's column."""
    import torch

    from skyjo_rl_amd import SkyjoVecEnv, _lib
    from tests import rollout_targets_ref as tref

    L = _lib.load()
    B, T, N, W = br.TARGETS_B, br.TARGETS_T, 4, br.WIDTH
    assert br.CASES["targets"]["n"] == (T + 1) * B and (T - 1) * B * 64 == 2 ** 32          # byte 2^32: game 0 of the last acting step
    g = learner_synth.geometry(N, True)
    off_agent, off_done, rb = g["mask_offset"] + 26, g["mask_offset"] + 28, g["record_bytes"]
    rng = np.random.default_rng(505)
    wg = np.concatenate([np.arange(W), np.arange(B - W, B)])
    wrec = learner_synth.records(T + 1, 2 * W, g, rng)
    agent, done = learner_synth.meta(wrec, g)
    cols, _ = learner_synth.target_columns(T, 2 * W, N, rng, done=done)
    steps = np.arange(T + 1)
    prec = rng.integers(0, 256, size=(T + 1, 2, rb), dtype=np.uint8)
    for c in (0, 1):
        prec[:, c, off_agent], prec[:, c, off_done] = (steps + c) % 2, 0
    pend = np.zeros((T, 2), dtype=np.uint8)
    pend[1::2] = 1
    prew = rng.standard_normal((T, 2, N)) * 4.0 + rng.random((T, 2, N)) * 2.0 ** -30
    pval = rng.standard_normal((T + 1, 2)).astype(np.float32)
    pagent, pdone = learner_synth.meta(prec, g)
    both = dict(agent=np.concatenate([agent, pagent], 1), done=np.concatenate([done, pdone], 1), episode_end=np.concatenate([cols["episode_end"], pend], 1),
                values=np.concatenate([cols["values"], pval], 1), final_rewards=np.concatenate([cols["final_rewards"], prew], 1))
    gamma, lam = 0.99, 0.95
    want = tref.targets_f32(gamma=gamma, lam=lam, **both)
    assert (want[3][:, 2 * W:] & 1).sum() > T and (want[3][:, :2 * W] & 1).sum() > T * W

    env = SkyjoVecEnv(B, num_players=N, observe_other_player_indirect=True)
    try:
        assert env.record_bytes == rb and env.mask_offset == g["mask_offset"]
        dev = "cuda:0"
        cls, wg_d = torch.arange(B, device=dev) % 2, _dev(wg)
        tiles, k = B // 64, 8
        rec = torch.empty((T + 1, tiles, rb // 16, 64, 16) if planar else (T + 1, B, rb), dtype=torch.uint8, device=dev)
        prec_d = _dev(prec)
        for t0 in range(0, T + 1, k):                         # 8 steps, 32 MiB, at a time
            chunk = prec_d[t0:t0 + k].index_select(1, cls)
            chunk[:, wg_d] = _dev(wrec[t0:t0 + k])
            rec[t0:t0 + k] = chunk.view(-1, tiles, 64, rb // 16, 16).permute(0, 1, 3, 2, 4) if planar else chunk
        values = _dev(pval).index_select(1, cls)
        values[:, wg_d] = _dev(cols["values"])
        rewards = _dev(prew).index_select(1, cls)
        rewards[:, wg_d] = _dev(cols["final_rewards"])
        end = _dev(pend).index_select(1, cls)
        end[:, wg_d] = _dev(cols["episode_end"])
        outs = [_guarded((T, B), torch.float32) for _ in range(3)] + [_guarded((T, B), torch.uint8)]
        rc = L.skyjo_vec_rollout_targets(env._h, _vp(rec), _lib.REC_TILE_PLANAR if planar else _lib.REC_ROW_MAJOR, T, _vp(values), 1, _vp(rewards), _vp(end),
                                         gamma, lam, *[_vp(o[1]) for o in outs], env._stream())
        assert rc == 0, L.skyjo_vec_last_error()
        torch.cuda.synchronize()
        _intact(*outs)
        names = ("advantages", "value_targets", "returns", "flags")
        got = [o[1][:, wg_d].cpu().numpy() for o in outs]
        for name, x, w in zip(names, got, want):
            assert _same_bits(x, w[:, :2 * W]), name
        mid = cls[W:B - W]
        for name, o, w in zip(names, outs, want):
            w_d = _dev(w[:, 2 * W:])
            for t0 in range(0, T, 64):
                exp = w_d[t0:t0 + 64].index_select(1, mid)
                x = o[1][t0:t0 + 64, W:B - W]
                same = torch.equal(x.view(torch.int32), exp.view(torch.int32)) if x.dtype == torch.float32 else torch.equal(x, exp)
                assert same, (name, t0)
        few = slice(0, 64)                                    # the textbook recursion is a Python loop: the first 64 window games
        sub = {k_: v[:, few] for k_, v in both.items()}
        adv64, tgt64, has64, info = tref.targets_f64(gamma=gamma, lam=lam, **sub)
        M = max(float(np.abs(sub["values"]).max()), float(np.abs(sub["final_rewards"]).max()))
        bound = 4 * info["longest"] * 2.0 ** -24 * M
        err = max(float(np.abs(got[0][:, few] - adv64).max()), float(np.abs(got[1][:, few] - tgt64).max()))
        print("textbook: L=%d M=%.4f bound=%.3e max error=%.3e" % (info["longest"], M, bound, err))
        assert np.array_equal((got[3][:, few] & 1) != 0, has64) and int(has64.sum()) > 0 and err <= bound
    finally:
        env.close()


# ---------------------------------------------------------------- 11. the collection loop
@pytest.mark.parametrize("layout", ["row-major", "tile-planar-all"])
def test_collect_into_a_buffer_past_4_gib(layout):
    """``rollout.collect`` (skyjo_vec_model_rollout), 65 536 four-player games, T = 1 024: the records buffer crosses byte 2^32.  A second
    engine with the same seeds collects the same iterations as eight calls of 128 into a small buffer (first_ticket, first_records);
    every column of every slice equals the big buffer's slice byte for byte."""
    import torch

    from skyjo_rl_amd import SkyjoVecEnv
    from skyjo_rl_amd.action_mask_model import ActionMaskModel, FusedNet
    from skyjo_rl_amd.rollout import RolloutBuffer, collect

    B, T, S, N = br.COLLECT_B, br.COLLECT_T, br.COLLECT_SLICE, 4
    assert br.CASES["collect"]["n"] == (T + 1) * B and T % S == 0
    torch.manual_seed(3)
    model = ActionMaskModel(obs_dim=31).cuda()
    pol, val = FusedNet(model.policy, precision="bf16"), FusedNet(model.value, precision="bf16")
    envs = []
    try:
        for _ in range(2):
            env = SkyjoVecEnv(B, num_players=N, auto_reset=True)
            env.set_record_layout(layout)
            assert env.record_layout == layout and env.record_bytes == 64
            env.seed(None, 21)
            envs.append(env)
        big, small = RolloutBuffer(envs[0], T), RolloutBuffer(envs[1], S)
        guarded = _guarded(tuple(big.records.shape), torch.uint8)
        big.records = guarded[1]
        assert big.records.numel() > 2 ** 32
        collect(envs[0], pol, val, big, seed=6, first_ticket=0)
        torch.cuda.synchronize()
        _intact(guarded)
        ends = 0
        for k in range(T // S):
            first = None if k == 0 else small.records[S].clone()
            collect(envs[1], pol, val, small, seed=6, first_ticket=k * S, first_records=first)
            lo, hi = k * S, (k + 1) * S
            assert torch.equal(big.records[lo:hi + 1], small.records), ("records", k)
            assert torch.equal(big.actions[lo:hi], small.actions), ("actions", k)
            assert torch.equal(big.logp[lo:hi].view(torch.int32), small.logp.view(torch.int32)), ("logp", k)
            assert torch.equal(big.values[lo:hi + 1].view(torch.int32), small.values.view(torch.int32)), ("values", k)
            assert torch.equal(big.final_rewards[lo:hi].view(torch.int64), small.final_rewards.view(torch.int64)), ("final_rewards", k)
            assert torch.equal(big.episode_end[lo:hi], small.episode_end), ("episode_end", k)
            ends += int(small.episode_end.sum())
        assert ends > B                                       # (several episodes per game)
        for env in envs:
            env.check_error()
    finally:
        for env in envs:
            env.close()
        pol.close()
        val.close()
