"""Packed nets on the direct observation - 32 to 163 inputs: the packer and the Adam step behind it (``k_mlp_update``, csrc/skyjo_update.h),
the wide net kernels (``k_net_bf16_wide`` / ``k_net_split_wide``, csrc/skyjo_policy.hip) on the synthetic records of
tests/net_wide_ref.py, the pair draw behind them, and the engine's rollout forms with such nets.  The forward sweep runs every width of
net_wide_ref.SWEEP_OBS - every (MKS, KS) pair of the two instantiations, so every number of padding k-steps -; the pair draw every player
count 1 .. 12; the rollouts 1 .. 5, 8, 11 and 12 players direct and 5 and 12 indirect (tests/test_gpu_net_wide_rollouts.py: episode ends).

Bounds (tests/net_ref.py: check_forward): float32-grade max |kernel - Q| <= M_FP32 x F, F the float32 torch module's own deviation from X
on the case; bf16: the project's emulation bound against Q.  The project's 1e-4 / 8e-2 against X were measured at 31 inputs and are not
asserted here; every case prints max |kernel - X| (EXPERIMENTS, wide nets, has the MI355X run's figures)."""
import numpy as np
import pytest

from tests import mlp_pack_ref as pk, mlp_pack_wide_ref as wide, net_ref as ref, net_wide_ref as wref

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0DEAD
GUARD_ROWS = 4
PRECISIONS = ("fp32", "bf16")
ONE_NET_PASSES_ROWS = 65537       # the smallest counts at which sk_launch_mlp takes passes > 1: one net, two nets
TWO_NET_PASSES_ROWS = 32769
RATIOS = {}


def launch_geometry(n, nets):
    """(passes, workgroups per net) as sk_launch_mlp states them."""
    batches = (n + 255) // 256
    passes = min(8, max(1, (batches * nets + 255) // 256))
    return passes, (batches + passes - 1) // passes


def test_row_counts_reach_the_launch_geometries_they_claim():
    assert launch_geometry(ONE_NET_PASSES_ROWS - 1, 1) == (1, 256) and launch_geometry(ONE_NET_PASSES_ROWS, 1) == (2, 129)
    assert launch_geometry(TWO_NET_PASSES_ROWS - 1, 2) == (1, 128) and launch_geometry(TWO_NET_PASSES_ROWS, 2) == (2, 65)
    assert [launch_geometry(n, 1) for n in (1, 33, 257)] == [(1, 1), (1, 1), (1, 2)]          # one lane, two wavefronts, two blocks


def _guarded(rows, cols, dtype):
    import torch

    whole = torch.empty((rows + 2 * GUARD_ROWS, cols) if cols else (rows + 2 * GUARD_ROWS,), dtype=dtype, device="cuda:0")
    whole.view(torch.int32).fill_(SENTINEL)
    return whole, whole[GUARD_ROWS:GUARD_ROWS + rows]


def _intact(*bufs):
    import torch

    for whole, view in bufs:
        w = whole.view(torch.int32)
        assert bool((w[:GUARD_ROWS] == SENTINEL).all()) and bool((w[GUARD_ROWS + view.shape[0]:] == SENTINEL).all()), "a guard row was written"


def _seq(params):
    import torch
    from torch import nn

    obs_dim, out_dim = params[0].shape[1], params[4].shape[0]
    seq = nn.Sequential(nn.Linear(obs_dim, 256), nn.Tanh(), nn.Linear(256, 256), nn.Tanh(), nn.Linear(256, out_dim))
    with torch.no_grad():
        for p, w in zip(seq.parameters(), params):
            p.copy_(torch.from_numpy(np.array(w)))
    return seq.cuda()


_NETS = {}


def _net(params, precision, key):
    from skyjo_rl_amd.action_mask_model import FusedNet

    if (key, precision) not in _NETS:
        _NETS[(key, precision)] = FusedNet(_seq(params), precision=precision)
    return _NETS[(key, precision)]


def _case_net(case, precision):
    return _net(case["params"], precision, (case["shape"], case["wset"]))


def _same(a, b):
    import torch

    return a.shape == b.shape and torch.equal(a, b)


# ---------------------------------------------------------------- pack and update
# one width per KS 3 .. 11 beside the edges of WIDE_OBS: k_mlp_update's wide piece at every number of k-steps
UPDATE_SHAPES = wide.WIDE_SHAPES + tuple((d, 26 if k % 2 else 1) for k, d in sorted(wref.ONE_PER_KS.items()) if d not in wide.WIDE_OBS)


def test_update_shapes_hold_every_number_of_ksteps():
    assert {wide.ksteps(d) for d, _ in UPDATE_SHAPES} == set(range(3, 12)) and {o for _, o in UPDATE_SHAPES} == {1, 26}


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("shape", UPDATE_SHAPES, ids=lambda s: "%dx%d" % s)
def test_export_is_the_reference_bytes_and_update_a_fresh_pack(shape, precision):
    import torch
    from skyjo_rl_amd.action_mask_model import FusedNet

    A, B = wide.default_init(shape[0], shape[1], 0), pk.weights_b(*shape)
    seq_a, seq_b = _seq(A), _seq(B)
    net = FusedNet(seq_a, precision=precision)
    want = {"A": torch.from_numpy(wide.pack(*A, precision=precision)).cuda(), "B": torch.from_numpy(wide.pack(*B, precision=precision)).cuda()}
    assert _same(net.export(), want["A"])
    for name, seq in (("B", seq_b), ("A", seq_a)):              # (back and forth on ONE handle: a stale piece would show)
        net.update(seq)
        fresh = FusedNet(seq, precision=precision)
        got = net.export()
        assert _same(got, fresh.export()) and _same(got, want[name]), name
        fresh.close()
    net.close()


@pytest.mark.parametrize("out_dim", [26, 1])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_export_is_the_reference_bytes_at_every_wide_obs_dim(precision, out_dim):
    """Every obs_dim 32 .. 163 (132 nets in one test): the blob is tests/mlp_pack_wide_ref.py's, byte for byte."""
    import torch
    from skyjo_rl_amd.action_mask_model import FusedNet

    for obs_dim in range(32, wide.MAX_OBS + 1):
        params = pk.weights_b(obs_dim, out_dim)
        net = FusedNet(_seq(params), precision=precision)
        got = net.export().cpu()
        want = torch.from_numpy(wide.pack(*params, precision=precision))
        assert got.numel() == wide.packed_bytes(obs_dim, precision) and _same(got, want), (obs_dim, int((got != want).sum()) if got.shape == want.shape else got.shape)
        net.close()


@pytest.mark.parametrize("obs_dim", [0, 164])
def test_obs_dim_outside_1_to_163_is_refused(obs_dim):
    import warnings

    from skyjo_rl_amd import _lib
    from skyjo_rl_amd.action_mask_model import FusedNet

    rng = np.random.default_rng(0)
    params = [rng.standard_normal(s).astype(np.float32) for s in ((256, obs_dim), (256,), (256, 256), (256,), (26, 256), (26,))]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        seq = _seq(params)
    with pytest.raises(_lib.SkyjoNativeError, match="1..163"):
        FusedNet(seq)


def test_native_branch_keeps_its_limit_of_31_inputs():
    from skyjo_rl_amd.action_mask_model import ActionMaskModel
    from skyjo_rl_amd.learner import NativeBranch

    with pytest.raises(ValueError, match="1..31 inputs"):
        NativeBranch(ActionMaskModel(obs_dim=43).cuda().policy, 256)


@pytest.mark.parametrize("clipped", [False, True], ids=["plain", "clipped"])
@pytest.mark.parametrize("steps", [1, 3])
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("shape", [(67, 26), (163, 1)], ids=lambda s: "%dx%d" % s)
def test_native_adam_is_torch_adam_and_a_fresh_pack(shape, precision, steps, clipped):
    """The way tests/test_gpu_mlp_update.py holds narrow nets: after every step the blob is a fresh net's and the reference pack of the
    parameters as they then are; p, exp_avg and exp_avg_sq of the policy branch are no further from the float64 rule than 4 x
    torch.optim.Adam's own float32 distance (CPU, foreach=False).  Clipped: ``NativeAdam(max_grad_norm=)`` - the rule takes g times the
    coefficient on the device (one float32 multiply), which is torch's clipping coefficient of the twelve gradients' global norm."""
    import torch
    from skyjo_rl_amd.action_mask_model import ActionMaskModel, FusedNet
    from skyjo_rl_amd.learner import NativeAdam

    obs_dim, out_dim = shape
    max_norm = 0.5
    torch.manual_seed(0)
    model = ActionMaskModel(obs_dim=obs_dim, num_outputs=out_dim).cuda()
    nets = [FusedNet(model.policy, precision=precision), FusedNet(model.value, precision=precision)]
    opt = NativeAdam(model, nets[0], nets[1], max_grad_norm=max_norm if clipped else None, **pk.ADAM_HYPER)
    branches = [list(model.policy.parameters()), list(model.value.parameters())]
    start = [p.detach().cpu().numpy().copy() for p in branches[0]]
    used = []                                                   # per step: the policy branch's gradients as the rule took them
    for t in range(1, steps + 1):
        grads = [pk.adam_grads([tuple(p.shape) for p in params], t, seed=77 + b) for b, params in enumerate(branches)]
        for params, gs in zip(branches, grads):
            for p, g in zip(params, gs):
                p.grad = torch.from_numpy(g).cuda()
        opt.step()
        coef = np.float32(1.0)
        if clipped:
            norm, coef = (np.float32(x) for x in opt.grad_stats.cpu().numpy())
            want = float(np.sqrt(sum(float((g.astype(np.float64) ** 2).sum()) for gs in grads for g in gs)))
            assert abs(float(norm) - want) <= 1e-5 * want and want > max_norm
            assert abs(float(coef) - max_norm / (want + 1e-6)) <= 1e-5 * float(coef) and coef < 1
        used.append([(g * coef).astype(np.float32) for g in grads[0]])
        for b, seq in enumerate((model.policy, model.value)):
            fresh = FusedNet(seq, precision=precision)
            assert _same(nets[b].export(), fresh.export()), (t, b)
            fresh.close()
            want = wide.pack(*[p.detach().cpu().numpy() for p in branches[b]], precision=precision)
            assert _same(nets[b].export(), torch.from_numpy(want).cuda()), (t, b)
    assert opt.steps == steps
    # the float64 rule and torch.optim.Adam in float32 on the CPU, on the gradients the rule took
    tparams = [torch.nn.Parameter(torch.from_numpy(a.copy())) for a in start]
    topt = torch.optim.Adam(tparams, foreach=False, **pk.ADAM_HYPER)
    p64 = [a.astype(np.float64) for a in start]
    m64, v64 = [np.zeros_like(a) for a in p64], [np.zeros_like(a) for a in p64]
    for t, gs in enumerate(used, start=1):
        for i, g in enumerate(gs):
            p64[i], m64[i], v64[i] = pk.adam_ref(p64[i], g, m64[i], v64[i], t=t, **pk.ADAM_HYPER)
            tparams[i].grad = torch.from_numpy(g.copy())
        topt.step()
    ours = {"p": [p.detach().cpu().numpy() for p in branches[0]], "exp_avg": [opt.state[p]["exp_avg"].cpu().numpy() for p in branches[0]],
            "exp_avg_sq": [opt.state[p]["exp_avg_sq"].cpu().numpy() for p in branches[0]]}
    theirs = {"p": [p.detach().numpy() for p in tparams], "exp_avg": [topt.state[p]["exp_avg"].numpy() for p in tparams],
              "exp_avg_sq": [topt.state[p]["exp_avg_sq"].numpy() for p in tparams]}
    for what, exact in (("p", p64), ("exp_avg", m64), ("exp_avg_sq", v64)):
        for i in range(6):
            d_ours = float(np.abs(ours[what][i].astype(np.float64) - exact[i]).max())
            d_torch = float(np.abs(theirs[what][i].astype(np.float64) - exact[i]).max())
            assert d_ours <= 4.0 * d_torch, (what, i, d_ours, d_torch)
    assert np.array_equal(ours["p"][pk.ADAM_ZERO_TENSOR].view(np.uint32), start[pk.ADAM_ZERO_TENSOR].view(np.uint32))   # zero gradient, zero state
    for n in nets:
        n.close()


# ---------------------------------------------------------------- forward on synthetic records
def _device_records(case, n):
    import torch

    pool = torch.from_numpy(np.array(case["pool"])).to("cuda:0")
    return pool[torch.arange(n, device="cuda:0") % ref.POOL].contiguous()


def _forward_checked(got, case, precision, group, n):
    f = ref.forward_figures(got, case, precision)
    print("WIDE %s %s n=%d set=%s shape=%s range=%s rb=%d: |got-X| max %.3e mean %.3e  |got-Q| max %.3e mean %.3e  F %.3e  ratio %.3f"
          % (precision, group, n, case["wset"], case["shape"], case["feature_range"], case["record_bytes"], f["max_x"], f["mean_x"], f["max_q"],
             f["mean_q"], f["F"], f["ratio"]))
    if precision == "fp32":
        RATIOS[group] = max(RATIOS.get(group, 0.0), f["ratio"])
    assert ref.check_forward(got, case, precision) == []


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("shape", wref.FORWARD_SHAPES, ids=lambda s: "%dx%d" % s)
def test_rows_record_sizes_and_layouts(shape, precision):
    """1, 33 and 257 rows, row-major at the engine's record size and at one larger, tile-planar with a dirty partial last tile."""
    import torch

    rb0 = wref.engine_record_bytes(shape[0])
    for rb in (rb0, rb0 + 32):
        case = wref.forward_case(shape, "B", record_bytes=rb, feature_range=wref.GAME_RANGE)
        net = _case_net(case, precision)
        for n in (1, 33, 257):
            rows = wref.case_records(case, n)
            planar = ref.to_planar(rows, np.random.default_rng(n + rb))
            assert planar.shape == ((n + 63) // 64, rb // 16, 64, 16) and n % 64 != 0
            rec, pl = torch.from_numpy(rows).to("cuda:0"), torch.from_numpy(planar).to("cuda:0")
            a, b = _guarded(n, shape[1], torch.float32), _guarded(n, shape[1], torch.float32)
            assert net(rec, out=a[1]) is a[1]
            net(pl, out=b[1], planar=True)
            _intact(a, b)
            got = a[1].cpu().numpy()
            q = case["Q"][ref.Q_KEY[precision]][:n]
            assert np.isfinite(got).all()
            assert np.abs(got - q).max() <= (ref.M_FP32 * case["F"] if precision == "fp32" else ref.EMU_BF16["max"]), (n, rb)
            assert torch.equal(a[1], b[1])                      # the layout changes where a byte lies, nothing else
        n = ref.POOL + 33
        out = _guarded(n, shape[1], torch.float32)
        net(_device_records(case, n), out=out[1])
        _intact(out)
        _forward_checked(out[1].cpu().numpy(), case, precision, "shapes", n)


def _sweep_forward(shape, precision):
    """POOL + 33 row-major rows at the engine's record size, weight set B, game-range features, held to the project's bounds; then 257
    rows tile-planar with a dirty partial last tile: the bits of the row-major launch, guard rows intact."""
    import torch

    KS, mks = wide.ksteps(shape[0]), wref.kernel_ksteps(shape[0])
    case = wref.forward_case(shape, "B", feature_range=wref.GAME_RANGE)
    assert case["record_bytes"] == wref.engine_record_bytes(shape[0]) >= 16 * KS
    net = _case_net(case, precision)
    n = ref.POOL + 33
    out = _guarded(n, shape[1], torch.float32)
    net(_device_records(case, n), out=out[1])
    _intact(out)
    got = out[1].cpu().numpy()
    print("SWEEP obs %d out %d KS %d MKS %d padding %d" % (shape[0], shape[1], KS, mks, mks - KS))
    _forward_checked(got, case, precision, "sweep", n)
    if precision == "fp32":
        per_ks = "sweep-ks%02d" % KS
        RATIOS[per_ks] = max(RATIOS.get(per_ks, 0.0), ref.forward_figures(got, case, precision)["ratio"])
    n = 257
    rows = wref.case_records(case, n)
    planar = ref.to_planar(rows, np.random.default_rng(n + shape[0]))
    assert planar.shape == ((n + 63) // 64, case["record_bytes"] // 16, 64, 16)
    a, b = _guarded(n, shape[1], torch.float32), _guarded(n, shape[1], torch.float32)
    net(torch.from_numpy(rows).to("cuda:0"), out=a[1])
    net(torch.from_numpy(planar).to("cuda:0"), out=b[1], planar=True)
    _intact(a, b)
    assert torch.equal(a[1], b[1])
    assert ref.check_forward(a[1].cpu().numpy(), case, precision) == []


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("obs_dim", wref.SWEEP_OBS)
def test_forward_at_every_sweep_width(obs_dim, precision):
    """26 outputs at every width of net_wide_ref.SWEEP_OBS: every (MKS, KS) pair - so every number of padding k-steps either
    instantiation can run -, every multiple of 16, 16 k - 1, both sides of the switch at 79 / 80."""
    _sweep_forward((obs_dim, 26), precision)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("obs_dim", sorted(wref.ONE_PER_KS.values()))
def test_forward_with_one_output_at_one_width_per_kstep_count(obs_dim, precision):
    _sweep_forward((obs_dim, 1), precision)


def test_records_shorter_than_layer_1_are_refused():
    import torch
    from skyjo_rl_amd import _lib

    case = wref.forward_case((67, 26), "B", feature_range=wref.GAME_RANGE)
    net = _case_net(case, "bf16")
    with pytest.raises(_lib.SkyjoNativeError):
        net(torch.zeros((8, 64), dtype=torch.uint8, device="cuda:0"))          # K = 80 columns do not lie inside 64 bytes


def _one_net_passes(obs_dim, precision):
    import torch

    n = ONE_NET_PASSES_ROWS
    assert launch_geometry(n, 1)[0] == 2
    case = wref.forward_case((obs_dim, 26), "B", feature_range=wref.GAME_RANGE)
    out = _guarded(n, 26, torch.float32)
    _case_net(case, precision)(_device_records(case, n), out=out[1])
    _intact(out)
    _forward_checked(out[1].cpu().numpy(), case, precision, "rows-one-net", n)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_one_net_with_passes_above_one(precision):
    _one_net_passes(67, precision)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_one_net_with_passes_above_one_and_padding_ksteps(precision):
    """91 inputs (six players): KS = 6 of the instantiation for 11 - a workgroup's second batch runs its five padding k-steps again."""
    assert (wide.ksteps(91), wref.kernel_ksteps(91)) == (6, 11)
    _one_net_passes(91, precision)


@pytest.fixture(scope="module")
def envs():
    """Direct-observation engines of 64 games: the geometry FusedNet.act reads (record size, mask offset)."""
    from skyjo_rl_amd import SkyjoVecEnv

    made = {}
    for N in range(1, 13):
        env = SkyjoVecEnv(64, num_players=N, observe_other_player_indirect=False)
        D = 19 + 12 * N
        assert (env.obs_dim, env.mask_offset, env.record_bytes) == (D, (D + 3) & ~3, wref.engine_record_bytes(D))
        made[N] = env
    yield made
    for env in made.values():
        env.close()


def _two_nets_passes(N, precision, envs):
    import torch

    n = TWO_NET_PASSES_ROWS
    assert launch_geometry(n, 2)[0] == 2
    D, off = envs[N].obs_dim, envs[N].mask_offset
    pc = wref.forward_case((D, 26), "B", feature_range=wref.GAME_RANGE)
    vc = wref.forward_case((D, 1), "B", feature_range=wref.GAME_RANGE)
    assert np.array_equal(pc["pool"], vc["pool"])                              # one set of records, two nets
    pol, val = _case_net(pc, precision), _case_net(vc, precision)
    rec = _device_records(pc, n)
    logits, values = _guarded(n, 26, torch.float32), _guarded(n, 1, torch.float32)
    actions, logp = _guarded(n, 0, torch.int32), _guarded(n, 0, torch.float32)
    pol.act(envs[N], rec, seed=5, ticket=9, actions=actions[1], logp=logp[1], logits=logits[1], value_net=val, values=values[1])
    _intact(logits, values, actions, logp)
    _forward_checked(logits[1].cpu().numpy(), pc, precision, "rows-two-nets", n)
    _forward_checked(values[1].cpu().numpy(), vc, precision, "rows-two-nets", n)
    a = actions[1].long()
    assert bool(((a >= 0) & (a < 26)).all())
    assert bool(rec[:, off:off + 26].gather(1, a[:, None]).ne(0).all())        # (every byte of a record is random: legal = non-zero)
    assert torch.equal(pol(rec), logits[1]) and torch.equal(val(rec), values[1])  # the single-net launches (passes = 1): same bits


@pytest.mark.parametrize("precision", PRECISIONS)
def test_two_nets_in_one_launch_with_passes_above_one(precision, envs):
    assert (envs[4].obs_dim, envs[4].mask_offset) == (67, 68)
    _two_nets_passes(4, precision, envs)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_two_nets_in_one_launch_with_passes_above_one_and_a_padding_kstep(precision, envs):
    """151 inputs (eleven players): KS = 10 of 11, the policy and the value net of one launch each run one padding k-step per batch."""
    assert envs[11].obs_dim == 151 and (wide.ksteps(151), wref.kernel_ksteps(151)) == (10, 11)
    _two_nets_passes(11, precision, envs)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("feature_range", [wref.GAME_RANGE, (-128, 127)], ids=["game", "int8"])
@pytest.mark.parametrize("wset", ref.WEIGHT_SETS)
@pytest.mark.parametrize("shape", [(67, 26), (163, 26), (91, 26), (151, 26)], ids=lambda s: "%dx%d" % s)
def test_weight_sets_and_the_full_int8_range(shape, wset, feature_range, precision):
    import torch

    n = ref.POOL + 33
    case = wref.forward_case(shape, wset, feature_range=feature_range)
    out = _guarded(n, shape[1], torch.float32)
    _case_net(case, precision)(_device_records(case, n), out=out[1])
    _intact(out)
    _forward_checked(out[1].cpu().numpy(), case, precision, "set-%s-%s" % (wset, "game" if feature_range == wref.GAME_RANGE else "int8"), n)


# ---------------------------------------------------------------- the pair draw behind a wide net
DRAW_ROWS = 1197          # 19 rows of every (mask family, logit family position) pair: 9 x 7 x 19


MASK_OVER_THREE_PIECES = (2, 3, 6, 7, 10, 11)          # player counts whose mask offset is 8 or 12 mod 16: 26 bytes from there reach a third piece


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("N", list(range(1, 13)))
def test_act_is_the_one_lane_draw_on_the_launchs_logits(N, precision, envs):
    """FusedNet.act with and without a value net, row-major and tile-planar: actions and logp are the bits of
    skyjo_vec_sample_actions_layout on the same launch's logits.  Every player count on the direct observation; one player is 31
    inputs, the narrow kernels on a direct-observation record.  At four players the mask (bytes 68 .. 93) straddles two 16-byte pieces,
    as at 1, 5, 8, 9 and 12; at 2, 3, 6, 7, 10 and 11 players it lies over three."""
    import torch

    env = envs[N]
    D, rb, off = env.obs_dim, env.record_bytes, env.mask_offset
    if N == 4:
        assert off // 16 != (off + 25) // 16 and (off, off + 25) == (68, 93)
    assert (off + 25) // 16 - off // 16 == (2 if N in MASK_OVER_THREE_PIECES else 1)
    assert (D > 31) == (N > 1)
    pol = _net(ref.weights((D, 26), "B"), precision, ((D, 26), "B"))
    val = _net(ref.weights((D, 1), "B"), precision, ((D, 1), "B"))
    seed, ticket = 2 ** 32 + 3, 2 ** 40 + 1
    case = ref.draw_case(DRAW_ROWS, seed, ticket, rng_seed=N, record_bytes=rb, mask_offset=off, obs_dim=D)
    n = case["n"]
    rec = torch.from_numpy(case["records"]).to("cuda:0")
    single = [torch.empty((n, 26), device="cuda:0"), torch.empty(n, dtype=torch.int32, device="cuda:0"), torch.empty(n, device="cuda:0")]
    for with_value in (False, True):
        lg, a, lp, v = _guarded(n, 26, torch.float32), _guarded(n, 0, torch.int32), _guarded(n, 0, torch.float32), _guarded(n, 1, torch.float32)
        kw = dict(value_net=val, values=v[1]) if with_value else {}
        pol.act(env, rec, seed=seed, ticket=ticket, actions=a[1], logp=lp[1], logits=lg[1], **kw)
        _intact(lg, a, lp, v)
        if with_value:
            assert torch.equal(lg[1], single[0]) and torch.equal(a[1], single[1]) and torch.equal(lp[1].view(torch.int32), single[2].view(torch.int32))
            assert torch.equal(v[1], val(rec))
            continue
        single = [lg[1].clone(), a[1].clone(), lp[1].clone()]
        assert torch.equal(lg[1], pol(rec))
        logits = lg[1].clone()
        lp1, u1 = torch.empty(n, device="cuda:0"), torch.empty(n, device="cuda:0")
        a1 = env.sample_actions(logits, rec, seed=seed, ticket=ticket, logp=lp1, uniform=u1)
        assert torch.equal(a1, a[1]) and torch.equal(lp1.view(torch.int32), lp[1].view(torch.int32))
        got_a = a[1].cpu().numpy()
        assert ref.check_draw(got_a, lp[1].cpu().numpy(), u1.cpu().numpy(), ref.with_logits(case, logits.cpu().numpy())) == []
        for fam in ("single", "draw-phase"):                    # masked actions are never drawn
            rows = np.flatnonzero(case["mask_family"] == ref.MASK_FAMILIES.index(fam))
            assert rows.size > 100 and (case["mask"][rows, got_a[rows]] == 1).all(), fam
    # tile-planar: ONE iteration's block of the engine (64 games), dirty beyond them
    rows64 = case["records"][:64]
    pl = torch.from_numpy(ref.to_planar(rows64[:50], np.random.default_rng(N))).to("cuda:0")
    small = type(env)(50, num_players=N, observe_other_player_indirect=False)
    a_rm, lp_rm, lg_rm = torch.empty(50, dtype=torch.int32, device="cuda:0"), torch.empty(50, device="cuda:0"), torch.empty((50, 26), device="cuda:0")
    a_pl, lp_pl, lg_pl = _guarded(50, 0, torch.int32), _guarded(50, 0, torch.float32), _guarded(50, 26, torch.float32)
    v_rm, v_pl = torch.empty((50, 1), device="cuda:0"), _guarded(50, 1, torch.float32)
    pol.act(small, torch.from_numpy(rows64[:50].copy()).to("cuda:0"), seed=seed, ticket=ticket, actions=a_rm, logp=lp_rm, logits=lg_rm, value_net=val, values=v_rm)
    pol.act(small, pl, seed=seed, ticket=ticket, actions=a_pl[1], logp=lp_pl[1], logits=lg_pl[1], value_net=val, values=v_pl[1], planar=True)
    _intact(a_pl, lp_pl, lg_pl, v_pl)
    assert torch.equal(a_rm, a_pl[1]) and torch.equal(lp_rm.view(torch.int32), lp_pl[1].view(torch.int32)) and torch.equal(lg_rm, lg_pl[1])
    assert torch.equal(v_rm, v_pl[1]) and torch.equal(a_rm, single[1][:50])
    small.close()


# ---------------------------------------------------------------- the engine on the direct observation
B_ENGINE, T_ENGINE = 130, 40


COLUMNS = ("records", "actions", "logp", "values", "final_rewards", "episode_end")


def _column(buf, name):
    """A column of a rollout buffer; of the records the bytes the engine defines (mask_offset + 32 of record_bytes: at two players the
    last four of the 80 are padding that nobody writes)."""
    x = getattr(buf, name)
    return x[..., :buf._env.mask_offset + 32].contiguous() if name == "records" else x


def _cfg(N, indirect=False):
    return dict(num_players=N, score_penalty=2.0, observe_other_player_indirect=indirect, mean_reward=1.0, reward_refunded=0.001, rng_mode=0,
                auto_reset=True)


# The player counts of the model rollouts.  Direct observation: one player (31 inputs: the narrow nets on a direct-observation record),
# two to four (the step kernels compiled for their count), five to twelve (the generic-N step kernel under skyjo_vec_step_collect;
# five is the last width of the instantiation for 5 k-steps, eight and eleven run the one for 11 with padding k-steps, twelve without).
# Indirect observation at five and twelve players: narrow nets on the generic step kernels.
ROLLOUT_RUNS = [1, 2, 3, 4, 5, 8, 11, 12, (5, True), (12, True)]


def _run_id(p):
    return "%d" % p if isinstance(p, int) else "%d-indirect" % p[0]


def _rollout_run(N, indirect, forms):
    import torch
    from skyjo_rl_amd import SkyjoVecEnv
    from skyjo_rl_amd.action_mask_model import ActionMaskModel, FusedNet
    from skyjo_rl_amd.rollout import RolloutBuffer

    D = 31 if indirect else 19 + 12 * N
    torch.manual_seed(4 + N)
    model = ActionMaskModel(obs_dim=D).cuda()
    pol, val = FusedNet(model.policy), FusedNet(model.value)
    bufs, envs_ = {}, []
    for form in forms:
        env = SkyjoVecEnv(B_ENGINE, **_cfg(N, indirect))
        assert env.obs_dim == D and env.num_players == N
        env.seed(None, 33)
        buf = RolloutBuffer(env, T_ENGINE)
        form(env, pol, val, buf, seed=8, first_ticket=0)
        assert env.counters()["illegal"] == 0
        bufs[form.__name__] = buf
        envs_.append(env)
    return dict(N=N, indirect=indirect, model=model, pol=pol, val=val, bufs=bufs, envs=envs_)


def _close_run(run):
    run["pol"].close(), run["val"].close()
    for env in run["envs"]:
        env.close()


@pytest.fixture(scope="module", params=ROLLOUT_RUNS, ids=_run_id)
def rollout_run(request):
    """rollout.collect and collect_stepwise on two engines seeded alike, the model and its nets: computed once per player count."""
    from skyjo_rl_amd.rollout import collect, collect_stepwise

    N, indirect = (request.param, False) if isinstance(request.param, int) else request.param
    run = _rollout_run(N, indirect, (collect, collect_stepwise))
    yield run
    _close_run(run)


@pytest.fixture(scope="module", params=[2, 4])
def ppo_run(request):
    """A model, its nets and one collected buffer of their own: the PPO update moves them."""
    from skyjo_rl_amd.rollout import collect

    run = _rollout_run(request.param, False, (collect,))
    yield run
    _close_run(run)


def test_collect_equals_the_stepwise_loop(rollout_run):
    import torch

    a, b = rollout_run["bufs"]["collect"], rollout_run["bufs"]["collect_stepwise"]
    for name in COLUMNS:
        x, y = _column(a, name), _column(b, name)
        assert x.shape == y.shape and torch.equal(x.view(torch.uint8), y.view(torch.uint8)), name
    assert float(a.values.abs().max()) > 0 and bool(torch.isfinite(a.logp).all())


def records_against_the_oracle(env, buf, ora, step=None, whole_rewards=False):
    """Every record of a filled buffer, ``episode_end`` and ``final_rewards`` against an oracle that stands where the rollout started and
    is stepped under the buffer's actions (``step``: the call that steps it, default ``ora.step``).  ``whole_rewards``: the rows of games
    that did not end hold 0.0 as well.  Returns (episode ends, bool [B]: the games that ended inside the buffer)."""
    step = step or (lambda a: ora.step(a, threads=1))
    actions = buf.actions.cpu().numpy()
    ends, ended = 0, np.zeros(buf.B, dtype=bool)
    for t in range(buf.T + 1):
        v = env.split(buf.records[t])
        obs, mask, agent, phase = ora.observe()
        np.testing.assert_array_equal(v.observations.cpu().numpy(), obs, err_msg=f"obs t={t}")
        np.testing.assert_array_equal(v.action_mask.cpu().numpy(), mask, err_msg=f"mask t={t}")
        np.testing.assert_array_equal(v.agent.cpu().numpy(), agent)
        np.testing.assert_array_equal(v.phase.cpu().numpy(), phase)
        if t:
            dn = ora.dones.astype(bool)
            np.testing.assert_array_equal(v.done.cpu().numpy().astype(bool), dn, err_msg=f"done t={t}")
            np.testing.assert_array_equal(buf.episode_end[t - 1].cpu().numpy().astype(bool), dn, err_msg=f"episode_end t={t}")
            if dn.any():
                ends += int(dn.sum())
                ended |= dn
                np.testing.assert_array_equal(buf.final_rewards[t - 1].cpu().numpy()[dn], ora.rewards[dn], err_msg=f"rewards t={t}")
            if whole_rewards:
                np.testing.assert_array_equal(buf.final_rewards[t - 1].cpu().numpy(), np.where(dn[:, None], ora.rewards, 0.0), err_msg=f"rewards t={t}")
        if t < buf.T:
            step(actions[t])
    return ends, ended


def test_collects_records_are_the_oracles_under_the_buffers_actions(rollout_run):
    from oracle import skyjo_oracle as so

    N, buf, env = rollout_run["N"], rollout_run["bufs"]["collect"], rollout_run["envs"][0]
    ora = so.OracleVec(num_envs=B_ENGINE, **_cfg(N, rollout_run["indirect"]))
    ora.seed(None, 33)
    ends, _ = records_against_the_oracle(env, buf, ora)
    print("episodes ended inside the rollout:", ends)


def test_arena_collect_with_one_policy_on_every_seat_is_collect(rollout_run):
    import torch
    from skyjo_rl_amd import SkyjoVecEnv, arena
    from skyjo_rl_amd.rollout import RolloutBuffer

    N, pol, val, want = rollout_run["N"], rollout_run["pol"], rollout_run["val"], rollout_run["bufs"]["collect"]
    env = SkyjoVecEnv(B_ENGINE, **_cfg(N, rollout_run["indirect"]))
    env.seed(None, 33)
    got = RolloutBuffer(env, T_ENGINE)
    arena.collect(env, [("sample", pol)] * N, [val] * N, got, seed=8, first_ticket=0)
    for name in COLUMNS:
        assert torch.equal(_column(got, name).view(torch.uint8), _column(want, name).view(torch.uint8)), name
    env.close()


def test_a_greedy_wide_net_against_random_seats_yields_episodes(rollout_run):
    from skyjo_rl_amd import SkyjoVecEnv, arena

    N, pol = rollout_run["N"], rollout_run["pol"]
    env = SkyjoVecEnv(B_ENGINE, **_cfg(N, rollout_run["indirect"]))
    env.seed(None, 5)
    env.reset()
    # (one player has no random seat beside it: a lone greedy seat of an untrained net repeats one draw-and-discard for ever - 0
    # episodes in 400 iterations on the MI355X -, so the one seat samples)
    stats = arena.evaluate(env, [("greedy", pol) if N > 1 else ("sample", pol)] + ["random"] * (N - 1), 400, seed=3)
    assert stats.episodes > 0 and len(stats.mean_reward) == N and all(np.isfinite(stats.mean_reward))
    assert env.counters()["illegal"] == 0
    env.close()


def test_behaviour_logits_read_the_rollouts_records_in_either_layout(rollout_run):
    """The rollout's records re-laid tile-planar (the engine writes 'tile-planar-all' records of the indirect observation only) give the
    policy net the same logits, and the recorded logp is the masked log-softmax of them at the recorded action."""
    import torch
    from skyjo_rl_amd.rollout import behaviour_logits

    N, pol, buf, env = rollout_run["N"], rollout_run["pol"], rollout_run["bufs"]["collect"], rollout_run["envs"][0]
    assert behaviour_logits(buf, pol) is buf
    lg = buf.behaviour
    assert tuple(lg.shape) == (T_ENGINE, B_ENGINE, 26)
    t = T_ENGINE // 2
    planar = torch.from_numpy(ref.to_planar(buf.records[t].cpu().numpy(), np.random.default_rng(t))).to("cuda:0")
    out = torch.empty((B_ENGINE, 26), device="cuda:0")
    pol(planar, out=out, planar=True)
    assert torch.equal(out, lg[t])
    v = env.split(buf.records[t])
    masked = lg[t].double() + torch.where(v.action_mask != 0, 0.0, float(ref.FLOAT_MIN)).double()
    own = torch.log_softmax(masked, -1).gather(1, buf.actions[t].long()[:, None])[:, 0]
    assert float((own - buf.logp[t].double()).abs().max()) < 1e-5 + 4 * 2.0 ** -24 * float(own.abs().max())


def test_one_ppo_update_through_autograd_moves_parameters_and_blobs(ppo_run):
    import torch
    from examples.ppo import ppo_update
    from skyjo_rl_amd.learner import NativeAdam

    model, pol, val, buf = ppo_run["model"], ppo_run["pol"], ppo_run["val"], ppo_run["bufs"]["collect"]
    before = [p.detach().clone() for p in model.parameters()]
    blobs = [pol.export().clone(), val.export().clone()]
    opt = NativeAdam(model, pol, val, lr=3e-4)
    with pytest.raises(ValueError, match="1..31 inputs"):
        ppo_update(model, buf, opt, epochs=1, minibatch=2048, gae=(0.99, 0.95), native_batches=True, native_loss=True, native_nets=True)
    assert all(torch.equal(p.detach(), q) for p, q in zip(model.parameters(), before))
    out = ppo_update(model, buf, opt, epochs=1, minibatch=2048, gae=(0.99, 0.95), native_batches=True, native_loss=True)
    assert out["transitions"] > 0
    assert all(float((p.detach() - q).abs().max()) > 0 for p, q in zip(model.parameters(), before))
    assert not torch.equal(pol.export(), blobs[0]) and not torch.equal(val.export(), blobs[1])
    for net, seq in ((pol, model.policy), (val, model.value)):
        want = wide.pack(*[p.detach().cpu().numpy() for p in seq.parameters()], precision="fp32")
        assert torch.equal(net.export(), torch.from_numpy(want).cuda())


def test_zz_float32_grade_ratios_of_this_run():
    """Last in the module: the largest max |got - Q| / F per group of wide cases of the float32-grade mode in this run, against the
    project's factor (tests/net_ref.py: M_FP32)."""
    for k in sorted(RATIOS):
        print("WIDERATIO %s %.3f" % (k, RATIOS[k]))
    assert all(v <= ref.M_FP32 for v in RATIOS.values())
