"""The inference hot path - ``k_net_split`` / ``k_net_bf16`` (csrc/skyjo_policy.hip), ``k_sample`` (csrc/skyjo_callers.h) and the two draw
forms of csrc/skyjo_draw.h - on the synthetic records, masks and logits of tests/net_ref.py, against its float64 references and
through its checks (the ones tests/test_net_ref.py shows to reject restated wrong kernels): every launch geometry of ``sk_launch_mlp``
(`passes` 1 .. 8, the cap, a second round of workgroups, fewer than 33 rows), every row compared with ITS record's reference (row g
holds pool row g % 4099), the full int8 range, saturated and near-zero hidden layers, dirty tile-planar padding, the draw's uniform
bit for bit against Philox4x32-10 with every high word in use, and mask / logit patterns no game writes.  Outputs sit between
sentinel-filled guard rows that must stay untouched.

Tolerances (tests/net_ref.py: check_forward, check_draw): T1 = 4 x the project's TOL against the exact float64 net where the project
measured it (features in [-32, 31], weight sets A and B); T2 against the packed arithmetic evaluated in float64, everywhere - "bf16":
max < 2e-2, mean < 2e-3; "fp32": M_FP32 x F, F the float32 torch module's own deviation on the case."""
import numpy as np
import pytest

from tests import net_ref as ref

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0DEAD         # a NaN with a payload, as float32 bits
GUARD_ROWS = 4                # rows before and after every output (a multiple of 16 bytes for every width)
ONE_NET_ROWS = (1, 31, 32, 33, 255, 256, 257, 513, 65535, 65536, 65537, 131073, 458753, 524289)
TWO_NET_ROWS = (32768, 32769, 229377, 262145)
DRAW_ROWS = 6553              # tests/test_net_ref.py: 104 rows of every (mask family, logit family) pair
HIGH_ID0 = 2 ** 32 - 100      # the game id's high word changes inside the batch
SEED_TICKET = ((0, 0), (77, 5), (2 ** 32 + 3, 2 ** 40 + 1), (2 ** 64 - 1, 2 ** 64 - 1))
RATIOS = {}                   # group -> largest max |got - Q| / F of the float32-grade mode in this run


def launch_geometry(n, nets):
    """(passes, workgroups per net) as sk_launch_mlp states them."""
    batches = (n + 255) // 256
    passes = min(8, max(1, (batches * nets + 255) // 256))
    return passes, (batches + passes - 1) // passes


def test_row_counts_reach_the_launch_geometries_they_claim():
    g1 = {n: launch_geometry(n, 1) for n in ONE_NET_ROWS}
    assert [g1[n][0] for n in (65535, 65536, 65537, 131073, 458753, 524289)] == [1, 1, 2, 3, 8, 8]
    assert g1[458753][1] == 225 and g1[524289][1] == 257                       # `passes` = 8 by count; the cap and a second round
    g2 = {n: launch_geometry(n, 2) for n in TWO_NET_ROWS}
    assert [g2[n] for n in TWO_NET_ROWS] == [(1, 128), (2, 65), (8, 113), (8, 129)]   # 2 x 129 = 258 workgroups


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


_NETS = {}


def _net(params, precision, key=None):
    """A FusedNet of the numpy parameters (cached under ``key``)."""
    import torch
    from torch import nn

    from skyjo_rl_amd.action_mask_model import FusedNet

    if key is not None and (key, precision) in _NETS:
        return _NETS[(key, precision)]
    obs_dim, out_dim = params[0].shape[1], params[4].shape[0]
    seq = nn.Sequential(nn.Linear(obs_dim, 256), nn.Tanh(), nn.Linear(256, 256), nn.Tanh(), nn.Linear(256, out_dim))
    with torch.no_grad():
        for lin, (w, b) in zip((seq[0], seq[2], seq[4]), ((params[0], params[1]), (params[2], params[3]), (params[4], params[5]))):
            lin.weight.copy_(torch.from_numpy(np.array(w)))
            lin.bias.copy_(torch.from_numpy(np.array(b)))
    net = FusedNet(seq, precision=precision)
    if key is not None:
        _NETS[(key, precision)] = net
    return net


def _case_net(case, precision):
    return _net(case["params"], precision, key=(case["shape"], case["wset"]))


def _device_records(case, n):
    """uint8 [n, record_bytes] on the GPU: row g is pool row g % POOL (gathered there from the numpy pool)."""
    import torch

    pool = torch.from_numpy(np.array(case["pool"])).to("cuda:0")
    return pool[torch.arange(n, device="cuda:0") % ref.POOL].contiguous()


def _forward_checked(got, case, precision, group, n):
    f = ref.forward_figures(got, case, precision)
    print("T2 %s %s n=%d set=%s shape=%s range=%s: |got-X| max %.3e mean %.3e  |got-Q| max %.3e mean %.3e  F %.3e  ratio %.3f"
          % (precision, group, n, case["wset"], case["shape"], case["feature_range"], f["max_x"], f["mean_x"], f["max_q"], f["mean_q"], f["F"], f["ratio"]))
    if precision == "fp32":
        RATIOS[group] = max(RATIOS.get(group, 0.0), f["ratio"])
        for key in ("fp32", "fp32-act32"):                                     # (both forms of Q, whichever the check uses)
            d = float(ref._cyclic_diff(got, case["Q"][key]).max())
            print("T2Q %s %s n=%d set=%s shape=%s range=%s max %.3e ratio %.3f" % (key, group, n, case["wset"], case["shape"], case["feature_range"], d, d / case["F"]))
    assert ref.check_forward(got, case, precision) == []


@pytest.fixture(scope="module")
def env64():
    from skyjo_rl_amd import SkyjoVecEnv

    env = SkyjoVecEnv(64)
    assert (env.obs_dim, env.mask_offset, env.record_bytes) == (31, 32, 64)    # the geometry the family records are laid out for
    yield env
    env.close()


@pytest.fixture(scope="module")
def env_high():
    from skyjo_rl_amd import SkyjoVecEnv

    env = SkyjoVecEnv(64, game_id0=HIGH_ID0)
    assert (env.obs_dim, env.mask_offset, env.record_bytes) == (31, 32, 64)
    yield env
    env.close()


# ---------------------------------------------------------------- launch geometry
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("n", ONE_NET_ROWS)
def test_one_net_at_every_launch_geometry(n, precision):
    import torch

    case = ref.forward_case((31, 26), "B", feature_range=ref.T1_RANGE)
    net = _case_net(case, precision)
    rec = _device_records(case, n)
    out = _guarded(n, 26, torch.float32)
    assert net(rec, out=out[1]) is out[1]
    _intact(out)
    _forward_checked(out[1].cpu().numpy(), case, precision, "rows-one-net", n)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("n", TWO_NET_ROWS)
def test_two_nets_in_one_launch_at_every_launch_geometry(n, precision, env64):
    import torch

    pc = ref.forward_case((31, 26), "B", feature_range=ref.T1_RANGE)
    vc = ref.forward_case((31, 1), "B", feature_range=ref.T1_RANGE)
    assert np.array_equal(pc["pool"], vc["pool"])                             # one set of records, two nets
    pol, val = _case_net(pc, precision), _case_net(vc, precision)
    rec = _device_records(pc, n)
    logits, values = _guarded(n, 26, torch.float32), _guarded(n, 1, torch.float32)
    actions, logp = _guarded(n, 0, torch.int32), _guarded(n, 0, torch.float32)
    pol.act(env64, rec, seed=5, ticket=9, actions=actions[1], logp=logp[1], logits=logits[1], value_net=val, values=values[1])
    _intact(logits, values, actions, logp)
    _forward_checked(logits[1].cpu().numpy(), pc, precision, "rows-two-nets", n)
    _forward_checked(values[1].cpu().numpy(), vc, precision, "rows-two-nets", n)
    a = actions[1].long()
    assert bool(((a >= 0) & (a < 26)).all())
    assert bool(rec[:, 32:58].gather(1, a[:, None]).ne(0).all())               # (every byte of a record is random: legal = non-zero)
    assert torch.equal(pol(rec), logits[1]) and torch.equal(val(rec), values[1])  # the single-net launches (other `passes`): same bits
    lp = logp[1]
    own = torch.log_softmax(logits[1].double() + torch.where(rec[:, 32:58] != 0, 0.0, float(ref.FLOAT_MIN)).double(), -1).gather(1, a[:, None])[:, 0]
    assert float((own - lp.double()).abs().max()) < 1e-5 + 4 * 2.0 ** -24 * float(own.abs().max())


# ---------------------------------------------------------------- shapes and layouts
@pytest.mark.parametrize("record_bytes", [32, 48, 64, 112])
@pytest.mark.parametrize("shape", ref.SHAPES)
def test_every_shape_record_size_and_layout(shape, record_bytes):
    import torch

    for n, rng_ in ((777, ref.T1_RANGE), (4100, (-128, 127))):
        case = ref.forward_case(shape, "B", record_bytes=record_bytes, feature_range=rng_)
        rows = ref.case_records(case, n)
        planar = ref.to_planar(rows, np.random.default_rng(n + record_bytes))
        assert planar.shape == ((n + 63) // 64, record_bytes // 16, 64, 16) and n % 64 != 0
        rec, pl = torch.from_numpy(rows).to("cuda:0"), torch.from_numpy(planar).to("cuda:0")
        for precision in ("fp32", "bf16"):
            net = _case_net(case, precision)
            a, b = _guarded(n, shape[1], torch.float32), _guarded(n, shape[1], torch.float32)
            net(rec, out=a[1])
            net(pl, out=b[1], planar=True)
            _intact(a, b)
            _forward_checked(a[1].cpu().numpy(), case, precision, "shapes", n)
            assert torch.equal(a[1], b[1])                                     # the layout changes where a byte lies, nothing else


# ---------------------------------------------------------------- inputs
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("feature_range", [ref.T1_RANGE, (-128, 127)], ids=["small", "int8"])
@pytest.mark.parametrize("wset", ref.WEIGHT_SETS)
def test_weight_sets_and_the_full_int8_range(wset, feature_range, precision):
    import torch

    n = 4100 + 33
    case = ref.forward_case((31, 26), wset, feature_range=feature_range)
    out = _guarded(n, 26, torch.float32)
    _case_net(case, precision)(_device_records(case, n), out=out[1])
    _intact(out)
    _forward_checked(out[1].cpu().numpy(), case, precision, "set-%s-%s" % (wset, "small" if feature_range == ref.T1_RANGE else "int8"), n)


# ---------------------------------------------------------------- the uniform and the one-lane draw
def _sample(env, case, no_masking):
    import torch

    n = case["n"]
    rec, lg = torch.from_numpy(case["records"]).to("cuda:0"), torch.from_numpy(case["logits"]).to("cuda:0")
    a, lp, u = _guarded(n, 0, torch.int32), _guarded(n, 0, torch.float32), _guarded(n, 0, torch.float32)
    env.sample_actions(lg, rec, seed=case["seed"], ticket=case["ticket"], no_masking=no_masking, actions=a[1], logp=lp[1], uniform=u[1])
    _intact(a, lp, u)
    return a[1].cpu().numpy(), lp[1].cpu().numpy(), u[1].cpu().numpy()


@pytest.mark.parametrize("seed,ticket", SEED_TICKET)
def test_uniform_is_philox_word_0_bit_for_bit(seed, ticket, env64, env_high):
    for env, id0, n in ((env64, 0, DRAW_ROWS), (env_high, HIGH_ID0, 300)):
        case = ref.draw_case(n, seed, ticket, game_id0=id0)
        a, lp, u = _sample(env, case, False)
        assert np.array_equal(u.view(np.uint32), case["u"].view(np.uint32)), (seed, ticket, id0)
        assert ref.check_draw(a, lp, u, case) == []


@pytest.mark.parametrize("no_masking", [False, True])
def test_one_lane_draw_on_mask_and_logit_families(no_masking, env64, env_high):
    for env, id0, (seed, ticket) in ((env64, 0, SEED_TICKET[1]), (env_high, HIGH_ID0, SEED_TICKET[2])):
        case = ref.draw_case(DRAW_ROWS, seed, ticket, game_id0=id0, no_masking=no_masking)
        a, lp, u = _sample(env, case, no_masking)
        fails = ref.check_draw(a, lp, u, case)
        print("ambiguous rows", int(case["ref"]["ambiguous"].sum()), "differing from the reference", int((a != case["ref"]["action"]).sum()))
        assert fails == []
        if not no_masking:
            legal = case["mask"].sum(1) > 0
            assert (case["mask"][legal, a[legal]] == 1).all()


# ---------------------------------------------------------------- the pair draw
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["ties", "ramp", "sharp"])
def test_pair_draw_equals_one_lane_draw_and_the_reference(kind, precision, env_high):
    import torch

    net = _net(ref.steered(kind), precision, key=("steered", kind))
    seed, ticket = SEED_TICKET[2]
    for no_masking in (False, True):
        case = ref.draw_case(DRAW_ROWS, seed, ticket + no_masking, game_id0=HIGH_ID0, no_masking=no_masking, rng_seed=1)
        n = case["n"]
        rec = torch.from_numpy(case["records"]).to("cuda:0")
        lg, a, lp = _guarded(n, 26, torch.float32), _guarded(n, 0, torch.int32), _guarded(n, 0, torch.float32)
        net.act(env_high, rec, seed=seed, ticket=ticket + no_masking, no_masking=no_masking, actions=a[1], logp=lp[1], logits=lg[1])
        _intact(lg, a, lp)
        logits = lg[1].clone()                                                 # (16-byte aligned, as k_sample reads it)
        lp1, u1 = torch.empty(n, device="cuda:0"), torch.empty(n, device="cuda:0")
        a1 = env_high.sample_actions(logits, rec, seed=seed, ticket=ticket + no_masking, no_masking=no_masking, logp=lp1, uniform=u1)
        assert torch.equal(a1, a[1]) and torch.equal(lp1.view(torch.int32), lp[1].view(torch.int32))
        got = logits.cpu().numpy()
        if kind == "ties":
            assert (got == np.float32(1.25)).all()
        elif kind == "ramp":
            assert np.abs(got - np.linspace(0.0, -120.0, 26)).max() < 120 * 2.0 ** -16   # (a bias is the sum of two bf16 values)
        else:
            assert np.abs(got).max() > 20.0
        assert ref.check_draw(a[1].cpu().numpy(), lp[1].cpu().numpy(), u1.cpu().numpy(), ref.with_logits(case, got)) == []


def test_zz_float32_grade_ratios_of_this_run():
    """Last in the module: the largest max |got - Q| / F per group of cases of the float32-grade mode in this run, against the committed
    factor (tests/net_ref.py: M_FP32, RATIOS_SEEN)."""
    for k in sorted(RATIOS):
        print("T2RATIO %s %.3f" % (k, RATIOS[k]))
    assert all(v <= ref.M_FP32 for v in RATIOS.values())
