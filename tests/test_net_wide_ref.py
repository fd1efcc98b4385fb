"""tests/net_wide_ref.py without a GPU: its Q is net_ref's on a narrow net, its records are what they claim, and net_ref.check_forward
on a wide case accepts the reference's own float32 rounding and rejects three restated wrong kernels - one that sees only the first 32
features, one that takes the bias from column 31, one that lets byte obs_dim of the record in as a feature - by orders of magnitude.
The sweep: net_wide_ref.SWEEP_OBS holds every (MKS, KS) pair of the two wide instantiations and every edge, check_forward rejects three
restated wrong padding k-steps wherever KS < MKS and - the blind spot of 67 and 163 inputs, written down - accepts them where KS == MKS.
Last, the oracle alone: brink boards end episodes inside BRINK_T iterations of its random policy, twice as often as the GPU rollouts need."""
import numpy as np
import pytest

from tests import mlp_pack_ref as pk, mlp_pack_wide_ref as wide, net_ref as ref, net_wide_ref as wref

SMALL_POOL = 257


def _small_case(shape, wset="B", feature_range=wref.GAME_RANGE):
    """A case on a pool of SMALL_POOL rows (the CPU tests need no 4099)."""
    rng = np.random.default_rng(1000 * shape[0] + shape[1])
    rows = wref.wide_records(wref.engine_record_bytes(shape[0]), shape[0], rng, pool=SMALL_POOL, feature_range=feature_range)
    params = ref.weights(shape, wset)
    x = rows[:, :shape[0]].view(np.int8).astype(np.float64)
    X = ref.exact(params, x)
    return dict(shape=shape, wset=wset, params=params, pool=rows, x=x, X=X, t1=False, feature_range=feature_range,
                Q={"fp32": wref.packed(params, rows, "fp32"), "bf16": wref.packed(params, rows, "bf16"),
                   "fp32-act32": wref.packed(params, rows, "fp32", act32=True)},
                F=float(np.abs(ref.float32_module(params, x) - X).max()))


@pytest.fixture(scope="module", params=[(43, 26), (67, 1), (163, 26)], ids=lambda s: "%dx%d" % s)
def case(request):
    return _small_case(request.param)


def test_engine_record_bytes_of_the_direct_observation():
    assert [wref.engine_record_bytes(19 + 12 * n) for n in (2, 4, 12)] == [80, 112, 208]
    for d in (43, 47, 67, 163):
        assert wide.columns(d) <= d + 16 < wref.engine_record_bytes(d) + 16 and wide.columns(d) <= wref.engine_record_bytes(d)


def test_on_a_narrow_net_the_wide_q_is_net_refs():
    c = ref.forward_case((31, 26), "B", feature_range=ref.T1_RANGE)
    rows = c["pool"][:300]
    for precision, act32 in (("fp32", False), ("fp32", True), ("bf16", False)):
        got = wref.packed(c["params"], rows, precision, act32=act32)
        want = c["Q"]["fp32-act32" if act32 else precision][:300]
        assert np.array_equal(got, want)


def test_records_are_random_beyond_the_observation_and_hold_the_edge_rows():
    rows = wref.wide_records(112, 67, np.random.default_rng(5))
    feat = rows[:, :67].view(np.int8)
    assert (feat[1] == -128).all() and (feat[2] == 127).all() and (feat[3, ::2] == -128).all() and (feat[3, 1::2] == 127).all()
    assert (feat[4, ::2] == 127).all() and (feat[4, 1::2] == -128).all()
    for col in (67, 68, 93, 111):                                   # the action byte, the mask's first and last byte, the last byte
        assert np.unique(rows[:, col]).size > 200
    lo, hi = wref.GAME_RANGE
    f = wref.wide_records(80, 43, np.random.default_rng(6), feature_range=wref.GAME_RANGE)[:, :43].view(np.int8)
    assert f.min() == lo and f.max() == hi


def test_q_is_near_x(case):
    """float32-grade: the weights' 16 significant bits leave Q a few 1e-5 from X; bf16: well inside the project's 8e-2."""
    assert np.abs(case["Q"]["fp32"] - case["X"]).max() < 1e-3
    assert np.abs(case["Q"]["bf16"] - case["X"]).max() < 0.5
    assert np.abs(case["Q"]["fp32-act32"] - case["Q"]["fp32"]).max() < 1e-5


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_check_accepts_the_reference_rounded_to_float32(case, precision):
    got = case["Q"][ref.Q_KEY[precision]].astype(np.float32)
    assert ref.check_forward(got, case, precision) == []
    assert ref.check_forward(np.concatenate([got, got[:40]]), case, precision) == []     # (row g holds pool row g % pool)


def _figures(got, case, precision):
    q = case["Q"][ref.Q_KEY[precision]]
    return float(np.abs(got.astype(np.float64) - q).max())


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("wrong", ["first32", "bias31"])
def test_wrong_kernels_fail_by_orders_of_magnitude(case, wrong, precision):
    got = wref.packed(case["params"], case["pool"], precision, wrong=wrong, act32=precision == "fp32").astype(np.float32)
    d = _figures(got, case, precision)
    bound = ref.M_FP32 * case["F"] if precision == "fp32" else ref.EMU_BF16["max"]
    right = _figures(case["Q"][ref.Q_KEY[precision]].astype(np.float32), case, precision)
    print("%s %s %s: wrong %.3e right %.3e bound %.3e" % (case["shape"], wrong, precision, d, right, bound))
    assert right <= bound and d > 10 * bound
    if precision == "fp32":
        assert d > 1000 * bound


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_byte_obs_dim_as_a_feature(precision):
    """At 43 inputs column 43 of the packed layer 1 is zero: a kernel that lets byte 43 in computes the same - unless the blob has that
    column set, and then the check sees it.  At 47 inputs byte 47 is column K - 1, the bias column: the packed blob itself shows it,
    which is why 47 is among the GPU test's forward shapes."""
    c = _small_case((43, 26))
    params, rows = c["params"], c["pool"]
    bound = ref.M_FP32 * c["F"] if precision == "fp32" else ref.EMU_BF16["max"]
    act32 = precision == "fp32"
    q = c["Q"][ref.Q_KEY[precision]]
    assert np.array_equal(wref.packed(params, rows, precision, wrong="byte_obs", act32=act32), q)
    u = wide.unpack(wide.pack(*params, precision=precision), 43, precision)
    u["w1"] = u["w1"].copy()
    u["w1"][:, 43] = pk.bf16(pk.SCALE * params[0][:, 0])            # (a column of the size of a real one)
    right = wref.packed_from(u, wref.inputs(rows, 43), precision, 26, act32)
    wrong = wref.packed_from(u, wref.inputs(rows, 43, "byte_obs"), precision, 26, act32)
    assert np.array_equal(right, q)                                 # the right kernel masks the byte: the column does not matter
    assert np.abs(wrong - q).max() > 10 * bound
    c47 = _small_case((47, 26))
    assert wide.columns(47) - 1 == 47
    wrong47 = wref.packed(c47["params"], c47["pool"], precision, wrong="byte_obs", act32=act32)
    bound47 = ref.M_FP32 * c47["F"] if precision == "fp32" else ref.EMU_BF16["max"]
    assert np.abs(wrong47 - c47["Q"][ref.Q_KEY[precision]]).max() > 10 * bound47


# ---------------------------------------------------------------- the sweep: every (MKS, KS) pair and the padding k-steps
def test_kernel_ksteps_is_the_launchers_choice():
    assert [wref.kernel_ksteps(d) for d in (32, 47, 48, 79, 80, 91, 151, 163)] == [5, 5, 5, 5, 11, 11, 11, 11]
    assert [wide.ksteps(d) for d in (79, 80)] == [5, 6]             # the switch lies between 79 and 80 inputs
    with pytest.raises(AssertionError):
        wref.kernel_ksteps(31)                                      # (a narrow net: neither instantiation)


def test_sweep_widths_hold_every_pair_and_every_edge():
    obs = wref.SWEEP_OBS
    assert set(19 + 12 * n for n in range(2, 13)) <= set(obs) and all(32 <= d <= wide.MAX_OBS for d in obs) and len(set(obs)) == len(obs)
    pairs = {(wref.kernel_ksteps(d), wide.ksteps(d)) for d in obs}
    assert pairs == {(5, 3), (5, 4), (5, 5)} | {(11, k) for k in range(6, 12)}
    assert pairs == {(wref.kernel_ksteps(d), wide.ksteps(d)) for d in range(32, wide.MAX_OBS + 1)}    # ... which is every pair there is
    for mks in (5, 11):
        mine = [d for d in obs if wref.kernel_ksteps(d) == mks]
        assert any(d % 16 == 0 for d in mine), mks                  # the last k-step holds the bias column and no feature
        assert any(d % 16 == 15 for d in mine), mks                 # byte obs_dim of the record is the bias column
    assert {d for d in range(48, 161, 16)} <= set(obs)              # every multiple of 16 a wide net can have (32 as well)
    assert 32 in obs and {79, 80} <= set(obs)
    assert set(wref.ONE_PER_KS) == set(range(3, 12)) and all(wide.ksteps(d) == k and d in obs for k, d in wref.ONE_PER_KS.items())
    assert all(wide.ksteps(d) < wref.kernel_ksteps(d) for k, d in wref.ONE_PER_KS.items() if k not in (5, 11))
    for d in obs:                                                   # a record holds the padding k-step's "next piece"
        assert wref.engine_record_bytes(d) >= 16 * (wide.ksteps(d) + 1)


def _rejected(case, precision, wrong, mks=None):
    got = wref.packed(case["params"], case["pool"], precision, wrong=wrong, act32=precision == "fp32", mks=mks).astype(np.float32)
    return ref.check_forward(got, case, precision), _figures(got, case, precision)


@pytest.mark.parametrize("obs_dim", wref.SWEEP_OBS)
def test_check_forward_sees_a_wrong_padding_wherever_there_is_a_padding_step(obs_dim):
    """26 outputs, both precisions.  KS < MKS: the three wrong paddings are rejected.  KS == MKS (64, 67, 79; 160, 162, 163): there is
    no padding step, all three ARE the right kernel and are accepted - the blind spot of the forward shapes 67 and 163, written down.
    The three older wrong kernels are rejected where they differ from the right one: "first32" above 32 inputs, "bias31" everywhere,
    "byte_obs" where byte obs_dim is column K - 1 (16 k - 1 inputs)."""
    case = _small_case((obs_dim, 26))
    KS, mks = wide.ksteps(obs_dim), wref.kernel_ksteps(obs_dim)
    for precision in ("fp32", "bf16"):
        bound = ref.M_FP32 * case["F"] if precision == "fp32" else ref.EMU_BF16["max"]
        assert ref.check_forward(case["Q"][ref.Q_KEY[precision]].astype(np.float32), case, precision) == []
        for wrong in wref.PADDING_WRONG:
            fails, d = _rejected(case, precision, wrong, mks)
            print("%d KS %d MKS %d %s %s: max |wrong - Q| %.3e bound %.3e" % (obs_dim, KS, mks, wrong, precision, d, bound))
            if KS < mks:
                assert fails != [] and d > bound, (wrong, precision, d, bound)
            else:
                assert fails == [] and d <= 2.0 ** -23 * np.abs(case["Q"][ref.Q_KEY[precision]]).max(), (wrong, precision, d)
        older = ["bias31"] + (["first32"] if obs_dim > 32 else []) + (["byte_obs"] if obs_dim % 16 == 15 else [])
        for wrong in older:
            fails, d = _rejected(case, precision, wrong)
            assert fails != [] and d > bound, (wrong, precision, d, bound)
        if obs_dim == 32:                                           # no feature beyond the 32nd: "first32" is the right kernel
            assert _rejected(case, precision, "first32")[0] == []


def test_a_padding_step_reads_zeros_beyond_the_record():
    rows = wref.wide_records(64, 32, np.random.default_rng(1), pool=8)          # 4 pieces, KS = 3, MKS = 5: piece 3 exists, piece 4 does not
    pad = wref.padding_inputs(rows, 32, "next_piece", 5)
    assert pad.shape == (8, 32) and np.array_equal(pad[:, :16], rows[:, 48:64].view(np.int8)) and not pad[:, 16:].any()
    one = wref.padding_inputs(rows, 32, "one_again", 5)
    assert np.array_equal(np.flatnonzero(one[0]), [15, 31]) and (one[:, [15, 31]] == 1).all()
    assert np.array_equal(wref.padding_inputs(rows, 32, "unmasked", 5), np.tile(rows[:, 32:48].view(np.int8), (1, 2)))


# ---------------------------------------------------------------- brink boards under the random policy: the ends the GPU rollouts need
@pytest.mark.parametrize("N,indirect", wref.BRINK_CASES, ids=["N%d_%s" % (n, "ind" if i else "dir") for n, i in wref.BRINK_CASES])
def test_brink_boards_end_inside_the_rollout_under_the_random_policy(N, indirect):
    """tests/test_gpu_net_wide.py injects board_inject.brink_only into every game and asks that a quarter of the games end inside
    BRINK_T iterations of a freshly initialised net - close to uniform over the legal actions.  The oracle alone under its random
    admissible policy reaches at least twice that share, so the GPU condition has room."""
    from oracle import skyjo_oracle as so
    from tests import board_inject as bi, pile_inject as pi

    B, T = wref.BRINK_GAMES, wref.BRINK_T
    ora = so.OracleVec(num_envs=B, **pi.oracle_config(N, pi.MT, indirect))
    ora.seed(None, wref.BRINK_SEED)
    pi.inject(bi.brink_only, np.random.default_rng(wref.BRINK_SEED), ora)
    ended = np.zeros(B, dtype=bool)
    for _ in range(T):
        ora.rollout(1, pi.POLICY_SEED)
        ended |= ora.dones.astype(bool)
    print("brink N=%d %s: %d of %d games end inside %d iterations, %d episode ends" % (N, "indirect" if indirect else "direct", int(ended.sum()), B, T, ora.counters()["episodes"]))
    assert int(ended.sum()) >= 2 * wref.BRINK_SHARE * B
