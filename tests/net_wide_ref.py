"""tests/net_ref.py's two references of the forward pass for nets wider than 31 inputs (``k_net_bf16_wide`` / ``k_net_split_wide``,
csrc/skyjo_policy.hip), on pools of synthetic records of the same kind: X = ``net_ref.exact``, Q = ``packed`` - the documented arithmetic
of the packed net in float64 from ``mlp_pack_wide_ref.unpack(mlp_pack_wide_ref.pack(...))``, layer 1 over K = 16 KS columns instead of 32.
A case has net_ref's keys, so ``net_ref.check_forward`` and ``net_ref.forward_figures`` take it; T1 (the project's 1e-4 / 8e-2 against X)
was measured at 31 inputs and is not asserted on a wide case (t1 is False).  numpy only, nothing from the package.  Not collected: a
helper; tests/test_net_wide_ref.py shows without a GPU that the checks reject three restated wrong kernels and, wherever a kernel runs a
padding k-step (KS < MKS: ``kernel_ksteps``, ``SWEEP_OBS``), three restated wrong paddings.

Every byte of a record from obs_dim on is random - the action byte, the pad, the mask, the rest; pool rows 1 - 4 are the all-low,
all-high and alternating rows."""
import functools

import numpy as np

from tests import mlp_pack_ref as pk, mlp_pack_wide_ref as wide, net_ref as ref

POOL = ref.POOL
WRONG = ("first32", "bias31", "byte_obs")
# Wrong PADDING k-steps (a kernel compiled for MKS k-steps runs MKS - KS of them against k-step KS - 1's loads, and they must add
# nothing): "one_again" - the constant 1 enters in every step from KS - 1 on, so b1 is added MKS - KS times more; "unmasked" - the
# repeated record piece KS - 1 enters with all of its 16 bytes; "next_piece" - a padding step s reads record piece s and lets it in.
# All three take the kernel's MKS and are the right kernel where KS == MKS.
PADDING_WRONG = ("one_again", "unmasked", "next_piece")
# (obs_dim, out_dim) of the GPU forward cases: the direct observation of 2, 4 and 12 players, and 47 - K = 48: the bias column IS byte
# obs_dim of the record, so a kernel that lets that byte in is seen there through a non-zero weight
FORWARD_SHAPES = ((43, 26), (67, 26), (67, 1), (163, 26), (47, 26))
GAME_RANGE = (-2, 15)
# The widths of the forward sweep: the direct observation of 2 .. 12 players (19 + 12 N) and the edges - 32 (the first wide net), the
# multiples of 16 (the last k-step holds the bias column and no feature), 16 k - 1 (byte obs_dim of the record is the bias column),
# both sides of the switch between the two instantiations (79 / 80), 162 and 163 (KS = MKS = 11).
SWEEP_OBS = tuple(sorted({19 + 12 * n for n in range(2, 13)} | {32, 33, 48, 63, 64, 79, 80, 81, 95, 96, 112, 128, 144, 159, 160, 162}))
# one width per KS 3 .. 11 with a padding k-step wherever there is one (KS 5 and 11 are the instantiations' own sizes)
ONE_PER_KS = {3: 43, 4: 55, 5: 67, 6: 91, 7: 103, 8: 115, 9: 139, 10: 151, 11: 163}
# brink-board model rollouts (tests/test_gpu_net_wide.py): (players, indirect observation); games, iterations, the share of games that
# must end inside the iterations under a net, and under the oracle's own random policy (tests/test_net_wide_ref.py)
BRINK_CASES = ((2, False), (5, False), (12, False), (5, True))
BRINK_GAMES, BRINK_T, BRINK_SEED = 130, 24, 33
BRINK_SHARE = 0.25


def kernel_ksteps(obs_dim):
    """MKS of the instantiation sk_launch_mlp starts for a wide net (csrc/skyjo_policy.hip): 5 up to KS = 5, else 11."""
    assert obs_dim > 31
    return 5 if wide.ksteps(obs_dim) <= 5 else 11


def engine_record_bytes(obs_dim):
    """rec_bytes of the engine for an observation of obs_dim bytes (include/skyjo_vec.h): 80, 112, 208 at 43, 67, 163."""
    return (((obs_dim + 3) & ~3) + 32 + 15) & ~15


def wide_records(record_bytes, obs_dim, rng, pool=POOL, feature_range=(-128, 127)):
    """Pool rows uint8 [pool, record_bytes] as net_ref.net_records makes them, for any obs_dim."""
    lo, hi = feature_range
    assert -128 <= lo < hi <= 127 and record_bytes % 16 == 0 and record_bytes >= wide.columns(obs_dim) and pool >= 5
    rows = rng.integers(0, 256, size=(pool, record_bytes), dtype=np.uint8)
    feat = rng.integers(lo, hi + 1, size=(pool, obs_dim)).astype(np.int8)
    edges = np.array([lo, hi], dtype=np.int8)
    feat[1], feat[2] = lo, hi
    feat[3], feat[4] = edges[np.arange(obs_dim) % 2], edges[(np.arange(obs_dim) + 1) % 2]
    rows[:, :obs_dim] = feat.view(np.uint8)
    assert np.unique(rows[:, :obs_dim], axis=0).shape[0] == pool, "pool observations repeat"
    return rows


def padding_inputs(rows, obs_dim, wrong, mks):
    """The input columns float64 [n, 16 (mks - KS)] of the padding k-steps KS .. mks - 1 of a wrong kernel (the right one: zeros).  A
    record piece that lies beyond the record's end enters as zeros."""
    assert wrong in PADDING_WRONG and mks in (5, 11) and wide.ksteps(obs_dim) <= mks
    KS = wide.ksteps(obs_dim)
    n, pieces = rows.shape[0], rows.shape[1] // 16
    pad = np.zeros((n, mks - KS, 16), dtype=np.float64)
    for i, s in enumerate(range(KS, mks)):
        if wrong == "one_again":
            pad[:, i, 15] = 1.0
        elif wrong == "unmasked":
            pad[:, i] = rows[:, 16 * (KS - 1):16 * KS].view(np.int8)
        elif s < pieces:
            pad[:, i] = rows[:, 16 * s:16 * s + 16].view(np.int8)
    return pad.reshape(n, 16 * (mks - KS))


def padded_tables(u, obs_dim, mks):
    """The unpacked tables with layer 1 as a kernel of mks k-steps reads it: k-step KS - 1's columns again for every padding step."""
    KS = wide.ksteps(obs_dim)
    out = dict(u)
    for k in ("w1", "w1l"):
        if k in u:
            out[k] = np.concatenate([u[k]] + [u[k][:, 16 * (KS - 1):16 * KS]] * (mks - KS), axis=1)
    return out


def inputs(rows, obs_dim, wrong=None):
    """Layer 1's input columns float64 [n, K] of record rows: the features, zeros, the constant 1 in column K - 1.  ``wrong`` restates a
    wrong kernel: "first32" sees only the first 32 features; "bias31" has the constant 1 in column 31 (the narrow kernels' place);
    "byte_obs" lets byte obs_dim of the record in as a feature."""
    assert wrong in (None,) + WRONG
    K = wide.columns(obs_dim)
    x = np.zeros((rows.shape[0], K), dtype=np.float64)
    x[:, :obs_dim] = rows[:, :obs_dim].view(np.int8)
    x[:, K - 1] = 1.0
    if wrong == "first32":
        x[:, 32:K - 1] = 0.0
    elif wrong == "bias31":
        x[:, K - 1], x[:, 31] = 0.0, 1.0
    elif wrong == "byte_obs":
        x[:, obs_dim] = rows[:, obs_dim].view(np.int8)
    return x


def packed_from(u, xk, precision, out_dim, act32=False):
    """Q from unpacked tables (mlp_pack_wide_ref.unpack) and layer 1's input columns: net_ref.packed's arithmetic."""
    val, pair = ref._val, ref._pair
    b2h, b2l = pair(u["b2"])
    b3h, b3l = pair(u["b3"])
    if precision == "fp32":
        def split(h):
            h = h.astype(np.float32)
            return val(pk.bf16(h)), val(pk.bf16_lo(h))

        def act(y):
            if not act32:
                return 1.0 - 2.0 / (ref._exp2(y) + 1.0)
            f = np.float32
            with np.errstate(over="ignore", under="ignore"):
                e = ref._exp2(y).astype(f)
                r = (1.0 / (e + f(1.0)).astype(f).astype(np.float64)).astype(f)
            return (f(1.0) - f(2.0) * r).astype(np.float64)

        def prod(hh, hl, wh, wl):
            return hh @ wh.T + hl @ wh.T + hh @ wl.T

        h1h, h1l = split(act(xk @ (val(u["w1"]) + val(u["w1l"])).T))
        h2h, h2l = split(act(prod(h1h, h1l, val(u["w2"]), val(u["w2l"])) + b2h + b2l))
        out = prod(h2h, h2l, val(u["w3"]), val(u["w3l"])) + b3h + b3l
    else:
        def r(y):
            return val(pk.bf16((1.0 / (ref._exp2(y) + 1.0)).astype(np.float32)))

        r1 = r(xk @ val(u["w1"]).T)
        r2 = r(r1 @ val(u["w2"]).T + b2h + b2l)
        out = r2 @ val(u["w3"]).T + b3h + b3l
    return out[:, :out_dim]


def packed(params, rows, precision, wrong=None, act32=False, mks=None):
    """Q of record rows: float64 [n, out_dim].  A wrong padding (PADDING_WRONG) takes ``mks``, the k-steps the kernel is compiled for."""
    obs_dim, out_dim = np.shape(params[0])[1], np.shape(params[4])[0]
    u = wide.unpack(wide.pack(*params, precision=precision), obs_dim, precision)
    if wrong in PADDING_WRONG:
        xk = np.concatenate([inputs(rows, obs_dim), padding_inputs(rows, obs_dim, wrong, mks)], axis=1)
        return packed_from(padded_tables(u, obs_dim, mks), xk, precision, out_dim, act32)
    return packed_from(u, inputs(rows, obs_dim, wrong), precision, out_dim, act32)


@functools.lru_cache(maxsize=None)
def forward_case(shape, wset, record_bytes=None, feature_range=(-128, 127), seed=0):
    """One pool and its references, computed once and shared (do not write to it): net_ref.forward_case's dict."""
    shape = tuple(shape)
    record_bytes = record_bytes or engine_record_bytes(shape[0])
    rng = np.random.default_rng(19000 + 1000 * shape[0] + record_bytes + 7 * seed + ((feature_range[1] & 255) << 16))
    rows = wide_records(record_bytes, shape[0], rng, feature_range=feature_range)
    params = ref.weights(shape, wset)
    x = rows[:, :shape[0]].view(np.int8).astype(np.float64)
    X = ref.exact(params, x)
    case = dict(shape=shape, wset=wset, record_bytes=record_bytes, feature_range=tuple(feature_range), params=params, pool=rows, x=x, X=X,
                Q={"fp32": packed(params, rows, "fp32"), "bf16": packed(params, rows, "bf16"), "fp32-act32": packed(params, rows, "fp32", act32=True)},
                F=float(np.abs(ref.float32_module(params, x) - X).max()), t1=False)
    for v in (rows, x, X) + tuple(case["Q"].values()):
        v.setflags(write=False)
    return case


def case_records(case, n):
    return np.ascontiguousarray(case["pool"][np.arange(n) % POOL])
