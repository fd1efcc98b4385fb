"""float64 references for the inference hot path - the packed net (``k_net_split`` / ``k_net_bf16``, csrc/skyjo_policy.hip) and the
masked categorical draw (``k_sample``, csrc/skyjo_callers.h; the two draw forms of csrc/skyjo_draw.h) - and synthetic records, masks and
logits that no game produces.  numpy only, nothing from the package, deterministic from seeds (TEST INFRASTRUCTURE).  Written from the
documents (include/skyjo_vec.h: skyjo_vec_sample_actions, "The packed layout"); it shares no code with the library.
tests/test_net_ref.py asserts without a GPU that the references are what they claim and that the checks reject restated wrong kernels;
tests/test_gpu_net_synthetic.py feeds the same cases to the kernels and calls the same checks.  Not collected: a helper.

Two references of the forward pass:
  X = ``exact``: Linear - tanh - Linear - tanh - Linear in float64 on the unrounded float32 parameters;
  Q = ``packed``: the documented arithmetic of the packed net in float64, from ``mlp_pack_ref.unpack(mlp_pack_ref.pack(...))``.
      Only the roundings the definition names are made (the weights' and biases' bf16 halves, the activations' split into bf16
      halves through float32); every sum is float64.  What separates a correct kernel from Q is float32 accumulation and the
      hardware's exp2 / rcp.
"""
import functools

import numpy as np

from tests import learner_synth, mlp_pack_ref as pk, mlp_train_ref

H = 256
SHAPES = pk.SHAPES
FLOAT_MIN = np.float32(np.finfo(np.float32).min)
M32 = 0xFFFFFFFF

# The project's tolerances against the float32 module (tests/test_gpu_policy_net.py: TOL) and against the bf16 emulation.
TOL = {"fp32": dict(max=1e-4, mean=2e-5), "bf16": dict(max=8e-2, mean=1e-2)}
EMU_BF16 = dict(max=2e-2, mean=2e-3)
T1_RANGE = (-32, 31)          # the feature range at which the project measured 4 x TOL (test_net_on_caller_records_of_other_shapes)
T1_SETS = ("A", "B")

# T2 of the float32-grade mode: max |kernel - Q| <= M_FP32 * F, F = max |float32 torch module on the CPU - X| on the case's pool.
# M_FP32 is the smallest power of two at least twice the largest ratio max |kernel - Q| / F seen on an MI355X over every case of
# tests/test_gpu_net_synthetic.py (the factor two: the accumulation order differs between launch shapes).  RATIOS_SEEN: the largest
# ratio per group of cases in that run, against the Q the check uses and (second figure) against the Q whose activation is evaluated in
# float64; EXPERIMENTS.md has the entry.
#   With the float64 activation the largest ratio was 32.1 (set Z) and M would be 128: 128 F is more than a quarter of T1's bound.  The
#   missing term: the kernel evaluates 1 - 2 / (2^y + 1) in four float32 instructions, whose roundings (2^y + 1 above all: half an ulp of
#   2) are an ABSOLUTE error of about 2^-23 on h whatever its size, where torch's tanh - and so F - is relatively accurate near 0.  With
#   those four roundings made (exactly rounded operations: "fp32-act32") set Z's ratio halves; what is left is the hardware's 2^y and
#   reciprocal, 1 ulp each, which no document pins down.  M = 64, and 64 F was at most 6.6e-5 on the cases T1 covers (F_T1_SEEN),
#   against a quarter of T1's 4e-4.  F is torch's float32 matmul on the host CPU and differs between CPUs by up to a factor 2 (the
#   figures are the MI355X host's).
M_FP32 = 64.0
RATIOS_SEEN = {"rows-one-net": (4.329, 4.849), "rows-two-nets": (4.672, 4.849), "shapes": (4.329, 4.849), "set-A-small": (3.974, 4.126),
               "set-A-int8": (3.101, 2.912), "set-B-small": (4.329, 4.849), "set-B-int8": (1.214, 1.324), "set-S-small": (2.225, 1.933),
               "set-S-int8": (0.872, 0.825), "set-Z-small": (16.257, 30.080), "set-Z-int8": (17.022, 32.109)}
F_T1_SEEN = 1.017e-6          # the largest F of a case T1 covers, in that run
# Which Q a mode is held to: "fp32-act32" makes the four float32 roundings of the activation, "fp32" evaluates it in float64.
Q_KEY = {"fp32": "fp32-act32", "bf16": "bf16"}

WEIGHT_SETS = ("A", "B", "S", "Z")
POOL = 4099                   # prime: a row read from the wrong lane, wave, batch or pass meets a different pool row


# ---------------------------------------------------------------- weights
@functools.lru_cache(maxsize=None)
def weights(shape, wset):
    """(w1, b1, w2, b2, w3, b3) float32.  A: torch's default initialisation under a seed (``mlp_train_ref.weights``); B: A x 1.5, what
    tests/test_gpu_policy_net.py uses; S: w1 of A x 8 (``mlp_train_ref.SATURATE``): most of layer 1 saturates; Z: layers 1 and 2 of A
    x 1e-3 - weights AND biases, or tanh(b1) alone reaches 0.18 - so that both hidden layers stay near 0, where 1 - 2 r cancels."""
    assert wset in WEIGHT_SETS
    p = [np.array(t, dtype=np.float32) for t in mlp_train_ref.weights(tuple(shape), "S" if wset == "S" else "A")]
    if wset == "B":
        p = [(t * np.float32(1.5)).astype(np.float32) for t in p]
    if wset == "Z":
        p[:4] = [(t * np.float32(1e-3)).astype(np.float32) for t in p[:4]]
    for t in p:
        t.setflags(write=False)
    return tuple(p)


def steered(kind):
    """Set A (31 -> 26) with a last layer that steers the pair draw: "ties" - every logit 1.25; "ramp" - the logits 0 .. -120 descending
    in k, whatever the observation; "sharp" - w3 x 60, logits far apart.  A list of six float32 arrays."""
    p = [np.array(t) for t in weights((31, 26), "A")]
    if kind == "ties":
        p[4], p[5] = np.zeros_like(p[4]), np.full_like(p[5], 1.25)
    elif kind == "ramp":
        p[4], p[5] = np.zeros_like(p[4]), np.linspace(0.0, -120.0, 26).astype(np.float32)
    else:
        assert kind == "sharp"
        p[4] = (p[4] * np.float32(60.0)).astype(np.float32)
    return p


# ---------------------------------------------------------------- forward references
def exact(params, x):
    """X: float64 [n, out_dim]."""
    w1, b1, w2, b2, w3, b3 = (np.asarray(p, dtype=np.float64) for p in params)
    h1 = np.tanh(np.asarray(x, dtype=np.float64) @ w1.T + b1)
    return np.tanh(h1 @ w2.T + b2) @ w3.T + b3


def layer1_tanh(params, x):
    w1, b1 = (np.asarray(p, dtype=np.float64) for p in params[:2])
    return np.tanh(np.asarray(x, dtype=np.float64) @ w1.T + b1)


def float32_module(params, x):
    """The float32 torch module on the CPU, one thread (the same sums everywhere): float64 [n, out_dim]."""
    import torch

    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        p = [torch.from_numpy(np.array(t, dtype=np.float32)) for t in params]
        h = torch.from_numpy(np.array(x, dtype=np.float32))
        h = torch.tanh(torch.nn.functional.linear(h, p[0], p[1]))
        h = torch.tanh(torch.nn.functional.linear(h, p[2], p[3]))
        return torch.nn.functional.linear(h, p[4], p[5]).double().numpy()
    finally:
        torch.set_num_threads(threads)


def _val(h):
    return pk.bf16_value(h).astype(np.float64)


def _pair(b):
    """A float32 bias as the kernels carry it: the sum of two bf16 values (hi = bf16(b), lo = bf16(b - hi): skp_bias_split)."""
    b = np.ascontiguousarray(b, dtype=np.float32)
    return _val(pk.bf16(b)), _val(pk.bf16_lo(b))


def _exp2(y):
    with np.errstate(over="ignore", under="ignore"):
        return np.exp2(y)


def packed(params, x, precision, wrong=None, act32=False):
    """Q: float64 [n, out_dim].  x: integer-valued features [n, obs_dim] (what an int8 record holds).  ``wrong`` restates a wrong kernel
    for tests/test_net_ref.py: "w_lo_h_hi" leaves that term out of layer 2, "b2_lo" the low half of layer 2's bias."""
    assert precision in ("fp32", "bf16") and wrong in (None, "w_lo_h_hi", "b2_lo")
    u = pk.unpack(pk.pack(*params, precision=precision), precision)
    obs_dim, out_dim = np.shape(params[0])[1], np.shape(params[4])[0]
    x = np.asarray(x, dtype=np.float64)
    assert x.shape[1] == obs_dim and np.array_equal(x, np.round(x)) and np.abs(x).max() <= 128
    x32 = np.zeros((x.shape[0], pk.IN), dtype=np.float64)
    x32[:, :obs_dim] = x
    x32[:, pk.IN - 1] = 1.0                                   # layer 1's bias rides in column 31
    b2h, b2l = _pair(u["b2"])
    b3h, b3l = _pair(u["b3"])
    if wrong == "b2_lo":
        b2l = 0.0 * b2l
    if precision == "fp32":
        def split(h):                                         # an activated value as hi + lo, rounded through float32
            h = h.astype(np.float32)
            return _val(pk.bf16(h)), _val(pk.bf16_lo(h))

        def act(y):
            if not act32:
                return 1.0 - 2.0 / (_exp2(y) + 1.0)
            f = np.float32                                    # the four float32 instructions, each rounded once (ACT32 above)
            with np.errstate(over="ignore", under="ignore"):
                e = _exp2(y).astype(f)
                r = (1.0 / (e + f(1.0)).astype(f).astype(np.float64)).astype(f)
            return (f(1.0) - f(2.0) * r).astype(np.float64)   # (exact: 2 r is a float32 in [0, 2])

        def prod(hh, hl, wh, wl, drop=False):                 # w_hi h_hi + w_hi h_lo + w_lo h_hi (w_lo h_lo is left out)
            return hh @ wh.T + hl @ wh.T + (0.0 if drop else hh @ wl.T)

        h1h, h1l = split(act(x32 @ (_val(u["w1"]) + _val(u["w1l"])).T))     # (the inputs are exact in one bf16)
        h2h, h2l = split(act(prod(h1h, h1l, _val(u["w2"]), _val(u["w2l"]), wrong == "w_lo_h_hi") + b2h + b2l))
        out = prod(h2h, h2l, _val(u["w3"]), _val(u["w3l"])) + b3h + b3l
    else:
        def r(y):                                             # r = 1 / (2^y + 1) = (1 - tanh) / 2, rounded to bf16
            return _val(pk.bf16((1.0 / (_exp2(y) + 1.0)).astype(np.float32)))

        r1 = r(x32 @ _val(u["w1"]).T)
        r2 = r(r1 @ _val(u["w2"]).T + b2h + b2l)              # the blob holds - 2 W and b + W 1 already
        out = r2 @ _val(u["w3"]).T + b3h + b3l
    return out[:, :out_dim]


# ---------------------------------------------------------------- records
def net_records(n, record_bytes, obs_dim, rng, pool=POOL, feature_range=(-128, 127)):
    """(records uint8 [n, record_bytes], pool rows uint8 [pool, record_bytes]): ``pool`` distinct random rows, every byte random, the
    first obs_dim bytes int8 values in ``feature_range``; pool rows 1, 2 are all low / all high and rows 3, 4 alternate low / high and
    high / low (with the full range: learner_synth.OBS_EDGES).  Row g of the buffer is pool row g % pool."""
    lo, hi = feature_range
    assert -128 <= lo < hi <= 127 and record_bytes >= 32 and record_bytes % 16 == 0 and 1 <= obs_dim <= 31 and pool >= 5
    if (lo, hi) == (-128, 127):
        assert tuple(np.array(learner_synth.OBS_EDGES, dtype=np.uint8).view(np.int8)) == (lo, hi)
    rows = rng.integers(0, 256, size=(pool, record_bytes), dtype=np.uint8)
    feat = rng.integers(lo, hi + 1, size=(pool, obs_dim)).astype(np.int8)
    edges = np.array([lo, hi], dtype=np.int8)
    feat[1], feat[2] = lo, hi
    feat[3], feat[4] = edges[np.arange(obs_dim) % 2], edges[(np.arange(obs_dim) + 1) % 2]
    rows[:, :obs_dim] = feat.view(np.uint8)
    assert np.unique(rows, axis=0).shape[0] == pool, "pool rows repeat"
    if obs_dim > 2:                                           # (one or two features cannot give 4099 different observations)
        assert np.unique(rows[:, :obs_dim], axis=0).shape[0] == pool, "pool observations repeat"
    return np.ascontiguousarray(rows[np.arange(n) % pool]), rows


def features(pool_rows, obs_dim):
    return pool_rows[:, :obs_dim].view(np.int8).astype(np.float64)


def to_planar(rows, rng):
    """[n, record_bytes] -> tile-planar [tiles, P, 64, 16] with non-zero bytes in the padding of a partial last tile."""
    return learner_synth.to_planar_dirty(rows[None], rng)[0]


@functools.lru_cache(maxsize=None)
def forward_case(shape, wset, record_bytes=64, feature_range=(-128, 127), seed=0):
    """One pool and its references, computed once and shared (do not write to it): dict with params, pool (rows), x, X, Q = {precision:
    ...}, F, t1 (whether the project's numbers apply)."""
    shape = tuple(shape)
    # (the pool depends on the observation size, not on the outputs: a policy and a value net of one launch share it)
    rng = np.random.default_rng(9000 + 1000 * shape[0] + record_bytes + 7 * seed + (feature_range[1] << 16))
    _, rows = net_records(1, record_bytes, shape[0], rng, feature_range=feature_range)
    params = weights(shape, wset)
    x = features(rows, shape[0])
    X = exact(params, x)
    case = dict(shape=shape, wset=wset, record_bytes=record_bytes, feature_range=tuple(feature_range), params=params, pool=rows, x=x, X=X,
                Q={"fp32": packed(params, x, "fp32"), "bf16": packed(params, x, "bf16"), "fp32-act32": packed(params, x, "fp32", act32=True)}, F=float(np.abs(float32_module(params, x) - X).max()),
                t1=wset in T1_SETS and feature_range[0] >= T1_RANGE[0] and feature_range[1] <= T1_RANGE[1])
    for v in (rows, x, X) + tuple(case["Q"].values()):
        v.setflags(write=False)
    return case


def case_records(case, n):
    """Row-major records uint8 [n, record_bytes] of the case: row g is pool row g % POOL."""
    return np.ascontiguousarray(case["pool"][np.arange(n) % POOL])


def _cyclic_diff(got, ref):
    """|got[g] - ref[g % pool]| as float64 [n, out] without an index array of n rows."""
    got = np.asarray(got, dtype=np.float64)
    n, pool = got.shape[0], ref.shape[0]
    whole = n // pool
    d = np.empty_like(got)
    if whole:
        d[:whole * pool] = np.abs(got[:whole * pool].reshape(whole, pool, -1) - ref[None]).reshape(whole * pool, -1)
    d[whole * pool:] = np.abs(got[whole * pool:] - ref[:n - whole * pool])
    return d


def forward_figures(got, case, precision):
    """max / mean |got - X|, max / mean |got - Q|, F and the ratio max |got - Q| / F."""
    dx, dq = _cyclic_diff(got, case["X"]), _cyclic_diff(got, case["Q"][Q_KEY[precision]])
    return dict(max_x=float(dx.max()), mean_x=float(dx.mean()), max_q=float(dq.max()), mean_q=float(dq.mean()), F=case["F"],
                ratio=float(dq.max()) / case["F"])


def check_forward(got, case, precision, m_fp32="default"):
    """The failures (a list of strings, empty = pass) of outputs float32 [n, out_dim] whose row g was computed from pool row g % POOL:
    T1 against X where the project measured its numbers (4 x TOL: features in [-32, 31], sets A and B), T2 against Q everywhere
    ("bf16": the project's emulation bound; "fp32": M_FP32 x F)."""
    got = np.asarray(got)
    fails = []
    if got.ndim != 2 or got.shape[1] != case["shape"][1] or got.dtype != np.float32:
        return ["shape / dtype %s %s" % (got.shape, got.dtype)]
    if not np.isfinite(got).all():
        return ["%d non-finite outputs, first at row %d" % (int((~np.isfinite(got)).sum()), int(np.argwhere(~np.isfinite(got))[0, 0]))]
    f = forward_figures(got, case, precision)
    m = M_FP32 if m_fp32 == "default" else m_fp32
    if case["t1"]:
        t = TOL[precision]
        if not (f["max_x"] <= 4 * t["max"] and f["mean_x"] <= 4 * t["mean"]):
            fails.append("T1: |got - X| max %.3e mean %.3e against %.1e / %.1e" % (f["max_x"], f["mean_x"], 4 * t["max"], 4 * t["mean"]))
    if precision == "bf16":
        if not (f["max_q"] < EMU_BF16["max"] and f["mean_q"] < EMU_BF16["mean"]):
            fails.append("T2: |got - Q| max %.3e mean %.3e against %.1e / %.1e" % (f["max_q"], f["mean_q"], EMU_BF16["max"], EMU_BF16["mean"]))
    elif m is not None:
        if not f["max_q"] <= m * case["F"]:
            row = int(np.argmax(_cyclic_diff(got, case["Q"][Q_KEY[precision]]).max(axis=1)))
            fails.append("T2: |got - Q| max %.3e (row %d) against %g x F = %.3e" % (f["max_q"], row, m, m * case["F"]))
    return fails


# ---------------------------------------------------------------- Philox and the uniform
def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., SC'11; Random123): counter uint32 [..., 4], key uint32 [..., 2] -> uint32 [..., 4]."""
    c = [np.asarray(counter, dtype=np.uint32)[..., i].astype(np.uint64) for i in range(4)]
    k = [np.asarray(key, dtype=np.uint32)[..., i].astype(np.uint64) for i in range(2)]
    m0, m1, w0, w1, M = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85), np.uint64(M32)
    s = np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]                         # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> s) ^ c[1] ^ k[0], p1 & M, (p0 >> s) ^ c[3] ^ k[1], p0 & M]
        k = [(k[0] + w0) & M, (k[1] + w1) & M]
    return np.stack(np.broadcast_arrays(*c), axis=-1).astype(np.uint32)


def draw_counter(ticket, gid):
    """uint32 [n, 4]: (ticket & M, ticket >> 32, gid & M, 0x53414D50 ^ (gid >> 32)) for gid uint64 [n]."""
    gid = np.asarray(gid, dtype=np.uint64)
    ticket = int(ticket) & (2 ** 64 - 1)
    c = np.empty(gid.shape + (4,), dtype=np.uint32)
    c[..., 0], c[..., 1] = ticket & M32, ticket >> 32
    c[..., 2] = (gid & np.uint64(M32)).astype(np.uint32)
    c[..., 3] = np.uint32(0x53414D50) ^ (gid >> np.uint64(32)).astype(np.uint32)
    return c


def game_ids(game_id0, n):
    """game_id0 + i as a 64-bit sum (it wraps): uint64 [n]."""
    with np.errstate(over="ignore"):
        return np.uint64(int(game_id0) & (2 ** 64 - 1)) + np.arange(n, dtype=np.uint64)


def uniform(seed, ticket, gid, counter=draw_counter):
    """float32 [n]: (word 0 >> 8) * 2^-24 of Philox4x32-10 over the counter above, keyed by (seed & M, seed >> 32)."""
    seed = int(seed) & (2 ** 64 - 1)
    key = np.array([seed & M32, seed >> 32], dtype=np.uint32)
    w0 = philox4x32_10(counter(ticket, gid), key)[..., 0]
    return ((w0 >> np.uint32(8)).astype(np.float64) * 2.0 ** -24).astype(np.float32)


# ---------------------------------------------------------------- masks, logits, the draw
def _blocks(which):
    return [k for k in range(26) if which(k // 4)]


MASK_FAMILIES = ("ones", "zeros", "single", "draw-phase", "even-blocks", "odd-blocks", "heads", "no-heads", "random")
LOGIT_FAMILIES = ("normal", "equal", "ramp-down", "ramp-up", "spike", "offset", "masked-max")
AMBIGUOUS = 1e-5              # the number tests/test_gpu_sampler.py uses for a uniform next to a CDF step


def mask_rows(n, rng):
    """(mask uint8 [n, 26] of bytes 0 / 1, family index [n]): family g % 9; "single": action (g // 9) % 26 alone."""
    fam = np.arange(n) % len(MASK_FAMILIES)
    m = np.zeros((n, 26), dtype=np.uint8)
    fixed = {"ones": range(26), "zeros": [], "draw-phase": [24, 25], "even-blocks": _blocks(lambda j: j % 2 == 0),
             "odd-blocks": _blocks(lambda j: j % 2 == 1), "heads": range(0, 26, 4), "no-heads": [k for k in range(26) if k % 4]}
    for i, name in enumerate(MASK_FAMILIES):
        rows = np.flatnonzero(fam == i)
        if name in fixed:
            m[np.ix_(rows, list(fixed[name]))] = 1
        elif name == "single":
            m[rows, (rows // len(MASK_FAMILIES)) % 26] = 1
        else:
            m[rows] = rng.random((rows.size, 26)) < 0.5
    return m, fam


def logit_rows(n, mask, rng):
    """(logits float32 [n, 26], family index [n]): family g % 7 - normal x 3; all equal; a ramp 0 .. -120 descending / ascending in k;
    one action ((g // 7) % 26) at 0 and the rest at -17; normal x 3 + 1e4; normal x 3 with + 50 on a masked action (where there is one)."""
    fam = np.arange(n) % len(LOGIT_FAMILIES)
    lg = (rng.standard_normal((n, 26)) * 3.0).astype(np.float32)
    ramp = np.linspace(0.0, -120.0, 26).astype(np.float32)
    lg[fam == 1] = np.float32(1.25)
    lg[fam == 2] = ramp
    lg[fam == 3] = ramp[::-1]
    rows = np.flatnonzero(fam == 4)
    lg[rows] = np.float32(-17.0)
    lg[rows, (rows // len(LOGIT_FAMILIES)) % 26] = 0.0
    lg[fam == 5] += np.float32(1e4)
    for g in np.flatnonzero(fam == 6):
        off = np.flatnonzero(mask[g] == 0)
        if off.size:
            lg[g, off[(g // 63) % off.size]] = 50.0
    return lg, fam


def draw_reference(logits32, mask01, u, no_masking):
    """The definition in float64: masked = float32(logits + where(mask, 0, FLOAT_MIN)) - one float32 addition -, softmax and CDF in
    float64; the action is the smallest k of non-zero probability whose CDF value exceeds u, or the last k of non-zero probability.
    dict: action int [n], logp float64 [n, 26], p, cdf, ambiguous bool [n] (u within AMBIGUOUS of a CDF step of a non-zero-probability
    action)."""
    lg = np.asarray(logits32, dtype=np.float32)
    on = np.ones(lg.shape, dtype=bool) if no_masking else np.asarray(mask01) != 0
    with np.errstate(over="ignore"):
        masked = (lg + np.where(on, np.float32(0.0), FLOAT_MIN)).astype(np.float32).astype(np.float64)
    z = masked - masked.max(axis=1, keepdims=True)
    with np.errstate(under="ignore", divide="ignore"):
        e = np.exp(z)
        s = e.sum(axis=1, keepdims=True)
        p, logp = e / s, z - np.log(s)
    cdf = np.cumsum(p, axis=1)
    u64 = np.asarray(u, dtype=np.float64)[:, None]
    cand = (p > 0) & (cdf > u64)
    last = 25 - np.argmax((p > 0)[:, ::-1], axis=1)
    action = np.where(cand.any(axis=1), np.argmax(cand, axis=1), last)
    ambiguous = ((p > 0) & (np.abs(cdf - u64) <= AMBIGUOUS)).any(axis=1)
    return dict(action=action, logp=logp, p=p, cdf=cdf, ambiguous=ambiguous)


def draw_case(n, seed, ticket, game_id0=0, no_masking=False, rng_seed=0, record_bytes=64, mask_offset=32, obs_dim=31, u=None):
    """Family records (every other byte random), logits, the reference uniforms and the reference draw of one sample_actions call."""
    rng = np.random.default_rng(31000 + rng_seed)
    mask, mfam = mask_rows(n, rng)
    logits, lfam = logit_rows(n, mask, rng)
    rec = rng.integers(0, 256, size=(n, record_bytes), dtype=np.uint8)
    rec[:, mask_offset:mask_offset + 26] = mask
    want_u = uniform(seed, ticket, game_ids(game_id0, n)) if u is None else np.asarray(u, dtype=np.float32)
    case = dict(n=n, seed=seed, ticket=ticket, game_id0=game_id0, no_masking=no_masking, records=rec, mask=mask, mask_family=mfam,
                logits=logits, logit_family=lfam, u=want_u, obs_dim=obs_dim, mask_offset=mask_offset)
    case["ref"] = draw_reference(logits, mask, want_u, no_masking)
    return case


def with_logits(case, logits32):
    """The case with other logits (the pair draw: the ones the net's launch wrote) and its reference."""
    c = dict(case, logits=np.asarray(logits32, dtype=np.float32), logit_family=np.full(case["n"], -1))
    c["ref"] = draw_reference(c["logits"], c["mask"], c["u"], c["no_masking"])
    return c


def check_draw(actions, logp, uniform_out, case):
    """The failures of one draw: the uniforms (where given) bit for bit; every action of non-zero reference probability; the reference's
    action outside the ambiguous rows and, on those, an action whose CDF interval reaches within AMBIGUOUS of u (a neighbour of the step);
    logp (where given) within 1e-5 + 4 x 2^-24 |logp_ref| of the float64 value of the drawn action."""
    ref, n = case["ref"], case["n"]
    fails = []
    a = np.asarray(actions).astype(np.int64)
    if a.shape != (n,):
        return ["actions shape %s" % (a.shape,)]
    if uniform_out is not None:
        uo = np.asarray(uniform_out, dtype=np.float32)
        bad = np.flatnonzero(uo.view(np.uint32) != case["u"].view(np.uint32))
        if bad.size:
            fails.append("uniform: %d rows differ, first row %d: %r against %r" % (bad.size, bad[0], float(uo[bad[0]]), float(case["u"][bad[0]])))
    if ((a < 0) | (a > 25)).any():
        return fails + ["actions outside 0 .. 25: %d rows" % int(((a < 0) | (a > 25)).sum())]
    rows = np.arange(n)
    zero = np.flatnonzero(ref["p"][rows, a] <= 0)
    if zero.size:
        fails.append("an action of zero probability: %d rows, first row %d action %d (mask family %s)"
                     % (zero.size, zero[0], a[zero[0]], MASK_FAMILIES[case["mask_family"][zero[0]]]))
    clear = ~ref["ambiguous"]
    bad = np.flatnonzero(clear & (a != ref["action"]))
    if bad.size:
        fails.append("action: %d rows differ outside the ambiguous ones, first row %d: %d against %d (u = %r)"
                     % (bad.size, bad[0], a[bad[0]], ref["action"][bad[0]], float(case["u"][bad[0]])))
    u64 = case["u"].astype(np.float64)
    lo = np.where(a > 0, ref["cdf"][rows, np.maximum(a - 1, 0)], 0.0)
    hi = ref["cdf"][rows, a]
    bad = np.flatnonzero(~clear & ~((u64 >= lo - AMBIGUOUS) & (u64 <= hi + AMBIGUOUS)))
    if bad.size:
        fails.append("action: %d ambiguous rows away from the step, first row %d: %d against %d" % (bad.size, bad[0], a[bad[0]], ref["action"][bad[0]]))
    if logp is not None:
        want = ref["logp"][rows, a]
        with np.errstate(invalid="ignore"):
            off = np.abs(np.asarray(logp, dtype=np.float64) - want)
            bad = np.flatnonzero(~(off <= 1e-5 + 4 * 2.0 ** -24 * np.abs(want)) & (ref["p"][rows, a] > 0))
        if bad.size:
            fails.append("logp: %d rows, first row %d: %r against %r" % (bad.size, bad[0], float(np.asarray(logp)[bad[0]]), float(want[bad[0]])))
    return fails


def kernel_draw_f32(logits32, mask01, u, no_masking, nonzero_condition=True):
    """The draw's float32 arithmetic as csrc/skyjo_draw.h documents it (exponentials summed in blocks of four, block totals left to
    right, a block's CDF starting from the total before it), restated in numpy float32 - np.exp, not the device's fast exponential.
    ``nonzero_condition`` off restates the wrong kernel that may draw a masked action at the head of a block.  (action, logp float32)"""
    f = np.float32
    lg = np.asarray(logits32, dtype=f)
    on = np.ones(lg.shape, dtype=bool) if no_masking else np.asarray(mask01) != 0
    with np.errstate(over="ignore", under="ignore"):
        m = np.where(on, lg, (lg + FLOAT_MIN).astype(f)).astype(f)
        mx = m.max(axis=1, keepdims=True)
        e = np.exp((m - mx).astype(f)).astype(f)
        e[e < f(2.0 ** -126)] = 0.0                                       # (flushed)
    n = lg.shape[0]
    P = np.zeros((n, 8), dtype=f)
    for j in range(7):
        b = e[:, 4 * j].copy()
        for k in range(4 * j + 1, min(4 * j + 4, 26)):
            b = (b + e[:, k]).astype(f)
        P[:, j + 1] = (P[:, j] + b).astype(f)
    total = P[:, 7]
    target = (np.asarray(u, dtype=f) * total).astype(f)
    a, last_on = np.full(n, -1), np.zeros(n, dtype=np.int64)
    for j in range(7):
        acc = P[:, j].copy()
        for k in range(4 * j, min(4 * j + 4, 26)):
            acc = (acc + e[:, k]).astype(f)
            last_on = np.where(e[:, k] > 0, k, last_on)
            hit = (a < 0) & (acc > target)
            if nonzero_condition:
                hit &= e[:, k] > 0
            a = np.where(hit, k, a)
    a = np.where(a < 0, last_on, a)
    logp = ((m[np.arange(n), a] - mx[:, 0]).astype(f) - np.log(total).astype(f)).astype(f)
    return a, logp, dict(P=P, e=e, total=total)
