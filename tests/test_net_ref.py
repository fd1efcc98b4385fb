"""tests/net_ref.py without a GPU: its Philox against Random123's published vectors and the oracle's own, its forward references
against torch in float64 and the project's tolerances, the reach of its generators, and - with kernels restated wrongly in numpy -
that the checks tests/test_gpu_net_synthetic.py applies to the kernels reject what they are meant to reject."""
import numpy as np
import pytest

from tests import net_ref as ref

KAT = [  # Random123 kat_vectors: Philox4x32-10 (counter, key, output)
    ("00000000 00000000 00000000 00000000", "00000000 00000000", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1"),
]
DRAW_ROWS = 6553              # 104 rows of every (mask family, logit family) pair; 26 blocks of k_sample, the last one partial
HIGH = dict(seed=2 ** 32 + 3, ticket=2 ** 40 + 1)


def _words(s):
    return np.array([int(w, 16) for w in s.split()], dtype=np.uint32)


def test_philox_reproduces_the_published_vectors():
    for c, k, out in KAT:
        assert np.array_equal(ref.philox4x32_10(_words(c), _words(k)), _words(out)), c
    got = ref.philox4x32_10(np.stack([_words(c) for c, _, _ in KAT]), np.stack([_words(k) for _, k, _ in KAT]))
    assert np.array_equal(got, np.stack([_words(o) for _, _, o in KAT]))  # (vectorised over rows)


def test_philox_agrees_with_the_oracle():
    import ctypes as C

    from oracle import skyjo_oracle as so

    L = so.lib()
    rng = np.random.default_rng(3)
    ctr = rng.integers(0, 2 ** 32, size=(300, 4), dtype=np.uint64).astype(np.uint32)
    key = rng.integers(0, 2 ** 32, size=(300, 2), dtype=np.uint64).astype(np.uint32)
    want = ref.philox4x32_10(ctr, key)
    out = np.zeros(4, dtype=np.uint32)
    for i in range(300):
        c, k = np.ascontiguousarray(ctr[i]), np.ascontiguousarray(key[i])
        L.sko_philox4x32_10(c.ctypes.data_as(C.c_void_p), k.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
        assert np.array_equal(out, want[i]), i


def test_uniform_counter_layout():
    gid = ref.game_ids(2 ** 32 - 2, 4)
    assert gid.tolist() == [2 ** 32 - 2, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1]
    c = ref.draw_counter(2 ** 40 + 1, gid)
    assert c[:, 0].tolist() == [1] * 4 and c[:, 1].tolist() == [256] * 4
    assert c[:, 2].tolist() == [2 ** 32 - 2, 2 ** 32 - 1, 0, 1] and c[:, 3].tolist() == [0x53414D50, 0x53414D50, 0x53414D51, 0x53414D51]
    assert ref.game_ids(2 ** 64 - 1, 2).tolist() == [2 ** 64 - 1, 0]
    u = ref.uniform(2 ** 64 - 1, 2 ** 64 - 1, ref.game_ids(0, 5000))
    assert u.dtype == np.float32 and (u >= 0).all() and (u < 1).all() and abs(float(u.mean()) - 0.5) < 0.02
    w0 = ref.philox4x32_10(np.array([5, 0, 9, 0x53414D50], dtype=np.uint32), np.array([77, 0], dtype=np.uint32))[0]
    assert ref.uniform(77, 5, np.array([9], dtype=np.uint64))[0] == np.float32((int(w0) >> 8) * 2.0 ** -24)


@pytest.mark.parametrize("wset", ref.WEIGHT_SETS)
@pytest.mark.parametrize("shape", ref.SHAPES)
def test_exact_equals_the_torch_module_in_float64(shape, wset):
    import torch

    case = ref.forward_case(shape, wset, feature_range=ref.T1_RANGE)
    p = [torch.from_numpy(np.array(t)).double() for t in case["params"]]
    h = torch.from_numpy(np.array(case["x"][:600]))
    for i in range(3):
        h = torch.nn.functional.linear(h, p[2 * i], p[2 * i + 1])
        h = torch.tanh(h) if i < 2 else h
    assert np.abs(h.numpy() - case["X"][:600]).max() <= 1e-12 * max(1.0, np.abs(case["X"]).max())


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("wset", ref.T1_SETS)
@pytest.mark.parametrize("shape", ref.SHAPES)
def test_packed_lies_within_the_projects_tolerance_of_exact(shape, wset, precision):
    """The emulation models the net the project measured: on features in [-32, 31] with sets A and B, Q is within TOL of X."""
    case = ref.forward_case(shape, wset, feature_range=ref.T1_RANGE)
    d = np.abs(case["Q"][precision] - case["X"])
    print(shape, wset, precision, "max %.3e mean %.3e F %.3e" % (d.max(), d.mean(), case["F"]))
    assert case["t1"] and d.max() <= ref.TOL[precision]["max"] and d.mean() <= ref.TOL[precision]["mean"]
    d = np.abs(case["Q"][ref.Q_KEY[precision]] - case["X"])                    # (the form of Q the check uses)
    assert d.max() <= ref.TOL[precision]["max"] and d.mean() <= ref.TOL[precision]["mean"]
    assert case["F"] > 0.0
    assert ref.check_forward(case["Q"][precision].astype(np.float32), case, precision) == []


def test_pool_rows_and_planar_padding():
    rng = np.random.default_rng(1)
    rec, pool = ref.net_records(2 * ref.POOL + 5, 48, 17, rng)
    f = pool[:, :17].view(np.int8)
    assert (f[1] == -128).all() and (f[2] == 127).all() and set(f[3][::2]) == {-128} and set(f[3][1::2]) == {127} and set(f[4][::2]) == {127}
    assert f.min() == -128 and f.max() == 127
    assert np.array_equal(rec[ref.POOL + 7], pool[7]) and np.array_equal(rec[2 * ref.POOL + 4], pool[4])
    _, small = ref.net_records(1, 64, 31, rng, feature_range=ref.T1_RANGE)
    g = small[:, :31].view(np.int8)
    assert g.min() == -32 and g.max() == 31 and (small[:, 31:] > 127).any()        # the other bytes are anything
    planar = ref.to_planar(rec[:777], rng)
    assert planar.shape == (13, 3, 64, 16)
    assert np.array_equal(planar[12, :, 8, :].reshape(-1), rec[776])
    assert (planar[12, :, 9:, :] != 0).all()                                       # dirty padding


def test_saturating_and_near_zero_sets_reach_what_they_claim():
    for rng_ in (ref.T1_RANGE, (-128, 127)):
        s = np.abs(ref.layer1_tanh(ref.weights((31, 26), "S"), ref.forward_case((31, 26), "S", feature_range=rng_)["x"]))
        print(rng_, "S: share saturated %.3f" % (s >= 1 - 2.0 ** -24).mean())
        assert (s >= 1 - 2.0 ** -24).mean() >= 0.5
    z = np.abs(ref.layer1_tanh(ref.weights((31, 26), "Z"), ref.forward_case((31, 26), "Z", feature_range=ref.T1_RANGE)["x"]))
    print("Z: max |tanh| %.4f" % z.max())
    assert z.max() < 0.1


@pytest.fixture(scope="module")
def draw_cases():
    return {nm: ref.draw_case(DRAW_ROWS, HIGH["seed"], HIGH["ticket"], game_id0=2 ** 32 - 100, no_masking=nm) for nm in (False, True)}


def test_every_mask_family_meets_every_logit_family(draw_cases):
    c = draw_cases[False]
    assert set(np.unique(c["mask"])) == {0, 1}
    pairs = np.zeros((len(ref.MASK_FAMILIES), len(ref.LOGIT_FAMILIES)), dtype=int)
    np.add.at(pairs, (c["mask_family"], c["logit_family"]), 1)
    assert pairs.min() >= 32, pairs
    single = c["mask"][c["mask_family"] == ref.MASK_FAMILIES.index("single")]
    assert (single.sum(1) == 1).all() and set(np.argmax(single, 1)) == set(range(26))
    for k in range(26):   # one legal action at each k under every logit family
        rows = (c["mask_family"] == 2) & (c["mask"][:, k] == 1)
        assert set(c["logit_family"][rows]) == set(range(len(ref.LOGIT_FAMILIES))), k
    fam = lambda name: c["mask"][c["mask_family"] == ref.MASK_FAMILIES.index(name)][0].nonzero()[0].tolist()
    assert fam("even-blocks") == [0, 1, 2, 3, 8, 9, 10, 11, 16, 17, 18, 19, 24, 25] and fam("heads") == [0, 4, 8, 12, 16, 20, 24]
    assert fam("odd-blocks") == [4, 5, 6, 7, 12, 13, 14, 15, 20, 21, 22, 23] and fam("draw-phase") == [24, 25]
    lg = c["logits"]
    spread = lg.max(1) - lg.min(1)
    assert (spread[c["logit_family"] == 2] == 120).all() and (spread[c["logit_family"] == 1] == 0).all() and lg[c["logit_family"] == 5].min() > 9900
    mm = np.flatnonzero((c["logit_family"] == 6) & (c["mask"].min(1) == 0))
    assert mm.size > 500 and (c["mask"][mm, np.argmax(lg[mm], 1)] == 0).all()      # the maximum sits on a masked action


def test_ambiguous_share_is_small(draw_cases):
    """At most 26 steps x 2e-5 = 5.2e-4 of the rows for a uniform u; the cap is 2e-3, from the reference alone."""
    for nm, c in draw_cases.items():
        share = float(c["ref"]["ambiguous"].mean())
        print("no_masking", nm, "ambiguous share %.2e" % share)
        assert share <= 2e-3


@pytest.mark.parametrize("no_masking", [False, True])
def test_restated_draw_passes_the_check(draw_cases, no_masking):
    """The positive control: the documented float32 arithmetic, restated in numpy, passes check_draw on every family."""
    c = draw_cases[no_masking]
    a, lp, _ = ref.kernel_draw_f32(c["logits"], c["mask"], c["u"], no_masking)
    assert ref.check_draw(a, lp, c["u"], c) == []
    if not no_masking:
        legal = c["mask"].sum(1) > 0
        assert (c["mask"][legal, a[legal]] == 1).all()
        zeros = c["mask_family"] == ref.MASK_FAMILIES.index("zeros")
        assert len(set(a[zeros])) >= 20                                            # an all-zero mask: a uniform draw over 26


def test_check_forward_rejects_wrong_kernels():
    case = ref.forward_case((31, 26), "B", feature_range=ref.T1_RANGE)
    n = ref.POOL + 600
    idx = np.arange(n) % ref.POOL
    good = case["Q"][ref.Q_KEY["fp32"]][idx].astype(np.float32)
    m = ref.M_FP32
    assert ref.check_forward(good, case, "fp32") == []
    for wrong in ("w_lo_h_hi", "b2_lo"):
        bad = ref.packed(case["params"], case["x"], "fp32", wrong=wrong, act32=True)[idx].astype(np.float32)
        fails = ref.check_forward(bad, case, "fp32")
        print(wrong, fails, "max |bad - Q| %.3e" % np.abs(bad - good).max())
        assert fails, wrong
    for precision in ("fp32", "bf16"):   # batch b's outputs written as batch b + 1's
        q = case["Q"][ref.Q_KEY[precision]][idx].astype(np.float32)
        assert ref.check_forward(q, case, precision) == []
        assert ref.check_forward(np.roll(q, 256, axis=0), case, precision)
        swapped = q.copy()
        swapped[[40, 41]] = swapped[[41, 40]]             # two lanes exchanged
        assert ref.check_forward(swapped, case, precision)


def test_t2_bound_is_at_most_a_quarter_of_t1():
    """M_FP32 is the smallest power of two at least twice the largest recorded ratio, and M_FP32 x F stays within a quarter of T1's bound
    on the cases T1 covers - with the F of the run that measured the ratios (F is torch's float32 matmul and differs between CPUs; this
    machine's figures are printed)."""
    seen = max(r[0] for r in ref.RATIOS_SEEN.values())
    assert ref.M_FP32 == 2.0 ** round(np.log2(ref.M_FP32)) and ref.M_FP32 / 2 < 2 * seen <= ref.M_FP32
    assert ref.M_FP32 * ref.F_T1_SEEN <= 4 * ref.TOL["fp32"]["max"] / 4
    assert max(r[1] for r in ref.RATIOS_SEEN.values()) > seen                 # the float64 activation was the worse model
    for shape in ref.SHAPES:
        for wset in ref.T1_SETS:
            case = ref.forward_case(shape, wset, feature_range=ref.T1_RANGE)
            print(shape, wset, "F %.3e  M x F %.3e" % (case["F"], ref.M_FP32 * case["F"]))
            assert ref.M_FP32 * case["F"] <= 4 * ref.TOL["fp32"]["max"] / 2   # (and within half of it on any CPU seen so far)


def test_check_draw_rejects_wrong_philox(draw_cases):
    c = draw_cases[False]
    gid = ref.game_ids(c["game_id0"], c["n"])

    def low_ticket(ticket, g):
        k = ref.draw_counter(ticket, g)
        k[..., 1] = 0
        return k

    for name, u in (("ticket's high word dropped", ref.uniform(c["seed"], c["ticket"], gid, counter=low_ticket)),
                    ("game_id0 not added", ref.uniform(c["seed"], c["ticket"], ref.game_ids(0, c["n"]))),
                    ("game id's high word dropped", ref.uniform(c["seed"], c["ticket"], gid & np.uint64(ref.M32))),
                    ("seed's high word dropped", ref.uniform(c["seed"] & ref.M32, c["ticket"], gid))):
        a, lp, _ = ref.kernel_draw_f32(c["logits"], c["mask"], u, False)
        assert any(f.startswith("uniform") for f in ref.check_draw(a, lp, u, c)), name
        assert any(f.startswith("action") for f in ref.check_draw(a, lp, None, c)), name   # (even when the uniforms are not looked at)
    half = np.flatnonzero(gid >> np.uint64(32) == 0)
    assert 0 < half.size < c["n"]                          # the game id's high word changes inside the batch


def test_check_draw_rejects_a_draw_without_the_nonzero_condition():
    """A block's CDF starts from a total rounded on another path than the running sum of the block before; where it lies an ulp above,
    a uniform between the two draws the block's masked head unless zero-probability actions are excluded.  Such uniforms are
    constructed here for rows of the heads-masked family."""
    base = ref.draw_case(DRAW_ROWS, 1, 2)
    _, _, t = ref.kernel_draw_f32(base["logits"], base["mask"], base["u"], False)
    u = base["u"].copy()
    hits = []
    fam = ref.MASK_FAMILIES.index("no-heads")
    f = np.float32
    for g in np.flatnonzero(base["mask_family"] == fam):
        P, e, total = t["P"][g], t["e"][g], t["total"][g]
        for j in range(1, 7):
            end = P[j - 1]
            for k in range(4 * (j - 1), 4 * j):
                end = f(end + e[k])
            if not P[j] > end or total <= 0:
                continue
            for w in range(-2, 3):
                cand = f((int(float(end) / float(total) * 2 ** 24) + w) * 2.0 ** -24)
                if 0 <= cand < 1 and end <= f(cand * total) < P[j]:
                    u[g] = cand
                    hits.append((g, 4 * j))
                    break
            else:
                continue
            break
    assert len(hits) >= 3, len(hits)
    case = ref.draw_case(DRAW_ROWS, 1, 2, u=u)
    good, lp, _ = ref.kernel_draw_f32(case["logits"], case["mask"], u, False)
    assert ref.check_draw(good, lp, u, case) == []
    bad, lp, _ = ref.kernel_draw_f32(case["logits"], case["mask"], u, False, nonzero_condition=False)
    drew_head = [g for g, k in hits if bad[g] == k]
    assert drew_head and all(case["mask"][g, bad[g]] == 0 for g in drew_head)
    assert any(f_.startswith("an action of zero probability") for f_ in ref.check_draw(bad, lp, u, case))
