"""The float64 ORDER of the two scoring functions, pinned to the reference without a GPU.

tests/golden/scoring_order.npz (oracle/gen_golden.py: gen_scoring) holds what the imported reference's ``SkyjoGame._evaluate_game``
(skyjo.py:477-498) and ``SimpleSkyjoEnv._calc_final_rewards`` (skyjo_env.py:293-312) returned for end hands of N = 1 .. 12 under the
penalties 2, 1.3, 1/3 and 0.01 and for arbitrary float64 score vectors.  With integer scores and a dyadic penalty every sum is exact
and no order shows; with these it does:

  * the CPU oracle (oracle/skyjo_oracle.c) gives the fixture bit for bit - the pairwise branch of its np_sum_f64 included;
  * so does the plain-Python restatement of the right order (tests/scoring_order_ref.py), which the GPU tests use to count the
    episodes whose mean is order-sensitive;
  * three wrong orders are each REJECTED by the fixture, for every N at which they can differ at all: the left-to-right sum from
    eight players on, the reversed sum below eight, and a sum whose addition of the penalised score is a fused multiply-add;
  * from eight players on at least 5 % of the penalty-1/3 rows separate the pairwise sum from the left-to-right one (the shares
    are printed: ``pytest -s``).
"""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import skyjo_oracle as so
from tests import scoring_order_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PLAYERS = list(range(1, 13))


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(GOLDEN, "scoring_order.npz")))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _oracle_scores(hand, finisher, penalty):
    L = so.lib()
    h = np.ascontiguousarray(hand, dtype=np.int8)
    out = np.zeros(h.shape[0], dtype=np.float64)
    L.sko_evaluate_game(h.ctypes.data_as(C.c_void_p), int(h.shape[0]), int(finisher), float(penalty), out.ctypes.data_as(C.c_void_p))
    return out


def _oracle_rewards(scores, refunded, mr, rr):
    L = so.lib()
    g = so.Game()
    g.num_players = len(scores)
    for p, (s, r) in enumerate(zip(scores, refunded)):
        g.final_score[p], g.num_refunded[p] = float(s), int(r)
    out = np.zeros(len(scores), dtype=np.float64)
    L.sko_final_rewards(C.byref(g), float(mr), float(rr), out.ctypes.data_as(C.c_void_p))
    return out


def _hand_rows(fx, N):
    """(penalty index, penalty, hand index, reward pair) of every hand row of the fixture at N players."""
    p = "N%d_" % N
    for k, pen in enumerate(fx["penalties"]):
        for e in range(fx[p + "hands"].shape[0]):
            yield k, float(pen), e, tuple(float(x) for x in fx["reward_cfgs"][fx[p + "cfg"][k, e]])


def test_fixture_shape_and_contents(fx):
    assert list(fx["players"]) == PLAYERS
    np.testing.assert_array_equal(fx["penalties"], [2.0, 1.3, 1.0 / 3.0, 0.01])
    np.testing.assert_array_equal(fx["reward_cfgs"], [(1.0, 0.001), (0.1, 0.007), (1.0 / 3.0, 0.0), (-1.0, 0.01)])
    triples = equal_rows = negative = 0
    refund_counts = set()
    for N in PLAYERS:
        p = "N%d_" % N
        h = fx[p + "hands"]
        assert h.dtype == np.int8 and h.shape[1:] == (N, 12) and h.min() >= -2 and h.max() <= 12
        refund_counts |= set(fx[p + "refunded"].ravel().tolist()) | set(fx[p + "frefunded"].ravel().tolist())
        assert N == 1 or (fx[p + "refunded"].min() == 0 and fx[p + "refunded"].max() == 4)
        cols = h.reshape(h.shape[0], N, 4, 3)
        triples += int((cols.min(-1) == cols.max(-1)).sum())
        equal_rows += int((h.min(-1) == h.max(-1)).sum())
        negative += int((fx[p + "scores"] < 0).sum())
        # every reward pair under every penalty
        for k in range(len(fx["penalties"])):
            assert set(fx[p + "cfg"][k]) == set(range(len(fx["reward_cfgs"])))
        f = np.abs(fx[p + "fscores"])
        assert f.min() >= 1e-3 and f.max() <= 1e6 and (fx[p + "fscores"] < 0).any() and (fx[p + "fscores"] > 0).any()
    assert triples > 100 and equal_rows > 10 and negative > 100 and refund_counts == {0, 1, 2, 3, 4}


@pytest.mark.parametrize("N", PLAYERS)
def test_oracle_and_restatement_give_the_fixture_bit_for_bit(fx, N):
    p = "N%d_" % N
    hands, fin, refunded = fx[p + "hands"], fx[p + "finisher"], fx[p + "refunded"]
    for k, pen, e, (mr, rr) in _hand_rows(fx, N):
        want_s, want_r = fx[p + "scores"][k, e], fx[p + "rewards"][k, e]
        at = f"N={N} penalty={pen} hand={e}"
        sc = _oracle_scores(hands[e], fin[e], pen)
        np.testing.assert_array_equal(_bits(sc), _bits(want_s), err_msg="oracle scores, " + at)
        np.testing.assert_array_equal(_bits(_oracle_rewards(sc, refunded[e], mr, rr)), _bits(want_r), err_msg="oracle rewards, " + at)
        rs = ref.scores(hands[e], int(fin[e]), pen)
        np.testing.assert_array_equal(_bits(rs), _bits(want_s), err_msg="restated scores, " + at)
        np.testing.assert_array_equal(_bits(ref.rewards(rs, refunded[e], mr, rr)), _bits(want_r), err_msg="restated rewards, " + at)
    for j, (mr, rr) in enumerate(fx["reward_cfgs"]):
        for f in range(fx[p + "fscores"].shape[0]):
            v, rf, want = fx[p + "fscores"][f], fx[p + "frefunded"][f], fx[p + "frewards"][j, f]
            at = f"N={N} pair={j} vector={f}"
            np.testing.assert_array_equal(_bits(_oracle_rewards(v, rf, mr, rr)), _bits(want), err_msg="oracle rewards, " + at)
            np.testing.assert_array_equal(_bits(ref.rewards(v, rf, float(mr), float(rr))), _bits(want), err_msg="restated rewards, " + at)


def _rejections(fx, N, summer):
    """Rows of the fixture that a _calc_final_rewards with `summer` as its sum gets wrong: (hand rows, score-vector rows)."""
    p = "N%d_" % N
    hand_rows = vec_rows = 0
    for k, pen, e, (mr, rr) in _hand_rows(fx, N):
        got = ref.rewards(fx[p + "scores"][k, e], fx[p + "refunded"][e], mr, rr, summer)
        hand_rows += not np.array_equal(_bits(got), _bits(fx[p + "rewards"][k, e]))
    for j, (mr, rr) in enumerate(fx["reward_cfgs"]):
        for f in range(fx[p + "fscores"].shape[0]):
            got = ref.rewards(fx[p + "fscores"][f], fx[p + "frefunded"][f], float(mr), float(rr), summer)
            vec_rows += not np.array_equal(_bits(got), _bits(fx[p + "frewards"][j, f]))
    return hand_rows, vec_rows


@pytest.mark.parametrize("N", PLAYERS)
def test_left_to_right_sum_from_eight_players_on_is_rejected(fx, N):
    hand_rows, vec_rows = _rejections(fx, N, ref.sum_wrong_left_from_8)
    print(f"left-to-right sum at N={N}: rejected by {hand_rows} hand rows and {vec_rows} score-vector rows")
    if N >= 8:
        assert hand_rows > 0 and vec_rows > 0
    else:
        assert hand_rows == 0 and vec_rows == 0  # below eight the left-to-right sum IS np.mean's


@pytest.mark.parametrize("N", PLAYERS)
def test_reversed_sum_below_eight_players_is_rejected(fx, N):
    hand_rows, vec_rows = _rejections(fx, N, ref.sum_wrong_reversed_below_8)
    print(f"reversed sum at N={N}: rejected by {hand_rows} hand rows and {vec_rows} score-vector rows")
    if 3 <= N < 8:
        assert hand_rows > 0 and vec_rows > 0
    else:
        assert hand_rows == 0 and vec_rows == 0  # one or two addends: no order; from eight on the restatement is the right one


@pytest.mark.parametrize("N", PLAYERS)
def test_fused_multiply_add_in_the_sum_is_rejected(fx, N):
    p = "N%d_" % N
    wrong = 0
    for k, pen, e, (mr, rr) in _hand_rows(fx, N):
        got = ref.rewards_wrong_fused(fx[p + "hands"][e], int(fx[p + "finisher"][e]), pen, fx[p + "refunded"][e], mr, rr)
        bad = not np.array_equal(_bits(got), _bits(fx[p + "rewards"][k, e]))
        assert not (bad and pen == 2.0), "a product with a power of two is exact: fusing cannot change it"
        wrong += bad
    print(f"fused multiply-add at N={N}: rejected by {wrong} hand rows")
    if N >= 2:
        assert wrong > 0
    else:
        assert wrong == 0  # one player is never penalised


def test_order_sensitivity_shares(fx):
    """From eight players on: the share of rows whose np.mean differs from the left-to-right sum divided by N, per penalty and
    for the arbitrary score vectors.  At least 5 % of the penalty-1/3 rows, for every N."""
    third = int(np.flatnonzero(fx["penalties"] == 1.0 / 3.0)[0])
    for N in range(8, 13):
        p = "N%d_" % N
        shares = []
        for k in range(len(fx["penalties"])):
            rows = fx[p + "scores"][k]
            shares.append(sum(ref.order_sensitive(r) for r in rows) / len(rows))
        vec = sum(ref.order_sensitive(r) for r in fx[p + "fscores"]) / len(fx[p + "fscores"])
        print(f"N={N}: order-sensitive share of the hand rows per penalty " +
              ", ".join(f"{float(q):.4g}: {100 * s:.1f} %" for q, s in zip(fx["penalties"], shares)) + f"; of the score vectors {100 * vec:.1f} %")
        assert shares[0] == 0.0  # penalty 2: every sum exact
        assert shares[third] >= 0.05, (N, shares)
