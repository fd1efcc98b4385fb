"""tests/board_inject.py on the CPU, oracle only: what every injected state must satisfy, and the conditions that keep
tests/test_gpu_late_boards.py from passing on boards that never get interesting - for every case of its every-action table and of its
rollout table, each count of board_inject.required() is above zero and at or above half of what the oracle showed when the table
below was recorded (a later change of a family cannot thin a case out unnoticed).  Also that the segment comparison sees the three
ways the collapse branch can be wrong, restated on the oracle's own records."""
import numpy as np
import pytest

from oracle import skyjo_oracle as so
from tests import board_inject as bi
from tests import pile_inject as pi

# (players, generator, indirect observation, games) -> what the oracle reached in the two compared segments (64 iterations each)
ROLLOUT_REACHED = {
    (2, 0, False, 320): {'rows_ref2': 1575, 'rows_ref3': 704, 'rows_ref4': 244, 'collapses': 157, 'multi_collapses': 41, 'ends': 693, 'ends_by_collapse': 30, 'ends_penalty': 217, 'ends_negative_penalty': 19, 'ends_tie': 65, 'rows_clip': 24, 'rows_hist40': 456, 'hist_max': 79, 'reshuffles': 0},
    (2, 0, True, 320): {'rows_ref2': 1575, 'rows_ref3': 704, 'rows_ref4': 244, 'collapses': 157, 'multi_collapses': 41, 'ends': 693, 'ends_by_collapse': 30, 'ends_penalty': 217, 'ends_negative_penalty': 19, 'ends_tie': 65, 'rows_clip': 24, 'rows_hist40': 456, 'hist_max': 79, 'reshuffles': 0},
    (2, 1, False, 320): {'rows_ref2': 1766, 'rows_ref3': 665, 'rows_ref4': 261, 'collapses': 159, 'multi_collapses': 37, 'ends': 696, 'ends_by_collapse': 26, 'ends_penalty': 203, 'ends_negative_penalty': 17, 'ends_tie': 72, 'rows_clip': 31, 'rows_hist40': 422, 'hist_max': 79, 'reshuffles': 0},
    (2, 1, True, 320): {'rows_ref2': 1766, 'rows_ref3': 665, 'rows_ref4': 261, 'collapses': 159, 'multi_collapses': 37, 'ends': 696, 'ends_by_collapse': 26, 'ends_penalty': 203, 'ends_negative_penalty': 17, 'ends_tie': 72, 'rows_clip': 31, 'rows_hist40': 422, 'hist_max': 79, 'reshuffles': 0},
    (3, 0, False, 320): {'rows_ref2': 1324, 'rows_ref3': 673, 'rows_ref4': 327, 'collapses': 151, 'multi_collapses': 33, 'ends': 615, 'ends_by_collapse': 23, 'ends_penalty': 223, 'ends_negative_penalty': 26, 'ends_tie': 109, 'rows_clip': 13, 'rows_hist40': 656, 'hist_max': 86, 'reshuffles': 0},
    (3, 0, True, 320): {'rows_ref2': 1324, 'rows_ref3': 673, 'rows_ref4': 327, 'collapses': 151, 'multi_collapses': 33, 'ends': 615, 'ends_by_collapse': 23, 'ends_penalty': 223, 'ends_negative_penalty': 26, 'ends_tie': 109, 'rows_clip': 13, 'rows_hist40': 656, 'hist_max': 86, 'reshuffles': 0},
    (3, 1, False, 320): {'rows_ref2': 1333, 'rows_ref3': 706, 'rows_ref4': 325, 'collapses': 141, 'multi_collapses': 32, 'ends': 614, 'ends_by_collapse': 17, 'ends_penalty': 222, 'ends_negative_penalty': 25, 'ends_tie': 111, 'rows_clip': 14, 'rows_hist40': 736, 'hist_max': 86, 'reshuffles': 0},
    (3, 1, True, 320): {'rows_ref2': 1333, 'rows_ref3': 706, 'rows_ref4': 325, 'collapses': 141, 'multi_collapses': 32, 'ends': 614, 'ends_by_collapse': 17, 'ends_penalty': 222, 'ends_negative_penalty': 25, 'ends_tie': 111, 'rows_clip': 14, 'rows_hist40': 736, 'hist_max': 86, 'reshuffles': 0},
    (4, 0, False, 300): {'rows_ref2': 1000, 'rows_ref3': 653, 'rows_ref4': 349, 'collapses': 146, 'multi_collapses': 25, 'ends': 562, 'ends_by_collapse': 18, 'ends_penalty': 214, 'ends_negative_penalty': 13, 'ends_tie': 130, 'rows_clip': 25, 'rows_hist40': 633, 'hist_max': 100, 'reshuffles': 0},
    (4, 0, False, 320): {'rows_ref2': 1057, 'rows_ref3': 698, 'rows_ref4': 387, 'collapses': 149, 'multi_collapses': 26, 'ends': 600, 'ends_by_collapse': 18, 'ends_penalty': 228, 'ends_negative_penalty': 15, 'ends_tie': 144, 'rows_clip': 25, 'rows_hist40': 647, 'hist_max': 100, 'reshuffles': 0},
    (4, 0, True, 300): {'rows_ref2': 1000, 'rows_ref3': 653, 'rows_ref4': 349, 'collapses': 146, 'multi_collapses': 25, 'ends': 562, 'ends_by_collapse': 18, 'ends_penalty': 214, 'ends_negative_penalty': 13, 'ends_tie': 130, 'rows_clip': 25, 'rows_hist40': 626, 'hist_max': 99, 'reshuffles': 0},
    (4, 0, True, 320): {'rows_ref2': 1057, 'rows_ref3': 698, 'rows_ref4': 387, 'collapses': 149, 'multi_collapses': 26, 'ends': 600, 'ends_by_collapse': 18, 'ends_penalty': 228, 'ends_negative_penalty': 15, 'ends_tie': 144, 'rows_clip': 25, 'rows_hist40': 640, 'hist_max': 99, 'reshuffles': 0},
    (4, 1, False, 320): {'rows_ref2': 1056, 'rows_ref3': 727, 'rows_ref4': 375, 'collapses': 137, 'multi_collapses': 29, 'ends': 596, 'ends_by_collapse': 18, 'ends_penalty': 243, 'ends_negative_penalty': 20, 'ends_tie': 139, 'rows_clip': 23, 'rows_hist40': 771, 'hist_max': 99, 'reshuffles': 0},
    (4, 1, True, 300): {'rows_ref2': 1015, 'rows_ref3': 693, 'rows_ref4': 352, 'collapses': 130, 'multi_collapses': 27, 'ends': 562, 'ends_by_collapse': 18, 'ends_penalty': 230, 'ends_negative_penalty': 18, 'ends_tie': 128, 'rows_clip': 23, 'rows_hist40': 740, 'hist_max': 99, 'reshuffles': 0},
    (4, 1, True, 320): {'rows_ref2': 1056, 'rows_ref3': 727, 'rows_ref4': 375, 'collapses': 137, 'multi_collapses': 29, 'ends': 596, 'ends_by_collapse': 18, 'ends_penalty': 243, 'ends_negative_penalty': 20, 'ends_tie': 139, 'rows_clip': 23, 'rows_hist40': 755, 'hist_max': 99, 'reshuffles': 0},
    (5, 0, True, 320): {'rows_ref2': 831, 'rows_ref3': 578, 'rows_ref4': 420, 'collapses': 132, 'multi_collapses': 31, 'ends': 588, 'ends_by_collapse': 12, 'ends_penalty': 252, 'ends_negative_penalty': 15, 'ends_tie': 217, 'rows_clip': 40, 'rows_hist40': 609, 'hist_max': 106, 'reshuffles': 0},
    (12, 0, False, 128): {'rows_ref2': 1364, 'rows_ref3': 65, 'rows_ref4': 0, 'collapses': 133, 'multi_collapses': 11, 'ends': 211, 'ends_by_collapse': 9, 'ends_penalty': 192, 'ends_negative_penalty': 7, 'ends_tie': 13, 'rows_clip': 10, 'rows_hist40': 1538, 'hist_max': 94, 'reshuffles': 496},
}
ACTION_REACHED = {
    (2, 0, True): {'rows_ref2': 155, 'rows_ref3': 186, 'rows_ref4': 217, 'collapses': 55, 'multi_collapses': 26, 'ends': 34, 'ends_by_collapse': 0, 'ends_penalty': 12, 'ends_negative_penalty': 4, 'ends_tie': 8, 'rows_clip': 62, 'rows_hist40': 124, 'hist_max': 66, 'reshuffles': 0, 'reveal_open': 86, 'reveal_refunded': 63, 'place_on_refunded': 63, 'draw_while_holding': 30, 'place_without_hand': 600, 'range_draw': 125, 'range_place': 75},
    (2, 1, False): {'rows_ref2': 93, 'rows_ref3': 279, 'rows_ref4': 186, 'collapses': 55, 'multi_collapses': 27, 'ends': 34, 'ends_by_collapse': 0, 'ends_penalty': 14, 'ends_negative_penalty': 4, 'ends_tie': 8, 'rows_clip': 62, 'rows_hist40': 124, 'hist_max': 67, 'reshuffles': 0, 'reveal_open': 73, 'reveal_refunded': 63, 'place_on_refunded': 63, 'draw_while_holding': 28, 'place_without_hand': 624, 'range_draw': 130, 'range_place': 70},
    (3, 1, True): {'rows_ref2': 155, 'rows_ref3': 310, 'rows_ref4': 124, 'collapses': 56, 'multi_collapses': 29, 'ends': 32, 'ends_by_collapse': 0, 'ends_penalty': 16, 'ends_negative_penalty': 4, 'ends_tie': 8, 'rows_clip': 62, 'rows_hist40': 124, 'hist_max': 81, 'reshuffles': 0, 'reveal_open': 68, 'reveal_refunded': 60, 'place_on_refunded': 60, 'draw_while_holding': 26, 'place_without_hand': 648, 'range_draw': 135, 'range_place': 65},
    (3, 0, False): {'rows_ref2': 155, 'rows_ref3': 279, 'rows_ref4': 124, 'collapses': 57, 'multi_collapses': 27, 'ends': 30, 'ends_by_collapse': 0, 'ends_penalty': 14, 'ends_negative_penalty': 4, 'ends_tie': 10, 'rows_clip': 62, 'rows_hist40': 124, 'hist_max': 81, 'reshuffles': 0, 'reveal_open': 82, 'reveal_refunded': 63, 'place_on_refunded': 63, 'draw_while_holding': 30, 'place_without_hand': 600, 'range_draw': 125, 'range_place': 75},
    (4, 0, True): {'rows_ref2': 217, 'rows_ref3': 186, 'rows_ref4': 124, 'collapses': 58, 'multi_collapses': 27, 'ends': 26, 'ends_by_collapse': 0, 'ends_penalty': 14, 'ends_negative_penalty': 4, 'ends_tie': 10, 'rows_clip': 62, 'rows_hist40': 186, 'hist_max': 90, 'reshuffles': 0, 'reveal_open': 87, 'reveal_refunded': 69, 'place_on_refunded': 69, 'draw_while_holding': 32, 'place_without_hand': 576, 'range_draw': 120, 'range_place': 80},
    (4, 1, False): {'rows_ref2': 155, 'rows_ref3': 217, 'rows_ref4': 124, 'collapses': 55, 'multi_collapses': 26, 'ends': 26, 'ends_by_collapse': 0, 'ends_penalty': 14, 'ends_negative_penalty': 4, 'ends_tie': 12, 'rows_clip': 62, 'rows_hist40': 248, 'hist_max': 91, 'reshuffles': 0, 'reveal_open': 99, 'reveal_refunded': 63, 'place_on_refunded': 63, 'draw_while_holding': 32, 'place_without_hand': 576, 'range_draw': 120, 'range_place': 80},
    (1, 1, True): {'rows_ref2': 62, 'rows_ref3': 248, 'rows_ref4': 186, 'collapses': 56, 'multi_collapses': 27, 'ends': 34, 'ends_by_collapse': 0, 'ends_penalty': 0, 'ends_negative_penalty': 0, 'ends_tie': 0, 'rows_clip': 0, 'rows_hist40': 124, 'hist_max': 57, 'reshuffles': 0, 'reveal_open': 85, 'reveal_refunded': 51, 'place_on_refunded': 51, 'draw_while_holding': 28, 'place_without_hand': 624, 'range_draw': 130, 'range_place': 70},
    (1, 0, False): {'rows_ref2': 62, 'rows_ref3': 248, 'rows_ref4': 186, 'collapses': 56, 'multi_collapses': 26, 'ends': 34, 'ends_by_collapse': 0, 'ends_penalty': 0, 'ends_negative_penalty': 0, 'ends_tie': 0, 'rows_clip': 0, 'rows_hist40': 124, 'hist_max': 57, 'reshuffles': 0, 'reveal_open': 83, 'reveal_refunded': 51, 'place_on_refunded': 51, 'draw_while_holding': 28, 'place_without_hand': 624, 'range_draw': 130, 'range_place': 70},
    (5, 0, True): {'rows_ref2': 124, 'rows_ref3': 217, 'rows_ref4': 155, 'collapses': 57, 'multi_collapses': 26, 'ends': 28, 'ends_by_collapse': 0, 'ends_penalty': 14, 'ends_negative_penalty': 4, 'ends_tie': 14, 'rows_clip': 62, 'rows_hist40': 248, 'hist_max': 99, 'reshuffles': 0, 'reveal_open': 92, 'reveal_refunded': 66, 'place_on_refunded': 66, 'draw_while_holding': 32, 'place_without_hand': 576, 'range_draw': 120, 'range_place': 80},
    (5, 1, False): {'rows_ref2': 155, 'rows_ref3': 186, 'rows_ref4': 155, 'collapses': 55, 'multi_collapses': 26, 'ends': 30, 'ends_by_collapse': 0, 'ends_penalty': 14, 'ends_negative_penalty': 4, 'ends_tie': 18, 'rows_clip': 62, 'rows_hist40': 217, 'hist_max': 100, 'reshuffles': 0, 'reveal_open': 78, 'reveal_refunded': 57, 'place_on_refunded': 57, 'draw_while_holding': 28, 'place_without_hand': 624, 'range_draw': 130, 'range_place': 70},
    (12, 1, True): {'rows_ref2': 496, 'rows_ref3': 0, 'rows_ref4': 0, 'collapses': 53, 'multi_collapses': 27, 'ends': 18, 'ends_by_collapse': 0, 'ends_penalty': 14, 'ends_negative_penalty': 4, 'ends_tie': 4, 'rows_clip': 62, 'rows_hist40': 310, 'hist_max': 48, 'reshuffles': 0, 'reveal_open': 96, 'reveal_refunded': 54, 'place_on_refunded': 54, 'draw_while_holding': 32, 'place_without_hand': 576, 'range_draw': 120, 'range_place': 80},
    (12, 0, False): {'rows_ref2': 465, 'rows_ref3': 0, 'rows_ref4': 0, 'collapses': 59, 'multi_collapses': 27, 'ends': 18, 'ends_by_collapse': 0, 'ends_penalty': 14, 'ends_negative_penalty': 4, 'ends_tie': 4, 'rows_clip': 62, 'rows_hist40': 434, 'hist_max': 94, 'reshuffles': 0, 'reveal_open': 91, 'reveal_refunded': 45, 'place_on_refunded': 45, 'draw_while_holding': 30, 'place_without_hand': 600, 'range_draw': 125, 'range_place': 75},
}


def _vec(N, rng_mode, indirect, B, auto_reset=True):
    return so.OracleVec(num_envs=B, **dict(pi.oracle_config(N, rng_mode, indirect), auto_reset=auto_reset))


def _hold(n, recorded, need, tag):
    print(tag, n)
    for k in need:
        assert n[k] > 0, (tag, k)
    for k, v in recorded.items():
        if k != "hist_max":
            assert n[k] >= v / 2, (tag, k, n[k], v)
    assert 40 <= n["hist_max"] <= 127, (tag, n["hist_max"])  # (above 127 the reference's int8 cast is not defined)


# ------------------------------------------------------------------------------------------ every injected state
@pytest.mark.parametrize("N", [1, 2, 3, 4, 5, 12])
def test_every_injected_state_is_one_the_reference_defines(N):
    """cards + piles = 150, a discard pile, MIN_PILE, n_disc <= 150, whole refunded columns only, and no histogram feature above 127 in
    either observation mode - for every family, every brink kind, every recipe in both phases; three zeros per refunded column."""
    B = 64
    ora = _vec(N, pi.MT, True, B)
    ora.seed(None, 3)
    dealt = [pi.oracle_state(ora, g) for g in range(B)]
    rng = np.random.default_rng(N)
    kinds = set()
    for g, s in enumerate(dealt):
        fns = [bi.late, bi.late_zeros, bi.pending, bi.mixed] + [lambda s, r, n, k=k: bi.brink(s, r, n, kind=k) for k in bi.BRINK_KINDS]
        fns += [lambda s, r, n, rp=rp: bi.recipe_board(rp[0], rp[1], s, r, n) for rp in bi.RECIPES]
        for fn in fns:
            board = fn(s, rng, N)
            bi.check_board(board, N)
            cards, masked, draw, disc, hand, player, phase = board
            assert player == s["player"] and disc[-1] == s["disc"][-1]            # the turn and the discard top stay
            zeros = int((disc == 0).sum()) - int((np.asarray(s["disc"]) == 0).sum())
            columns = int((masked == bi.C).reshape(N, 4, 3).all(axis=2).sum())
            assert zeros >= 3 * columns and (zeros == 3 * columns or len(draw) + (hand != bi.NONE) < len(s["draw"]))  # more only with late_zeros
            assert int((masked == bi.C).reshape(N, 4, 3).all(axis=2).sum(axis=1).max()) <= bi.max_ref(N)  # (per seat; 2 from six players on)
            kinds.add((int((masked[player] == bi.C).sum()) // 3, phase))
    assert {k for k, _ in kinds} == set(range(bi.max_ref(N) + 1)) and {ph for _, ph in kinds} == {0, 1}
    if N > 5:
        assert max(int((bi.late(s, rng, N)[1] == bi.C).sum(axis=1).max()) for s in dealt) == 3 * 2  # max_ref 2


def test_pile_families_are_untouched_by_the_whole_state_hook():
    """pile_inject.inject with a pile family still leaves the boards, the hand and the turn as dealt (the hook only adds a path)."""
    ora = _vec(3, pi.MT, True, 64)
    ora.seed(None, 3)
    before = [pi.oracle_state(ora, g) for g in range(64)]
    pi.inject("near-empty", np.random.default_rng(1), ora)
    for g in range(64):
        a, b = before[g], pi.oracle_state(ora, g)
        for k in ("cards", "masked"):
            np.testing.assert_array_equal(a[k], b[k])
        assert (a["hand"], a["player"], a["phase"]) == (b["hand"], b["player"], b["phase"])


# ------------------------------------------------------------------------------------------ what the GPU file's cases reach
@pytest.mark.parametrize("key", list(ACTION_REACHED), ids=["N%d_%s_%s" % (k[0], "px" if k[1] else "mt", "ind" if k[2] else "dir") for k in ACTION_REACHED])
def test_every_action_table_reaches_what_it_is_for(key):
    N, rng_mode, ind = key
    assert {(c[0], c[1], c[2]) for c in bi.ACTION_CASES.values()} == set(ACTION_REACHED)
    for auto_reset in (False, True):  # (the one step is the same; with auto_reset the oracle deals the finished games again)
        n = bi.every_action(_vec(N, rng_mode, ind, bi.BOARDS * len(bi.ACTIONS), auto_reset), bi.ACTION_SEED, ind)
        _hold(n, ACTION_REACHED[key], bi.required(N, 2) + list(bi.ILLEGAL), f"every action {key} auto_reset={auto_reset}:")


@pytest.mark.parametrize("key", list(ROLLOUT_REACHED), ids=["N%d_%s_%s_%d" % (k[0], "px" if k[1] else "mt", "ind" if k[2] else "dir", k[3]) for k in ROLLOUT_REACHED])
def test_rollout_table_reaches_what_it_is_for(key):
    N, rng_mode, ind, B = key
    assert {(c[0], c[1], c[2], c[3]) for c in bi.ROLLOUT_CASES.values()} | {bi.SNAPSHOT_CASE[:4]} == set(ROLLOUT_REACHED)
    rounds, n = bi.play(_vec(N, rng_mode, ind, B), ind)
    _hold(n, ROLLOUT_REACHED[key], bi.required(N, 3), f"rollout {key}:")
    if N == 12:
        assert n["reshuffles"] > 0  # (the reshuffle's histogram walk meets piles that hold collapse zeros)


def test_brink_family_ends_at_once_under_caller_actions():
    """tests/test_gpu_late_boards.py's step_collect case: a quarter of the games and more end within the injected boards' first turns."""
    N, rng_mode, ind, B, steps = bi.COLLECT_CASE
    early = [0]

    def after_step(t, acts, ended):
        early[0] += int(ended.sum()) if t < 2 * N + 2 else 0

    per_game, deepest, ends = pi.play_caller(_vec(N, rng_mode, ind, B), bi.brink_only, steps, after_step=after_step, reveal=True)
    print(f"brink under caller actions: {ends} ends, {early[0]} early")
    assert ends >= early[0] >= B // 4


# ------------------------------------------------------------------------------------------ teeth
class _WrongCollapse:
    """What three mistakes in the collapse branch of csrc/skyjo_transition.h would leave in the state it keeps incrementally, followed
    on the oracle's games through a compared segment: the seat's open sum keeps the three collapsed cards (+ 3 v per column), the
    histogram never gets the three zeros (- 3 per column on the zeros feature), num_refunded counts columns where the reference
    counts places.  All three start from zero at the injection (set_state rebuilds) and at every new deal."""

    def __init__(self, ora):
        self.ora, self.G, self.N = ora, bi.games_view(ora), ora.num_players
        self.obs0, self.zeros, self.extra, self.games = 0, 0, 0, [set(), set()]
        self.extra_finished, self.ends_with_extra = 0, 0  # ... of it in episodes that END inside the segment: what rewards and sums show

    def _now(self):
        N = self.N
        return (self.G["players_masked"][:, :N].copy(), self.G["players_cards"][:, :N].astype(np.int64), self.G["episode"].copy(),
                self.G["is_terminated"].copy())

    def __call__(self, t):
        B, N = self.ora.num_envs, self.N
        if t < 0:
            self.prev, self.sum_off, self.zero_off = self._now(), np.zeros((B, N), np.int64), np.zeros(B, np.int64)
            self.extra_off = np.zeros(B, np.int64)
            return
        (ma, ca, ea, oa), (mb, cb, eb, ob) = self.prev, self._now()
        same = ea == eb
        self.sum_off[~same], self.zero_off[~same], self.extra_off[~same] = 0, 0, 0
        new = same[:, None, None] & (mb.reshape(B, N, 4, 3)[..., 0] == bi.C) & (ma.reshape(B, N, 4, 3)[..., 0] != bi.C)
        value = np.median(ca.reshape(B, N, 4, 3), axis=3).astype(np.int64)  # two of the three cards stood there before the place
        self.sum_off += 3 * np.where(new, value, 0).sum(axis=2)
        self.zero_off -= 3 * new.sum(axis=(1, 2))
        self.extra += int(np.maximum(new.sum(axis=2) - 1, 0).sum())
        self.extra_off += np.maximum(new.sum(axis=2) - 1, 0).sum(axis=1)
        ended = same & (oa == 0) & (ob != 0)
        self.extra_finished += int(self.extra_off[ended].sum())
        self.ends_with_extra += int((self.extra_off[ended] > 0).sum())
        sums = np.where(mb == bi.O, cb, 0).sum(axis=2)
        wrong = np.minimum((sums + self.sum_off).min(axis=1), 127) != np.minimum(sums.min(axis=1), 127)
        self.obs0 += int(wrong.sum())
        self.zeros += int((self.zero_off != 0).sum())
        self.games[0].update(np.flatnonzero(wrong))
        self.games[1].update(np.flatnonzero(self.zero_off != 0))
        self.prev = (mb, cb, eb, ob)


@pytest.mark.parametrize("name", ["inline8_N2_mt_ind", "one8_S2_N3_px_ind", "one8_planar_all_N4_mt_ind", "inline8_N5_mt_ind", "two8_N12_mt_dir_128"])
def test_a_wrong_collapse_branch_shows_in_the_compared_fields(name):
    """In rollout cases of tests/test_gpu_late_boards.py - compile-time and generic kernels -, each of the three mistakes changes what
    that file compares with ==: obs[0] and obs[4] of many records in many games, and - through episodes with a multi-column collapse
    that end inside the compared iterations - the rewards of finished games and the per-seat sum of num_refunded."""
    N, rng_mode, ind, B = bi.ROLLOUT_CASES[name][:4]
    ora = _vec(N, rng_mode, ind, B)
    w = _WrongCollapse(ora)
    pi.play(ora, bi.mixed, iters=bi.ITERS, probe=w)
    print(f"{name}: a sum that keeps collapsed cards shows in obs[0] of {w.obs0} records ({len(w.games[0])} games), a histogram without the zeros in "
          f"obs[4] of {w.zeros} records ({len(w.games[1])} games), num_refunded per column counts {w.extra} too many, {w.extra_finished} of them in "
          f"{w.ends_with_extra} episodes that end inside the segments (their rewards and the per-seat sum of num_refunded show it)")
    assert len(w.games[0]) >= 10 and len(w.games[1]) >= 40 and w.extra >= 5
    if N <= 5:  # each such end changes rewards_host and counters()' sum_refunded; at twelve players no such episode ends within twice 64
        assert w.ends_with_extra >= 3 and w.extra_finished >= w.ends_with_extra  # iterations: there the every-action cases see it (get_state)
