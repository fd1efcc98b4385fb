"""Board injection: the late part of a game, where random play never gets (TEST INFRASTRUCTURE; numpy only, nothing from the package -
an engine and an oracle come in as arguments).  tests/pile_inject.py takes the draw pile away; this file deals the players' boards.

The environment kernels keep the derived state of a game incrementally (per seat the open-card sum, the hidden count and num_refunded;
the minima over seats; the u8[15] histogram; the visible-byte image; the discard count) and the reference recomputes all of it at every
observation (skyjo.py:148-257).  A wrong += or -= only shows on boards with several refunded columns, and 5.3 M steps of random play
show an acting seat with two refunded columns 192 times and with three never (EXPERIMENTS.md has the table).  Three families of WHOLE-state injections - pure functions of (the dealt state,
a numpy Generator, the player count) that return (cards, masked, draw, disc, hand, player, phase) - put such boards under a freshly
dealt game (pile_inject.inject: only at episode step 0 with no reshuffle yet):

  late     per seat k in 0 .. max_ref refunded columns (cards -14, masked 0; max_ref 4 up to five players, 2 above: 4 x 12 collapses
           would put 144 zeros into one histogram feature, and the reference's int8 cast is not defined above 127); every other
           column is one of five kinds - two equal open cards and the third equal and hidden (a reveal collapses it), two equal open
           cards and the third open and different (a place of the value collapses it), all open, one hidden, as dealt.
           late_zeros: the same with 40 .. 60 cards from the bottom of the draw pile turned into zeros under the discard top - what
           14 .. 20 collapses leave behind, more than one or two players can make (12 N + 10 zeros at most) - so that a histogram
           feature of 40 and more is met at every player count (up to five players; twelve get there on their own).
  brink    one or two actions from the end: the acting seat has no hidden card (the game ends at the goal check of its draw) / has
           exactly one, the third of an equal column (the game finishes by collapse) / finishes and is not the lowest (the penalty,
           also on a negative score) / finishes on a tie at the minimum / every column of every seat refunded (all scores 0; up to
           nine players, see above) / an open sum above 127 on every seat (obs[0] clips).
  pending  one to three columns of the acting seat are open and equal but not refunded.  Play cannot get there; the reference defines
           it (scenario multi_collapse, skyjo.py:418-419): the next place collapses them all at once with num_refunded + 1.

Three zeros go under the discard top for every refunded column - what the reference appends (skyjo.py:454-458) -, so cards + piles
stay 150.  `mixed` draws a family per game (the rollout cases), `RECIPES` is the fixed list of boards the every-action cases cycle
through; `every_action` is the whole of such a case - with an engine it holds the comparison itself (records, rewards, the state of
every game, counters, the step after an auto-reset), the way pile_inject.play holds that of a rollout case.  `Reach` counts, on the oracle alone, what a compared segment got to; tests/test_board_inject.py holds every case to floors.
"""
import warnings

import numpy as np

from tests import pile_inject as pi

REFUNDED, NONE = -14, 15
H, O, C = 2, 1, 0  # hidden / open / collapsed (skyjo.py:99,394,454)
ITERS = 64         # compared iterations of a segment
MT, PHILOX = pi.MT, pi.PHILOX
BRINK_KINDS = ("no_hidden", "last_collapse", "penalty", "penalty_negative", "tie", "all_refunded", "clip")


def max_ref(N):
    return 4 if N <= 5 else 2


# ------------------------------------------------------------------------------------------ pieces
def _start(state):
    assert state["hand"] == NONE and state["phase"] == 0 and len(state["disc"]) >= 1, "inject into a freshly dealt game"
    return (np.array(state["cards"], dtype=np.int8), np.array(state["masked"], dtype=np.int8), [int(x) for x in state["draw"]],
            [int(x) for x in state["disc"]])


def _done(cards, masked, draw, disc, hand, player, phase):
    assert len(disc) >= 1 and len(draw) + len(disc) >= pi.MIN_PILE and len(disc) <= 150
    return (np.ascontiguousarray(cards, dtype=np.int8), np.ascontiguousarray(masked, dtype=np.int8), np.asarray(draw, dtype=np.int8),
            np.asarray(disc, dtype=np.int8), int(hand), int(player), int(phase))


def _col(c):
    return slice(3 * c, 3 * c + 3)


def _refund(cards, masked, disc, p, c):
    cards[p, _col(c)], masked[p, _col(c)] = REFUNDED, C
    disc[-1:-1] = [0, 0, 0]  # (under the top)


def _unequal(cards, p, c):
    """An open column must not be three equal cards (that is the pending family)."""
    t = cards[p, _col(c)]
    if t[0] == t[1] == t[2]:
        t[2] = t[2] + 1 if t[2] < 12 else 11


def _open_all(cards, masked, p):
    for c in range(4):
        if masked[p, 3 * c] != C:
            masked[p, _col(c)] = O
            _unequal(cards, p, c)


def _pattern(cards, p, rng, low, high):
    """Seat p holds random cards low .. high, no column of three equal ones."""
    cards[p] = rng.integers(low, high + 1, size=12)
    for c in range(4):
        _unequal(cards, p, c)


def _late_column(cards, masked, rng, p, c, kind):
    s = _col(c)
    if kind == 0:    # two equal open, the third equal and hidden
        cards[p, s] = rng.integers(-2, 13)
        masked[p, s] = O
        masked[p, 3 * c + int(rng.integers(0, 3))] = H
    elif kind == 1:  # two equal open, the third open and different
        v = int(rng.integers(-2, 13))
        w = int(rng.integers(-2, 12))
        cards[p, s] = v
        cards[p, 3 * c + int(rng.integers(0, 3))] = w + (w >= v)
        masked[p, s] = O
    elif kind == 2:  # all open
        masked[p, s] = O
        _unequal(cards, p, c)
    elif kind == 3:  # one hidden
        masked[p, s] = O
        masked[p, 3 * c + int(rng.integers(0, 3))] = H
    # kind 4: as dealt


def _late_boards(cards, masked, disc, rng, N, acting=None, acting_k=None, acting_kinds=()):
    """acting_k: that many refunded columns (at most max_ref) on the acting seat; acting_kinds: the kinds of its first other columns."""
    for p in range(N):
        k = int(rng.integers(0, max_ref(N) + 1))
        if p == acting and acting_k is not None:
            k = min(acting_k, max_ref(N))
        cols = rng.permutation(4)
        for c in cols[:k]:
            _refund(cards, masked, disc, p, int(c))
        for i, c in enumerate(cols[k:]):
            kind = acting_kinds[i] if p == acting and i < len(acting_kinds) else int(rng.integers(0, 5))
            _late_column(cards, masked, rng, p, int(c), kind)


# ------------------------------------------------------------------------------------------ the families
def late(state, rng, N, acting_k=None, acting_kinds=()):
    cards, masked, draw, disc = _start(state)
    _late_boards(cards, masked, disc, rng, N, acting=state["player"], acting_k=acting_k, acting_kinds=acting_kinds)
    return _done(cards, masked, draw, disc, NONE, state["player"], 0)


def late_zeros(state, rng, N):
    cards, masked, draw, disc = _start(state)
    _late_boards(cards, masked, disc, rng, N)
    if N <= 5:
        z = int(rng.integers(40, 61))
        assert z < len(draw)
        del draw[:z]
        disc[-1:-1] = [0] * z
    return _done(cards, masked, draw, disc, NONE, state["player"], 0)


def brink(state, rng, N, kind=None):
    cards, masked, draw, disc = _start(state)
    p0 = state["player"]
    kind = BRINK_KINDS[int(rng.integers(0, len(BRINK_KINDS)))] if kind is None else kind
    assert kind in BRINK_KINDS
    if N == 1 and kind in ("penalty", "penalty_negative", "tie"):
        kind = "no_hidden"      # (one seat is always the lowest)
    if kind == "all_refunded" and 12 * N + 10 > 127:
        kind = "last_collapse"  # (the zeros feature would pass 127)
    q = (p0 + 1 + int(rng.integers(0, max(N - 1, 1)))) % N  # another seat (p0 itself when alone)
    if kind == "no_hidden":
        for p in range(N):
            if p == p0:
                _open_all(cards, masked, p)
            else:
                masked[p] = np.where(rng.random(12) < 0.6, O, masked[p])
                for c in range(4):
                    if (masked[p, _col(c)] == O).all():
                        _unequal(cards, p, c)
    elif kind == "last_collapse":
        c0 = int(rng.integers(0, 4))
        others = [c for c in rng.permutation(4) if c != c0]
        for c in others[:int(rng.integers(0, min(2, max_ref(N)) + 1))]:
            _refund(cards, masked, disc, p0, int(c))
        _open_all(cards, masked, p0)
        cards[p0, _col(c0)] = rng.integers(-2, 13)
        masked[p0, 3 * c0 + int(rng.integers(0, 3))] = H
    elif kind in ("penalty", "penalty_negative"):
        if kind == "penalty":
            _pattern(cards, p0, rng, 5, 12), _pattern(cards, q, rng, -2, 4)
        else:  # -8 against -20: the finisher's negative score is doubled
            cards[p0], cards[q] = np.tile([-1, -1, 0], 4), np.tile([-2, -2, -1], 4)
        _open_all(cards, masked, p0)
    elif kind == "tie":
        for p in range(N):
            _pattern(cards, p, rng, 6, 12)
        _pattern(cards, p0, rng, -2, 3)
        cards[q] = cards[p0]
        _open_all(cards, masked, p0)
    elif kind == "all_refunded":
        for p in range(N):
            for c in range(4):
                _refund(cards, masked, disc, p, c)
    elif kind == "clip":
        for p in range(N):
            cards[p] = np.concatenate([rng.permutation([12, 12, 11]) for _ in range(4)])  # 140 open, 128 and more with one hidden
            masked[p] = O
            if p == p0 or rng.random() < 0.5:
                masked[p, int(rng.integers(0, 12))] = H
    return _done(cards, masked, draw, disc, NONE, p0, 0)


def pending(state, rng, N, columns=None):
    cards, masked, draw, disc = _start(state)
    p0 = state["player"]
    j = int(rng.integers(1, 4)) if columns is None else columns
    cols = [int(c) for c in rng.permutation(4)]
    for c in cols[:j]:
        cards[p0, _col(c)], masked[p0, _col(c)] = rng.integers(-2, 13), O
    masked[p0, _col(cols[3])] = H  # (the seat can still play)
    return _done(cards, masked, draw, disc, NONE, p0, 0)


def mixed(state, rng, N):
    """The rollout cases' family: late boards, a share of the others per game."""
    u = rng.random()
    if u < 0.58:
        return late(state, rng, N)
    if u < 0.70:
        return late_zeros(state, rng, N)
    if u < 0.90:
        return brink(state, rng, N)
    return pending(state, rng, N)


def brink_only(state, rng, N):
    return brink(state, rng, N)


for _f in (late, late_zeros, brink, pending, mixed, brink_only):
    _f.whole_state = True  # (pile_inject.inject: the function returns the whole state)


def with_hand(board, rng, value=None):
    """The same board in the place phase: the top of the draw pile in the hand (`value`: that card instead - the count stays).  Only
    where the acting seat has a hidden card: without one the reference ends the game at the draw."""
    cards, masked, draw, disc, hand, player, phase = board
    if not (masked[player] == H).any() or len(draw) < 1 or len(draw) + len(disc) - 1 < pi.MIN_PILE:
        return board
    return _done(cards, masked, draw[:-1], disc, int(draw[-1]) if value is None else value, player, 1)


# ------------------------------------------------------------------------------------------ what every injected state must satisfy
def observation_histograms(cards, masked, disc):
    """obs[2:17] in both observation modes (skyjo.py:236-248): the discard pile alone, and with every open card."""
    ind = np.bincount(np.asarray(disc, dtype=np.int64) + 2, minlength=15)
    return ind, ind + np.bincount(np.asarray(cards, dtype=np.int64)[np.asarray(masked) == O] + 2, minlength=15)


def check_board(board, N):
    cards, masked, draw, disc, hand, player, phase = board
    assert cards.shape == masked.shape == (N, 12)
    refunded = masked == C
    assert ((cards == REFUNDED) == refunded).all() and (cards[~refunded] >= -2).all() and (cards[~refunded] <= 12).all()
    assert (refunded.reshape(N, 4, 3).all(axis=2) == refunded.reshape(N, 4, 3).any(axis=2)).all()  # whole columns
    assert int((~refunded).sum()) + len(draw) + len(disc) + (hand != NONE) == 150
    assert len(disc) >= 1 and len(draw) + len(disc) >= pi.MIN_PILE and len(disc) <= 150
    assert all(-2 <= int(x) <= 12 for x in draw) and all(-2 <= int(x) <= 12 for x in disc)
    for hist in observation_histograms(cards, masked, disc):
        assert hist.max() <= 127, hist
    assert 0 <= player < N and phase in (0, 1) and (hand == NONE) == (phase == 0)


# ------------------------------------------------------------------------------------------ what a segment reached (oracle only)
def games_view(ora):
    """The oracle's games as one live structured array (no copy)."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return np.ctypeslib.as_array(ora.v.contents.games, shape=(ora.num_envs,))


def raw_scores(cards):
    """skyjo.py:477-493 before the penalty: [..., N, 12] -> [..., N]."""
    t = np.asarray(cards, dtype=np.int64).reshape(cards.shape[:-1] + (4, 3))
    return np.where(t.min(axis=-1) != t.max(axis=-1), t.sum(axis=-1), 0).sum(axis=-1)


REACH = ("rows_ref2", "rows_ref3", "rows_ref4", "collapses", "multi_collapses", "ends", "ends_by_collapse", "ends_penalty",
         "ends_negative_penalty", "ends_tie", "rows_clip", "rows_hist40", "hist_max", "reshuffles")


def record_reach(reach, obs, agent, N, indirect):
    """Counts over records [..., D]: refunded columns the acting seat shows, the clip of obs[0], histogram features."""
    obs, agent = np.asarray(obs), np.asarray(agent).astype(np.int64)
    if indirect:
        own = obs[..., 19:31]
    else:
        own = np.take_along_axis(obs[..., 19:].reshape(obs.shape[:-1] + (N, 12)), agent[..., None, None], axis=-2)[..., 0, :]
    k = (own == REFUNDED).sum(axis=-1) // 3
    for n in (2, 3, 4):
        reach[f"rows_ref{n}"] += int((k == n).sum())
    if N >= 2:
        reach["rows_clip"] += int((obs[..., 0] == 127).sum())
    reach["rows_hist40"] += int((obs[..., 2:17].max(axis=-1) >= 40).sum())
    reach["hist_max"] = max(reach["hist_max"], int(obs[..., 2:17].max()))


class Reach:
    """pile_inject.oracle_segment's probe: looks at the oracle's games after every iteration of a compared segment."""

    def __init__(self, ora):
        self.ora, self.G, self.N = ora, games_view(ora), ora.num_players
        self.n = {k: 0 for k in REACH}
        self.prev = None

    def _now(self):
        G, N = self.G, self.N
        return dict(masked=G["players_masked"][:, :N].copy(), cards=G["players_cards"][:, :N].copy(), episode=G["episode"].copy(),
                    over=G["is_terminated"].copy(), resh=G["reshuffles_total"].copy())

    def begin(self):
        """After the injection, before the segment."""
        self.prev = self._now()
        self.by_collapse = np.zeros((self.ora.num_envs, self.N), dtype=bool)  # the seat's last hidden card went into a collapse

    def __call__(self, t):
        if t < 0:  # (pile_inject.play: the games as injected)
            return self.begin()
        a, b, n, N = self.prev, self._now(), self.n, self.N
        same = a["episode"] == b["episode"]
        self.by_collapse[~same] = False
        cols_a = (a["masked"] == C).sum(axis=2) // 3
        cols_b = (b["masked"] == C).sum(axis=2) // 3
        grown = np.where(same[:, None], cols_b - cols_a, 0)
        n["collapses"] += int((grown > 0).sum())
        n["multi_collapses"] += int((grown > 1).sum())
        hid_a, hid_b = (a["masked"] == H).sum(axis=2), (b["masked"] == H).sum(axis=2)
        last = same[:, None] & (hid_a > 0) & (hid_b == 0)
        self.by_collapse |= last & ~((a["masked"] == H) & (b["masked"] == O)).any(axis=2)
        ended = same & (a["over"] == 0) & (b["over"] != 0)
        for g in np.flatnonzero(ended):
            fin = int(self.G["exp_player"][g])
            raw = raw_scores(b["cards"][g])
            n["ends"] += 1
            n["ends_by_collapse"] += int(self.by_collapse[g, fin])
            if N >= 2:
                n["ends_penalty"] += int(raw.min() != raw[fin])
                n["ends_negative_penalty"] += int(raw.min() != raw[fin] and raw[fin] < 0)
                n["ends_tie"] += int((raw == raw.min()).sum() >= 2)
        n["reshuffles"] += int((b["resh"] - a["resh"]).sum())
        self.prev = b

    def records(self, seg, indirect):
        record_reach(self.n, seg["observations"], seg["agent"], self.N, indirect)


def required(N, table):
    """The counts that must be above zero in a case of table 2 (every action) or 3 (rollout forms)."""
    need = ["rows_ref2"] if N > 5 else ["rows_ref3", "rows_ref4"]
    need += ["collapses", "multi_collapses", "rows_hist40"]
    if N >= 2:
        need += ["ends_penalty", "ends_tie", "rows_clip"]
    if table == 3:
        need += ["ends_by_collapse"]  # (one step cannot both collapse a seat's last hidden card and reach its next draw)
    return need


# ------------------------------------------------------------------------------------------ table 2: every action from every board
ACTIONS = np.arange(-2, 29, dtype=np.int32)  # 26 actions and five out of range
BOARDS = 40
ILLEGAL = ("reveal_open", "reveal_refunded", "place_on_refunded", "draw_while_holding", "place_without_hand", "range_draw", "range_place")
# (recipe, phase): the boards a case cycles through - all three families in both phases
RECIPES = (("late", 0), ("late", 1), ("late_ref3", 1), ("late_ref3", 0), ("late_ref4", 0), ("late_hit", 1), ("late_zeros", 0), ("late_zeros", 1),
           ("no_hidden", 0), ("last_collapse", 0), ("last_collapse", 1), ("penalty", 0), ("penalty_negative", 0), ("tie", 0), ("all_refunded", 0),
           ("clip", 0), ("clip", 1), ("pending1", 0), ("pending1", 1), ("pending2", 1), ("pending3", 1), ("pending3", 0), ("late", 1), ("late", 0),
           ("late_ref3", 1))


def recipe_board(recipe, phase, state, rng, N):
    value = None
    if recipe == "late":
        b = late(state, rng, N)
    elif recipe == "late_ref3":   # three refunded columns (two from six players on) and one with a hidden card
        b = late(state, rng, N, acting_k=3, acting_kinds=(3, 3))
    elif recipe == "late_ref4":
        b = late(state, rng, N, acting_k=4)
    elif recipe == "late_hit":    # a column of two equal open cards and a different one, a column with a hidden card, the value in the hand
        b = late(state, rng, N, acting_k=2, acting_kinds=(1, 3))
        cards, masked, p0 = b[0], b[1], b[5]
        c = next(c for c in range(4) if masked[p0, 3 * c] == O and len(set(cards[p0, _col(c)])) == 2 and (masked[p0, _col(c)] == O).all())
        t = [int(x) for x in cards[p0, _col(c)]]
        value = max(t, key=t.count)
    elif recipe == "late_zeros":
        b = late_zeros(state, rng, N)
    elif recipe.startswith("pending"):
        b = pending(state, rng, N, columns=int(recipe[-1]))
    else:
        b = brink(state, rng, N, kind=recipe)
    return with_hand(b, rng, value) if phase else b


def oracle_full_state(ora, g):
    s, N = pi.oracle_state(ora, g), ora.num_players
    G = ora.game(g)
    s.update(is_terminated=bool(G.is_terminated), num_refunded=np.array(G.num_refunded[:N]), num_placed=np.array(G.num_placed[:N]),
             final_score=np.array(G.final_score[:N]))
    return s


def _same_full_state(e, o, tag):
    for k in ("cards", "masked", "draw", "disc", "num_refunded", "num_placed"):
        np.testing.assert_array_equal(e[k], o[k], err_msg=f"{tag}: {k}")
    for k in ("hand", "player", "phase", "is_terminated", "done", "episode_steps"):
        assert e[k] == o[k], (tag, k, e[k], o[k])
    if o["is_terminated"]:
        np.testing.assert_array_equal(e["final_score"], o["final_score"], err_msg=f"{tag}: final_score")


def _same_records(o, ora, acts, tag):
    obs, mask, agent, phase = ora.observe()
    for k, want in (("observations", obs), ("action_mask", mask), ("agent", agent), ("phase", phase), ("done", ora.dones), ("status", ora.status),
                    ("action", np.asarray(acts, dtype=np.int8))):  # (include/skyjo_vec.h: -2 an action outside 0 .. 25, -1 none)
        np.testing.assert_array_equal(getattr(o, k), want, err_msg=f"{tag}: {k}")


def every_action(ora, seed, indirect, eng=None, boards=BOARDS):
    """One engine / one OracleVec of boards x 31 games: game (b, a) holds board b and gets action a in -2 .. 28.  Seed -> the boards ->
    ONE step (with auto_reset one more, which deals the finished games again).  With an engine: record, rewards, the state of every game
    and the counters == the oracle's.  Returns the Reach-style counts and the illegal categories met."""
    N, A = ora.num_players, len(ACTIONS)
    B = boards * A
    assert ora.num_envs == B
    ora.seed(None, seed)
    if eng is not None:
        eng.seed(None, seed)
    dealt = [pi.oracle_state(ora, g) for g in range(B)]
    episodes = [0] * B
    if eng is not None:
        for g in range(B):
            se = eng.get_state(g)
            pi._same_state(se, dealt[g], f"dealt state of game {g}")
            episodes[g] = se["episode"]
    held = []
    for b in range(boards):
        recipe, phase = RECIPES[b % len(RECIPES)]
        board = recipe_board(recipe, phase, dealt[b * A], np.random.default_rng([seed, b]), N)
        check_board(board, N)
        held.append(board)
        for g in range(b * A, (b + 1) * A):
            assert dealt[g]["episode_steps"] == 0 and dealt[g]["reshuffles"] == 0 and not dealt[g]["done"]
            ora.set_state(g, *board)
            if eng is not None:
                eng.set_state(g, *board, episode=episodes[g])
    acts = np.tile(ACTIONS, boards)
    obs, mask, agent, phase = ora.observe()
    if eng is not None:
        o = eng.observe_host()
        for k, want in (("observations", obs), ("action_mask", mask), ("agent", agent), ("phase", phase)):
            np.testing.assert_array_equal(getattr(o, k), want, err_msg=f"before the step: {k}")
    n = {k: 0 for k in REACH + ILLEGAL}
    record_reach(n, obs, agent, N, indirect)
    legal = np.array([0 <= a <= 25 and mask[g, a] != 0 for g, a in enumerate(acts)])
    for g in np.flatnonzero(~legal):
        a, m = int(acts[g]), held[g // A][1][agent[g]]
        if phase[g]:
            kind = ("range_place" if not 0 <= a <= 25 else "draw_while_holding" if a >= 24 else
                    "reveal_open" if a >= 12 and m[a - 12] == O else "reveal_refunded" if a >= 12 else "place_on_refunded")
            assert kind != "place_on_refunded" or m[a] == C
        else:
            kind = "range_draw" if not 0 <= a <= 25 else "place_without_hand"
        n[kind] += 1
    view = games_view(ora)
    before = dict(masked=view["players_masked"][:, :N].copy())
    ora.step(acts)
    cols = ((view["players_masked"][:, :N] == C).sum(axis=2) - (before["masked"] == C).sum(axis=2)) // 3
    n["collapses"], n["multi_collapses"] = int((cols > 0).sum()), int((cols > 1).sum())
    for g in np.flatnonzero(view["is_terminated"] != 0):
        raw, fin = raw_scores(view["players_cards"][g, :N]), int(view["exp_player"][g])
        n["ends"] += 1
        if N >= 2:
            n["ends_penalty"] += int(raw.min() != raw[fin])
            n["ends_negative_penalty"] += int(raw.min() != raw[fin] and raw[fin] < 0)
            n["ends_tie"] += int((raw == raw.min()).sum() >= 2)
    oc = ora.counters()
    assert oc["illegal"] == int((~legal).sum()) == sum(n[k] for k in ILLEGAL)
    if eng is not None:
        o = eng.step_host(acts)
        _same_records(o, ora, np.where((acts >= 0) & (acts <= 25), acts, -2), "the step")
        rew, sc, done = eng.rewards_host()
        dn = ora.dones.astype(bool)
        np.testing.assert_array_equal(done.astype(bool), dn)
        np.testing.assert_array_equal(rew[dn], ora.rewards[dn], err_msg="rewards of the games that are done")
        for g in range(B):
            _same_full_state(eng.get_state(g), oracle_full_state(ora, g), f"game {g} (board {g // A}, action {int(acts[g])})")
        c = eng.counters()
        for k in ("steps", "episodes", "illegal", "resets", "sum_len", "reshuffles"):
            assert c[k] == oc[k], (k, c[k], oc[k])
        assert c["illegal"] == int((~legal).sum())
        score, refunded = ora.seat_sums()
        np.testing.assert_array_equal(c["sum_score"], score)
        np.testing.assert_array_equal(c["sum_refunded"], refunded)
        if ora.v.contents.auto_reset:
            again = np.full(B, 24, dtype=np.int32)
            ora.step(again)
            o = eng.step_host(again)
            _same_records(o, ora, np.where(dn, -1, again), "the step after")
            assert (o.status[dn] == pi.ST_RESET).all() and dn.any()
            for g in np.flatnonzero(dn):
                _same_full_state(eng.get_state(int(g)), oracle_full_state(ora, int(g)), f"game {g} dealt again")
            c, oc = eng.counters(), ora.counters()
            for k in ("steps", "episodes", "illegal", "resets", "sum_len", "reshuffles"):
                assert c[k] == oc[k], (k, c[k], oc[k])
        eng.check_error()
    return n


# id: players, rng mode, indirect observation, dealing form, auto_reset
ACTION_CASES = {}
for _N, _pairs in ((2, ((MT, "in line"), (PHILOX, "two streams"))), (3, ((PHILOX, "in line"), (MT, "two streams"))), (4, ((MT, "two streams"), (PHILOX, "in line"))),
                   (1, ((PHILOX, "two streams"), (MT, "in line"))), (5, ((MT, "in line"), (PHILOX, "two streams"))), (12, ((PHILOX, "in line"), (MT, "two streams")))):
    for _ind, (_mode, _form) in zip((True, False), _pairs):
        for _ar in (False, True):
            ACTION_CASES["N%d_%s_%s_%s_%s" % (_N, "ind" if _ind else "dir", "px" if _mode else "mt", _form.replace(" ", ""), "autoreset" if _ar else "stay")] = (_N, _mode, _ind, _form, _ar)
ACTION_SEED = 17


# ------------------------------------------------------------------------------------------ table 3: every rollout form
# id: players, rng mode, indirect observation, games, dealing form, dealing interval, options, record layout (as pile_inject.ROLLOUT_CASES)
ROLLOUT_CASES = {
    "inline8_N2_mt_ind": (2, MT, True, 320, "in line", 8, {}, "row-major"),
    "inline8_N3_px_dir": (3, PHILOX, False, 320, "in line", 8, {}, "row-major"),
    "inline8_N4_mt_dir_300": (4, MT, False, 300, "in line", 8, {}, "row-major"),
    "inline1000_N3_mt_ind": (3, MT, True, 320, "in line", 1000, {}, "row-major"),
    "inline1000_N4_px_ind": (4, PHILOX, True, 320, "in line", 1000, {}, "row-major"),
    "worklist8_N2_px_dir": (2, PHILOX, False, 320, "in line", 8, {"work_list": 1}, "row-major"),
    "worklist8_N4_mt_ind": (4, MT, True, 320, "in line", 8, {"work_list": 1}, "row-major"),
    "two8_N2_mt_dir": (2, MT, False, 320, "two streams", 8, {}, "row-major"),
    "two8_N3_mt_ind": (3, MT, True, 320, "two streams", 8, {}, "row-major"),
    "two8_N4_px_dir": (4, PHILOX, False, 320, "two streams", 8, {}, "row-major"),
    "unpipelined8_N3_mt_dir": (3, MT, False, 320, "two streams", 8, {"unpipelined": 1}, "row-major"),
    "unpipelined8_N2_px_ind": (2, PHILOX, True, 320, "two streams", 8, {"unpipelined": 1}, "row-major"),
    "one8_S1_N2_mt_ind": (2, MT, True, 320, "one kernel", 8, {"cycle_s": 1}, "row-major"),
    "one8_S2_N3_px_ind": (3, PHILOX, True, 320, "one kernel", 8, {"cycle_s": 2}, "row-major"),
    "one8_S4_N4_mt_dir": (4, MT, False, 320, "one kernel", 8, {"cycle_s": 4}, "row-major"),
    "one8_S2_N4_mt_ind_300": (4, MT, True, 300, "one kernel", 8, {"cycle_s": 2}, "row-major"),
    "one40_S4_N3_mt_dir": (3, MT, False, 320, "one kernel", 40, {"cycle_s": 4}, "row-major"),
    "one8_max1_N2_px_dir": (2, PHILOX, False, 320, "one kernel", 8, {"max_cycles": 1}, "row-major"),
    "one8_max16_N4_px_ind": (4, PHILOX, True, 320, "one kernel", 8, {"max_cycles": 16}, "row-major"),
    "one8_planar_N3_mt_dir": (3, MT, False, 320, "one kernel", 8, {}, "tile-planar"),
    "one8_planar_N4_px_ind_300": (4, PHILOX, True, 300, "one kernel", 8, {"cycle_s": 2}, "tile-planar"),
    "one8_planar_N2_mt_ind": (2, MT, True, 320, "one kernel", 8, {}, "tile-planar"),
    "one8_planar_all_N3_px_ind": (3, PHILOX, True, 320, "one kernel", 8, {}, "tile-planar-all"),
    "one8_planar_all_N4_mt_ind": (4, MT, True, 320, "one kernel", 8, {}, "tile-planar-all"),
    "inline8_N5_mt_ind": (5, MT, True, 320, "in line", 8, {}, "row-major"),        # the generic kernels
    "two8_N12_mt_dir_128": (12, MT, False, 128, "two streams", 8, {}, "row-major"),  # max_ref 2; reshuffles walk piles that hold collapse zeros
}
SNAPSHOT_CASE = (3, MT, False, 320, "one kernel", 8)
COLLECT_CASE = (3, MT, True, 320, 40)  # step_collect in a device loop on the brink family: players, rng mode, indirect, games, steps


def rollout_sets():
    """(players, generator, games): what the oracle's side of a rollout case depends on (not the observation mode - the policy sees
    masks only -, not the dealing form, the options or the record layout)."""
    return sorted({(c[0], c[1], c[3]) for c in ROLLOUT_CASES.values()} | {SNAPSHOT_CASE[:2] + (SNAPSHOT_CASE[3],)})


def play(ora, indirect, eng=None, rounds=2, family=mixed, on_segment=None):
    """pile_inject.play with a board family: warm-up, then `rounds` x [reset of all games -> a board into every game -> ITERS compared
    iterations].  Returns (the rounds of pile_inject.play, the Reach counts over all of them)."""
    reach = Reach(ora)

    def seg_done(r, st):
        reach.records(st["seg"], indirect)
        if on_segment is not None:
            on_segment(r, st)

    out = pi.play(ora, family, eng=eng, rounds=rounds, on_segment=seg_done, iters=ITERS, probe=reach)
    return out, dict(reach.n)
