"""tests/pile_inject.py on the CPU, oracle only: the oracle's reshuffle of a large pile against numpy's own legacy stream, what the two
injection families conserve, the condition that keeps tests/test_gpu_reshuffle_forms.py from being vacuous (every injected game
reshuffles inside the compared iterations, for every parameter set that file uses), and that the segment comparison sees a stream
that stands one draw too far - what a missing roll-back of the banked deals would leave behind."""
import ctypes as C

import numpy as np
import pytest

from oracle import skyjo_oracle as so
from tests import pile_inject as pi


def _vec(N, rng_mode, B, indirect=True):
    return so.OracleVec(num_envs=B, **pi.oracle_config(N, rng_mode, indirect))


# ------------------------------------------------------------------------------------------ the oracle's reshuffle against numpy
# 2 .. 7, around a refill of the engine's 16-word ring, the three near-empty sizes without a collapse (150 - 12 N), with one (+ 3), and
# the largest pile the engine's 150-byte buffer can be asked to reshuffle
PILE_SIZES = (2, 3, 4, 5, 6, 7, 15, 16, 17, 33, 64, 100, 102, 105, 114, 117, 126, 129, 150)


@pytest.mark.parametrize("N", [1, 2, 3, 4])
def test_oracle_reshuffle_is_numpys_legacy_shuffle(N):
    """seed_legacy_raw(s), a discard pile of n cards under an empty draw pile, act(player, 24): the new draw pile, the hand card and the
    discard pile are RandomState(s).shuffle of the same int8 array, then drawpile.pop() twice (skyjo.py:135-138, 366) - and the
    stream stands where numpy's stands."""
    gen = np.random.default_rng(100 + N)
    for n in PILE_SIZES:
        for s in (0, 7 + n, 123456):
            g = so.OracleGame(num_players=N, score_penalty=2.0, observe_other_player_indirect=True)
            g.seed_legacy_raw(s)
            pile = gen.integers(-2, 13, size=n).astype(np.int8)
            cards = gen.integers(-2, 13, size=(N, 12)).astype(np.int8)
            masked = np.full((N, 12), 2, dtype=np.int8)
            masked[:, :2] = 1
            player = int(gen.integers(0, N))
            g.set_state(cards, masked, np.zeros(0, np.int8), pile, 15, player, 0)
            assert g.act(player, 24) == 0
            rs = np.random.RandomState(s)
            want = pile.copy()
            rs.shuffle(want)
            drawpile = list(want)
            discard = [drawpile.pop()]
            hand = drawpile.pop()
            got = g.snapshot()
            assert got["hand"] == hand and (got["n_draw"], got["n_disc"]) == (n - 2, 1), (N, n, s)
            np.testing.assert_array_equal(got["draw"], np.array(drawpile, dtype=np.int8), err_msg=f"draw pile N={N} n={n} s={s}")
            np.testing.assert_array_equal(got["disc"], np.array(discard, dtype=np.int8))
            assert g.g.reshuffles == 1 and g.L.sko_rng_next(C.byref(g.g.rng)) == rs.randint(0, 1 << 32, dtype=np.uint32)


# ------------------------------------------------------------------------------------------ what the families conserve
@pytest.mark.parametrize("N", [2, 3, 4])
def test_families_conserve_what_they_say(N):
    B = 320
    for family in pi.FAMILIES:
        ora = _vec(N, pi.MT, B)
        ora.seed(None, 3)
        before = [pi.oracle_state(ora, g) for g in range(B)]
        sizes = pi.inject(family, np.random.default_rng(1), ora)
        kept, totals = set(), set()
        for g in range(B):
            a, b = before[g], pi.oracle_state(ora, g)
            for k in ("cards", "masked"):
                np.testing.assert_array_equal(a[k], b[k])  # the hands stay as dealt
            assert (b["hand"], b["player"], b["phase"]) == (a["hand"], a["player"], a["phase"]) and b["disc"][-1] == a["disc"][-1]
            assert sizes[g] == (len(b["draw"]), len(b["disc"]))
            np.testing.assert_array_equal(b["draw"], a["draw"][len(a["draw"]) - len(b["draw"]):])  # the top of the draw pile stays on top
            pile = np.concatenate([b["draw"], b["disc"]])
            kept.add(len(b["draw"])), totals.add(len(pile))
            if family == "near-empty":
                everything = np.concatenate([b["cards"].ravel(), pile])
                np.testing.assert_array_equal(np.bincount(everything + 2, minlength=15), np.full(15, 10))  # all 150 cards
                np.testing.assert_array_equal(b["disc"], np.concatenate([a["draw"][:len(a["draw"]) - len(b["draw"])], a["disc"]]))
        if family == "near-empty":
            assert kept == set(range(7)) and totals == {150 - 12 * N}, (kept, totals)
        else:
            assert kept == {0, 1, 2} and totals == {3, 4, 6}, (kept, totals)
            assert min(totals) >= pi.MIN_PILE + 1  # (one card may be in a hand when the draw pile runs out)


# ------------------------------------------------------------------------------------------ the GPU file's condition
ROLLOUT_SETS = sorted({(c[0], c[1], c[3], c[4]) for c in pi.ROLLOUT_CASES.values()} | {(c[0], c[1], c[3], c[4]) for c in pi.SNAPSHOT_CASES.values()})


@pytest.mark.parametrize("N,rng_mode,B,family", ROLLOUT_SETS, ids=["N%d_%s_%d_%s" % (s[0], "px" if s[1] else "mt", s[2], s[3]) for s in ROLLOUT_SETS])
def test_every_injected_game_reshuffles_inside_the_compared_iterations(N, rng_mode, B, family):
    """For every (players, generator, batch, family) the GPU file runs - the trajectories depend on nothing else: not on the observation,
    the dealing form or the record layout -, in BOTH rounds: every game reshuffles at least once inside the compared segment, keep = 0
    occurs (the first pile draw reshuffles), the in-episode count stays below 255 (the engine's H_RESH saturates there, the oracle's
    counter does not), the thin family reaches the reshuffle sessions 1 and 2 of an episode, and near-empty piles are 100 .. 129 cards."""
    rounds = pi.play(_vec(N, rng_mode, B), family)
    assert len(rounds) == 2
    for r, st in enumerate(rounds):
        print(f"N={N} rng={rng_mode} B={B} {family} round {r}: {st['total']} reshuffles, {st['min_per_game']} .. {int(st['per_game'].max())} per game, "
              f"at most {st['max_in_episode']} inside an episode, all games by iteration {st['all_by']}, piles of {st['sizes']} cards, "
              f"{st['redealt_after_rollback']} games dealt again after a reshuffle, {st['finished']} stand finished")
        assert st["min_per_game"] >= 1 and st["all_by"] <= pi.FAMILIES[family][1], (r, st["min_per_game"], st["all_by"])
        assert st["total"] >= B and st["max_in_episode"] < 255
        assert any(n_draw == 0 for n_draw, _ in st["injected"].values())
        if family == "thin":
            assert st["max_in_episode"] >= 3 and st["sizes"][0] >= pi.MIN_PILE + 1
        else:
            assert 100 <= st["sizes"][0] and st["sizes"][1] <= 150 - 12 * N + 3, st["sizes"]


CALLER_SETS = sorted({(c[0], c[1], c[3], pi.CALLER_GAMES, pi.CALLER_STEPS, False) for c in pi.CALLER_CASES.values()}
                     | {(pi.COLLECT_CASE[0], pi.COLLECT_CASE[1], pi.COLLECT_CASE[3], pi.COLLECT_CASE[4], pi.COLLECT_CASE[5], True)})


@pytest.mark.parametrize("N,rng_mode,family,B,steps,reveal", CALLER_SETS)
def test_every_injected_game_reshuffles_under_caller_actions(N, rng_mode, family, B, steps, reveal):
    per_game, deepest, ends = pi.play_caller(_vec(N, rng_mode, B), family, steps, reveal=reveal)
    print(f"N={N} rng={rng_mode} {family} x {steps} steps: {int(per_game.sum())} reshuffles, {int(per_game.min())} .. {int(per_game.max())} per game, "
          f"at most {deepest} inside an episode, {ends} episode ends")
    assert per_game.min() >= 1 and deepest < 255
    if reveal:
        assert ends > 0  # (the episode-end columns have something to show)


# ------------------------------------------------------------------------------------------ sensitivity
def _first_draw_is_rejected(word, n):
    """rk_interval(n - 1), the first draw of a shuffle of n cards, throws `word` away (legacy masked rejection)."""
    top = n - 1
    mask = top
    for sh in (1, 2, 4, 8, 16):
        mask |= mask >> sh
    return (word & mask) > top


@pytest.mark.parametrize("shift", [1, 300])
@pytest.mark.parametrize("N", [2, 3, 4])
def test_a_stream_that_stands_too_far_is_seen_in_every_game(N, shift):
    """Two oracles from the same injected state; in one every game's MT19937 stream is advanced first (sko_rng_next) - a reshuffle drawn
    from a position AFTER the banked deals is what a missing roll-back produces.  shift 300 (about one deal's worth of draws): the
    comparison reports EVERY game.  shift 1: it reports every game but those whose next word the shuffle's first rk_interval rejects -
    2, 14 or 26 words in 128 for piles of 126, 114 or 102 cards; the shuffle then starts on the word the advanced stream starts on,
    and the two games are the same from there on, stream position included.  That set is computed here, word by word, and the
    reported set must be exactly the rest."""
    B, family = 320, "near-empty"
    iters = pi.FAMILIES[family][1]
    segs, words = [], None
    for shifted in (False, True):
        ora = _vec(N, pi.MT, B)
        ora.seed(None, pi.SEED)
        ora.rollout(pi.WARMUP, pi.POLICY_SEED)
        ora.reset()
        pi.inject(family, np.random.default_rng(pi.INJECT_SEEDS[0]), ora)
        if shifted:
            for g in range(B):
                for _ in range(shift):
                    ora.L.sko_rng_next(C.byref(ora.game(g).rng))
        else:  # the word every game's stream gives next (on a copy)
            words = [int(ora.L.sko_rng_next(C.byref(so._Rng.from_buffer_copy(ora.game(g).rng)))) for g in range(B)]
        segs.append(pi.oracle_segment(ora, iters, pi.POLICY_SEED, range(B)))
    assert not pi.differences(segs[0], segs[0])
    # the stream is used by nothing before a game's first reshuffle: no game is dealt again before it
    first = {}
    for t, g, n in segs[0]["resh_sizes"]:
        first.setdefault(g, (t, n))
    assert len(first) == B
    for g, (t, n) in first.items():
        assert not (segs[0]["status"][:t + 1, g] == pi.ST_RESET).any(), g
    unseen = {g for g, (t, n) in first.items() if _first_draw_is_rejected(words[g], n)} if shift == 1 else set()
    d = pi.differences(segs[0], segs[1])
    rec, piles = d.get("records", {}), set(d.get("piles", []))
    fields, when = {}, []
    for g, (t, k) in rec.items():
        fields[k] = fields.get(k, 0) + 1
        when.append(t - first[g][0])
    print(f"N={N} shift={shift}: {len(rec)} of {B} games first differ in a record ({fields}; {sum(1 for w in when if w == 0)} in the record of the reshuffling "
          f"iteration itself, the latest {max(when)} iterations after it), {len(piles - set(rec))} only in the piles, {len(piles)} in the piles at all, "
          f"{len(unseen)} with a rejected first word")
    assert set(rec) | piles == set(range(B)) - unseen, (sorted(set(range(B)) - unseen - set(rec) - piles), sorted((set(rec) | piles) & unseen))
    assert shift != 1 or 0 < len(unseen) < B // 3
    with pytest.raises(AssertionError):
        pi.assert_same(segs[0], segs[1], "shifted stream")
