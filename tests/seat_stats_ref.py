"""The reference for the per-seat float64 sums of ``counters()`` - ``sum_score``, ``sum_reward``, ``sum_reward_sq``, ``sum_refunded``
(include/skyjo_vec.h) - built from the CPU oracle alone (TEST INFRASTRUCTURE): an EPISODE LOG, and the rule the sums are held to.

The log.  ``EpisodeLog`` drives an ``OracleVec`` ONE lockstep iteration at a time - with the restated on-device policy (``rollout``) or
with the caller's actions (``step``) - and after every iteration appends every episode that ended in it: game, iteration, kind
(``NATURAL``: the game's own end, ``ILLEGAL``: an illegal action), the final rewards, final scores and refunded counts of all seats, and
(not a sum, but what the case tables ask about) the seat that ended it and whether a finisher was penalised.  An episode ended in an
iteration iff its game was not ``done`` before it and is ``done`` after it.  Under auto-reset a finished game stands ``done`` for exactly one
iteration (the next one re-deals it), so nothing is missed and nothing is seen twice; without auto-reset a finished game stays ``done``,
and steps (``SKYJO_ST_NOOP_DONE``) and ``SKYJO_ACTION_SKIP`` on it are no transition: they add nothing.  A natural end counts for all four
sums; an illegal end for ``sum_reward`` and ``sum_reward_sq`` only, and there only for the offender (the other seats' reward is 0.0).

The rule, ``check(counters, log, N)``.  No tolerance in it is measured; both regimes are derived.

* EXACT - ``score_penalty = 2``, ``mean_reward = 1``, ``reward_refunded = 2**-10``, ``illegal_reward = -0.5`` and N in {1, 2, 4, 8}: ``==``.
  A raw score is an integer, at most 12 cards x 12 = 144 in magnitude, the penalised finisher's twice that: |d| <= 288 = 2^8.2, a
  multiple of 1.  The mean of N such scores, N a power of two up to 8, is a multiple of 1/8 and exact.  A reward is
  (-d + mean) + 1 + refunded * 2^-10 with refunded <= 12: a multiple of 2^-10, |r| <= 288 + 288 + 1 + 12 * 2^-10 < 2^10, so r = k * 2^-10 with
  |k| < 2^20 - exact, in any association.  Its square is k^2 * 2^-20 with k^2 < 2^40 - exact as one double product.  The illegal reward is
  -512 * 2^-10, its square 2^18 * 2^-20.  A sum of n such numbers, in ANY order and through any partial sums, stays a multiple of the
  unit below n * max|x|; it is exact as long as  n * max|x| / unit < 2^53:  n < 2^33 for rewards and n < 2^13 = 8192 for squares on the
  a-priori bounds, and far more on the values a log really holds (|r| < 2^8: n < 2^17 squares).  ``exact_budget`` computes
  n * max|x| / unit per sum kind FROM THE LOG and ``check`` refuses a log that does not fit - the CPU tests assert it for every case.
* BOUND - every other N and every other setting: the want is ``math.fsum`` of the log's addends (the correctly rounded sum), and the
  engine's sum - n addends in SOME order: per lane, a shuffle tree over the 64 lanes of a tile, over the launches, over the tiles - may
  differ from it by at most  n * 2^-53 * fsum(|x|)  (any order of recursive summation errs by at most (n - 1) u sum|x| + O(u^2), u =
  2^-53; the n-th u covers the second-order term and fsum's own rounding).  That is the allowance tests/test_gpu_scoring_geometry.py
  states for ``sum_score``.  For the squares an addend is r * r formed as ONE double product (the engine's unit is built with
  -ffp-contract=off: a multiply, then an add).
* ``sum_refunded`` is integer-valued and compared with ``==`` in both regimes, and so are the integer counters ``episodes`` and ``illegal``.
"""
import math
from collections import namedtuple

import numpy as np

from oracle import skyjo_oracle as so

NATURAL, ILLEGAL = 0, 1
KINDS = ("sum_score", "sum_reward", "sum_reward_sq", "sum_refunded")
EXACT_SETTINGS = dict(score_penalty=2.0, mean_reward=1.0, reward_refunded=2.0 ** -10, illegal_reward=-0.5)
EXACT_PLAYERS = (1, 2, 4, 8)
UNIT = {"sum_score": 1.0, "sum_reward": 2.0 ** -10, "sum_reward_sq": 2.0 ** -20, "sum_refunded": 1.0}

Episode = namedtuple("Episode", "game iteration kind rewards final_score num_refunded seat penalised")


def is_exact(settings, N):
    return N in EXACT_PLAYERS and all(float(settings[k]) == v for k, v in EXACT_SETTINGS.items())


def _raw_scores(g, N):
    """skyjo.py:488-493 on the oracle's card rows: a column of three equal cards cancels, hidden cards count."""
    out = []
    for p in range(N):
        c = list(g.players_cards[p])
        out.append(sum(0 if c[3 * k] == c[3 * k + 1] == c[3 * k + 2] else c[3 * k] + c[3 * k + 1] + c[3 * k + 2] for k in range(4)))
    return out


class EpisodeLog:
    """``entries``: the episodes ended so far, in the order (iteration, game).  ``settings``: the four reward settings of the oracle."""

    def __init__(self, ora, illegal_reward=None):
        self.ora, self.N = ora, ora.num_players
        if illegal_reward is not None:
            ora.v.contents.illegal_reward = float(illegal_reward)
        c = ora.v.contents
        self.settings = dict(score_penalty=c.score_penalty, mean_reward=c.mean_reward, reward_refunded=c.reward_refunded,
                             illegal_reward=c.illegal_reward)
        self.entries = []
        self.iteration = 0

    @property
    def exact(self):
        return is_exact(self.settings, self.N)

    def _append_ended(self, before):
        ora, N = self.ora, self.N
        after = ora.dones.astype(bool)
        ended = np.flatnonzero(after & ~before)
        if len(ended):
            status, rewards = ora.status, ora.rewards
            for i in ended:
                g = ora.game(int(i))
                kind = ILLEGAL if status[i] == so.ST_ILLEGAL else NATURAL
                assert kind == ILLEGAL or status[i] == so.ST_OK, status[i]
                seat, penalised = int(g.exp_player), False  # the finisher (skyjo.py:350-356: the turn is not advanced) or the offender
                if kind == NATURAL:
                    raw = _raw_scores(g, N)
                    penalised = raw[seat] != min(raw)
                self.entries.append(Episode(int(i), self.iteration, kind, tuple(float(x) for x in rewards[i]),
                                            tuple(float(g.final_score[p]) for p in range(N)),
                                            tuple(int(g.num_refunded[p]) for p in range(N)), seat, penalised))
        self.iteration += 1

    def rollout(self, iters, policy_seed, threads=1):
        """``iters`` lockstep iterations of the restated on-device policy, one at a time; returns the actions [iters, B]."""
        acts = []
        for _ in range(iters):
            before = self.ora.dones.astype(bool)
            acts.append(self.ora.rollout(1, policy_seed, threads=threads, record_actions=True)[0])
            self._append_ended(before)
        return np.stack(acts) if acts else np.zeros((0, self.ora.num_envs), dtype=np.int32)

    def step(self, actions, threads=1):
        """One step with the caller's actions (illegal ones, out-of-range ones, SKYJO_ACTION_SKIP, steps on finished games)."""
        before = self.ora.dones.astype(bool)
        self.ora.step(actions, threads=threads)
        self._append_ended(before)

    def tail(self, start):
        """A log of the entries from index ``start`` on (what the sums hold after ``reset_counters()`` at that point)."""
        t = EpisodeLog.__new__(EpisodeLog)
        t.ora, t.N, t.settings, t.entries, t.iteration = self.ora, self.N, self.settings, self.entries[start:], self.iteration
        return t

    def with_entries(self, entries):
        t = self.tail(0)
        t.entries = list(entries)
        return t


def addends(log, N):
    """{kind: [per seat: list of addends]} - what each of the four sums adds up, episode by episode in the log's order."""
    out = {k: [[] for _ in range(N)] for k in KINDS}
    for e in log.entries:
        for p in range(N):
            r = e.rewards[p]
            if e.kind == NATURAL:
                out["sum_score"][p].append(e.final_score[p])
                out["sum_refunded"][p].append(float(e.num_refunded[p]))
            elif r == 0.0:
                continue  # an illegal end: the offender alone
            out["sum_reward"][p].append(r)
            out["sum_reward_sq"][p].append(r * r)  # ONE double product
    return out


def counts(log):
    return (sum(e.kind == NATURAL for e in log.entries), sum(e.kind == ILLEGAL for e in log.entries))


def exact_budget(log, N):
    """Per kind: (every addend is a multiple of the kind's unit, n * max|x| / unit) over the seats - the exact regime needs True and
    less than 2^53."""
    out = {}
    for k, per_seat in addends(log, N).items():
        u = UNIT[k]
        multiple = all(float(x / u).is_integer() for xs in per_seat for x in xs)
        need = max((len(xs) * max(abs(x) for x in xs) / u for xs in per_seat if xs), default=0.0)
        out[k] = (multiple, need)
    return out


def naive_counters(log, N):
    """The sums of a log taken in the plainest way there is - one float64 accumulator per seat, episode after episode - and the two
    integer counters: a ``counters()`` that ``check`` must accept (the CPU tests), and the base the restated slips are applied to."""
    out = {}
    for k, per_seat in addends(log, N).items():
        acc = np.zeros(N, dtype=np.float64)
        for p, xs in enumerate(per_seat):
            for x in xs:
                acc[p] += x
        out[k] = acc
    out["episodes"], out["illegal"] = counts(log)
    return out


def check(counters, log, N, exact=None):
    """Hold ``counters`` (``SkyjoVecEnv.counters()``, or anything with its keys) to the log; AssertionError names the first sum that
    fails.  Returns {kind: the largest |got - want| / allowance over the seats} (0.0 where the comparison is ``==``): how much of the
    allowance is used - recorded by the tests, never asserted."""
    exact = log.exact if exact is None else exact
    episodes, illegal = counts(log)
    assert int(counters["episodes"]) == episodes, ("episodes", int(counters["episodes"]), episodes)
    assert int(counters["illegal"]) == illegal, ("illegal", int(counters["illegal"]), illegal)
    add = addends(log, N)
    if exact:
        for k, (multiple, need) in exact_budget(log, N).items():
            assert multiple and need < 2.0 ** 53, ("the log does not fit the exact regime", k, multiple, need)
    used = {}
    for k in KINDS:
        got = np.asarray(counters[k], dtype=np.float64)
        assert got.shape == (N,), (k, got.shape)
        used[k] = 0.0
        for p in range(N):
            xs = add[k][p]
            want = math.fsum(xs)
            if exact or k == "sum_refunded":
                assert float(got[p]) == want, (k, "seat", p, "got", float(got[p]), "want", want, "exact")
                continue
            allowance = len(xs) * 2.0 ** -53 * math.fsum(abs(x) for x in xs)
            err = abs(float(got[p]) - want)
            assert err <= allowance, (k, "seat", p, "got", float(got[p]), "want", want, "error", err, "allowance", allowance, "addends", len(xs))
            if allowance > 0.0:
                used[k] = max(used[k], err / allowance)
    return used


def conditions(log, N, num_envs, auto_reset=True, caller=False):
    """What every logged case must meet (decided on the CPU, by the oracle alone); returns the figures the case tables print.
    With auto-reset: at least 3 B ended episodes.  Without: a game has ONE episode, so at most B can end - all B must.  Every seat ends
    an episode as its finisher; with two players and more every seat is penalised once and the seats' sums differ (a sum on the wrong
    seat shows); caller actions bring an illegal end per seat up to four players and at least one overall above that."""
    nat = [e for e in log.entries if e.kind == NATURAL]
    ill = [e for e in log.entries if e.kind == ILLEGAL]
    ended = len(nat) + len(ill)
    if auto_reset:
        assert ended >= 3 * num_envs, (ended, 3 * num_envs)
    else:
        assert len({e.game for e in log.entries}) == ended == num_envs, (ended, num_envs)
    finishers = {e.seat for e in nat}
    assert finishers == set(range(N)), ("finishers", sorted(finishers))
    if N >= 2:
        penalised = {e.seat for e in nat if e.penalised}
        assert penalised == set(range(N)), ("penalised", sorted(penalised))
    if N >= 2:
        # a sum that lands on another seat must show: the seats' scores, rewards and squares differ pairwise; the refunded counts (small
        # integers, up to twelve seats) are not all the same, so that an off-by-one in the seat index - a rotation - changes one
        for k, per_seat in addends(log, N).items():
            sums = [math.fsum(xs) for xs in per_seat]
            if k == "sum_refunded":
                assert len(set(sums)) > 1, (k, sums)
            else:
                assert len(set(sums)) == N, (k, sums)
    if caller:
        offenders = {e.seat for e in ill}
        assert len(ill) >= 1 and (N > 4 or offenders == set(range(N))), ("offenders", sorted(offenders))
    return dict(natural=len(nat), illegal=len(ill), penalised=sum(e.penalised for e in nat))


# ----------------------------------------------------------------------------------------------------------------- restated slips
def _first(entries, pred):
    for j, e in enumerate(entries):
        if pred(e):
            return j
    raise AssertionError("the log holds no episode to apply this slip to")


def slipped_counters(log, N, slip):
    """``naive_counters`` of the log with ONE episode mishandled the way an index slip in the engine would - each must be rejected."""
    E = list(log.entries)
    c = None
    if slip == "seats exchanged":  # two seats' rewards exchanged
        j = _first(E, lambda e: e.kind == NATURAL and e.rewards[0] != e.rewards[1])
        r = list(E[j].rewards)
        r[0], r[1] = r[1], r[0]
        E[j] = E[j]._replace(rewards=tuple(r))
    elif slip == "episode dropped":
        del E[_first(E, lambda e: e.kind == NATURAL)]
    elif slip == "episode twice":
        j = _first(E, lambda e: e.kind == NATURAL)
        E.insert(j, E[j])
    elif slip == "illegal reward one seat on":  # credited to the seat after the offender
        j = _first(E, lambda e: e.kind == ILLEGAL)
        r = [0.0] * N
        r[(E[j].seat + 1) % N] = E[j].rewards[E[j].seat]
        E[j] = E[j]._replace(rewards=tuple(r))
    elif slip == "illegal end scored":  # an illegal end also added to sum_score (what the scores array holds for the game: the
        j = _first(E, lambda e: e.kind == ILLEGAL)  # last finished episode's scores - or, before any, its raw hand)
        c = naive_counters(log.with_entries(E), N)
        sc = E[j].final_score if any(E[j].final_score) else tuple(float(s) for s in _raw_scores(log.ora.game(E[j].game), N))
        assert any(sc)
        c["sum_score"] = c["sum_score"] + np.asarray(sc)
    elif slip == "square of the score":  # reward_sq taken from the score
        j = _first(E, lambda e: e.kind == NATURAL and abs(e.final_score[0]) != abs(e.rewards[0]))
        c = naive_counters(log.with_entries(E), N)
        c["sum_reward_sq"][0] += E[j].final_score[0] * E[j].final_score[0] - E[j].rewards[0] * E[j].rewards[0]
    elif slip == "refunded of the next seat":  # the refunded count of seat p read from seat p + 1
        j = _first(E, lambda e: e.kind == NATURAL and e.num_refunded[0] != e.num_refunded[1 % N])
        c = naive_counters(log.with_entries(E), N)
        c["sum_refunded"][0] += E[j].num_refunded[1 % N] - E[j].num_refunded[0]
    else:
        raise ValueError(slip)
    if c is None:
        c = naive_counters(log.with_entries(E), N)
    c["episodes"], c["illegal"] = counts(log)  # (the integer counters are not what these slips are about)
    return c


SLIPS = ("seats exchanged", "episode dropped", "episode twice", "illegal reward one seat on", "illegal end scored", "square of the score",
         "refunded of the next seat")
