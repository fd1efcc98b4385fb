"""numpy restatements of what the arena's learner columns add (TEST INFRASTRUCTURE; include/skyjo_vec.h: skyjo_vec_arena_act,
skyjo_vec_arena_collect, skyjo_vec_rollout_select_seats).  numpy only, nothing from the package; the definitions are
taken from the other restatements - ``net_ref.draw_reference`` for the masked distribution in float64, ``arena_ref.greedy_actions`` for
the greedy rule.  tests/test_arena_collect_ref.py asserts without a GPU what these functions claim; tests/test_gpu_arena_collect.py
compares the kernels with them.  Not collected: a helper.

``logp_at``: the log-probability of a GIVEN action under the masked distribution - the row of ``draw_reference``'s ``logp`` at the
action.  A sampled seat's action is the draw's, a greedy seat's the argmax of the masked logits, a random seat's the draw on 26 zero
logits, for which the value is - log(number of legal actions) (- log 26 for an empty mask: every masked logit is the same FLOAT_MIN).

``value_by_seat``: the acting seat's own value estimate - per seat a column [n] (its value net on every record) or None (0.0).

``select_by_seat``: the rows with every bit of ``require`` in which one of ``seats`` acted, ascending, and the float64 moments of their
advantages.
"""
import numpy as np

from tests import arena_ref, net_ref

TOL_ABS, TOL_REL = 1e-5, 4 * 2.0 ** -24      # net_ref.check_draw's bound on logp: 1e-5 + 4 x 2^-24 |logp_ref|


def logp_table(logits32, mask01):
    """float64 [n, 26]: ``net_ref.draw_reference``'s log-probabilities of every action (the uniforms play no part in them)."""
    lg = np.asarray(logits32, dtype=np.float32)
    return net_ref.draw_reference(lg, mask01, np.zeros(lg.shape[0], dtype=np.float32), False)["logp"]


def logp_at(logits32, mask01, actions):
    """float64 [n]: the reference log-probability of ``actions[g]`` in row g."""
    a = np.asarray(actions).astype(np.int64)
    return logp_table(logits32, mask01)[np.arange(a.shape[0]), a]


def random_logp(mask01):
    """float64 [n]: a random seat's log-probability, whatever legal action it drew - the reference on 26 zero logits."""
    mask01 = np.asarray(mask01)
    return logp_at(np.zeros(mask01.shape, dtype=np.float32), mask01, np.argmax(mask01 != 0, axis=1))


def greedy_logp(logits32, mask01):
    """(actions int32 [n], float64 [n]): the greedy rule's action and the reference log-probability at it."""
    a = arena_ref.greedy_actions(logits32, mask01)
    return a, logp_at(logits32, mask01, a)


def logp_failures(got, want):
    """The rows of float32 ``got`` outside 1e-5 + 4 x 2^-24 |want| of float64 ``want`` (a non-finite value fails)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.flatnonzero(~(np.abs(got - want) <= TOL_ABS + TOL_REL * np.abs(want)))


def value_by_seat(columns, agent):
    """float32 [n]: ``columns[agent[g]][g]``, 0.0 where the seat's entry is None.  ``columns``: per seat a float32 column [n] or None."""
    agent = np.asarray(agent).astype(np.int64)
    out = np.zeros(agent.shape[0], dtype=np.float32)
    for s, col in enumerate(columns):
        if col is not None:
            rows = agent == s
            out[rows] = np.asarray(col, dtype=np.float32).reshape(-1)[rows]
    return out


def seat_mask(seats):
    m = 0
    for s in seats:
        m |= 1 << int(s)
    return m


def select_by_seat(flags, require, agent, seats, advantages=None):
    """(index int64 ascending, count, (sum, sum of squares) in float64 or None): the rows r with (flags[r] & require) == require whose
    ``agent[r]`` is one of ``seats``; flags / agent / advantages flat [T * B], row r = t * B + b."""
    flags, agent = np.asarray(flags, dtype=np.uint8).reshape(-1), np.asarray(agent).reshape(-1).astype(np.int64)
    bit = np.zeros(256, dtype=bool)
    bit[[int(s) for s in seats]] = True
    index = np.flatnonzero(((flags & require) == require) & bit[agent]).astype(np.int64)
    if advantages is None:
        return index, int(index.size), None
    x = np.asarray(advantages, dtype=np.float32).reshape(-1)[index].astype(np.float64)
    return index, int(index.size), (float(x.sum()), float((x * x).sum()))
