"""Plain-Python restatements of the two scoring functions' float64 arithmetic (TEST INFRASTRUCTURE): the right operation order
(numpy's pairwise sum inside np.mean) and three wrong ones, which tests/golden/scoring_order.npz has to tell apart.

Python floats are IEEE doubles and every ``+``, ``*``, ``/`` below rounds once, so the order written here is the order computed.
A fused multiply-add is restated with exact rationals: ``float(Fraction)`` rounds once, to nearest even."""
from fractions import Fraction


def sum_pairwise(a):
    """np.add.reduce on a contiguous float64 vector of at most 128 elements: left to right below eight, eight partial sums
    combined as a tree from eight on, the tail left to right."""
    n = len(a)
    if n < 8:
        res = 0.0
        for x in a:
            res += x
        return res
    r = [float(x) for x in a[:8]]
    i = 8
    while i < n - (n % 8):
        for j in range(8):
            r[j] += a[i + j]
        i += 8
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for x in a[i:]:
        res += x
    return res


def sum_left(a):
    res = 0.0
    for x in a:
        res += x
    return res


def sum_reversed(a):
    return sum_left(list(a)[::-1])


def sum_wrong_left_from_8(a):
    """WRONG at N >= 8: no pairwise branch."""
    return sum_left(a)


def sum_wrong_reversed_below_8(a):
    """WRONG at N < 8: the last seat first."""
    return sum_reversed(a) if len(a) < 8 else sum_pairwise(a)


def rewards(scores, refunded, mean_reward, reward_refunded, summer=sum_pairwise):
    """_calc_final_rewards (skyjo_env.py:307-312) with the sum of np.mean done by `summer`."""
    scores = [float(x) for x in scores]
    n = len(scores)
    mean = summer(scores) / float(n)
    out = []
    for p in range(n):
        r = (-scores[p] + mean) + mean_reward
        if reward_refunded:
            r += float(int(refunded[p])) * reward_refunded
        out.append(r)
    return out


def raw_scores(hand):
    """Integer scores of an end hand [N][12] (skyjo.py:488-493): columns of three equal cards do not count."""
    out = []
    for row in hand:
        s = 0
        for c in range(4):
            t = [int(x) for x in row[3 * c:3 * c + 3]]
            if min(t) != max(t):
                s += sum(t)
        out.append(s)
    return out


def scores(hand, finisher, penalty):
    """_evaluate_game (skyjo.py:477-498)."""
    s = [float(x) for x in raw_scores(hand)]
    if min(s) != s[finisher]:
        s[finisher] *= penalty
    return s


class _Product:
    """s * penalty not yet rounded: what a contracted multiply-add keeps exact."""

    def __init__(self, s, penalty):
        self.s, self.penalty = float(s), float(penalty)


def _add(x, y):
    """x + y, fused where one operand is an unrounded product."""
    if isinstance(y, _Product):
        x, y = y, x
    if isinstance(x, _Product):
        if isinstance(y, _Product):
            raise AssertionError("only the finisher's score is a product")
        return float(Fraction(x.s) * Fraction(x.penalty) + Fraction(y))
    return x + y


def rewards_wrong_fused(hand, finisher, penalty, refunded, mean_reward, reward_refunded):
    """WRONG: the sum's addition of the penalised score contracted into fma(s, penalty, sum); everything else as it should be."""
    raw = [float(x) for x in raw_scores(hand)]
    sc = scores(hand, finisher, penalty)
    terms = list(sc)
    if min(raw) != raw[finisher]:
        terms[finisher] = _Product(raw[finisher], penalty)
    n = len(terms)
    if n < 8:
        total = 0.0
        for x in terms:
            total = _add(total, x)
    else:
        r = terms[:8]
        total = _add(_add(_add(r[0], r[1]), _add(r[2], r[3])), _add(_add(r[4], r[5]), _add(r[6], r[7])))
        for x in terms[8:]:
            total = _add(total, x)
    if isinstance(total, _Product):  # (one player: never penalised, so never reached; kept total a float for the division)
        total = total.s * total.penalty
    mean = total / float(n)
    out = []
    for p in range(n):
        r = (-sc[p] + mean) + mean_reward
        if reward_refunded:
            r += float(int(refunded[p])) * reward_refunded
        out.append(r)
    return out


def order_sensitive(score_vector):
    """True where np.mean of the vector differs from the left-to-right sum divided by N."""
    v = [float(x) for x in score_vector]
    return sum_pairwise(v) / float(len(v)) != sum_left(v) / float(len(v))
