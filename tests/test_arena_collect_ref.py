"""The restatements of tests/arena_collect_ref.py are what they claim (no GPU): a random seat's log-probability, the greedy seat's,
the value by seat, and the selection by seat as a partition of the unfiltered one."""
import itertools

import numpy as np
import pytest

from tests import arena_collect_ref as acr
from tests import learner_synth, net_ref
from tests import record_ref as ref


def _case(n, seed):
    rng = np.random.default_rng(seed)
    mask, fam = net_ref.mask_rows(n, rng)
    logits, _ = net_ref.logit_rows(n, mask, rng)
    return mask, fam, logits


def test_a_random_seats_logp_is_minus_log_of_the_legal_count():
    mask, fam, _ = _case(900, 1)
    legal = (mask != 0).sum(axis=1)
    assert {0, 1, 2, 26} <= set(legal.tolist())           # the empty mask, a single action, the draw phase, every action
    got = acr.random_logp(mask)
    want = -np.log(np.where(legal > 0, legal, 26).astype(np.float64))
    assert np.abs(got - want).max() <= 1e-12
    # ... at EVERY legal action, not only the first
    table = acr.logp_table(np.zeros(mask.shape, dtype=np.float32), mask)
    on = mask != 0
    assert np.abs(table - want[:, None])[on].max() <= 1e-12
    assert (table[~on & (legal > 0)[:, None]] < -1e30).all()    # a masked action next to a legal one: FLOAT_MIN below it


def test_greedy_logp_is_the_row_maximum_of_the_reference_logp():
    mask, fam, logits = _case(1800, 2)
    a, lp = acr.greedy_logp(logits, mask)
    table = acr.logp_table(logits, mask)
    assert np.array_equal(lp, table.max(axis=1))
    assert np.array_equal(a, np.argmax(table, axis=1))    # the first maximum on a tie ("equal" logits are among the families)
    legal = (mask != 0).any(axis=1)
    assert (mask[legal, a[legal]] != 0).all() and (a[~legal] == 0).all()
    assert (lp <= 0).all() and (lp[(mask != 0).sum(axis=1) == 1] == 0).all()
    # logp_at at an arbitrary legal action agrees with the table, and the probabilities of a row sum to 1
    assert np.abs(np.exp(table).sum(axis=1) - 1.0).max() <= 1e-12
    k = np.argmax((mask != 0)[:, ::-1], axis=1)
    last = np.where(legal, 25 - k, 0)
    assert np.array_equal(acr.logp_at(logits, mask, last), table[np.arange(len(last)), last])


def test_logp_failures_is_check_draws_bound():
    want = np.array([-1.0, -100.0, -1e-3, 0.0])
    edge = acr.TOL_ABS + acr.TOL_REL * np.abs(want)
    assert acr.TOL_ABS == 1e-5 and acr.TOL_REL == 4 * 2.0 ** -24
    assert acr.logp_failures(want + 0.99 * edge, want).size == 0 and acr.logp_failures(want - 0.99 * edge, want).size == 0
    assert acr.logp_failures(want + 1.01 * edge, want).tolist() == [0, 1, 2, 3]
    assert acr.logp_failures(np.array([np.nan, -1.0]), np.array([-1.0, -1.0])).tolist() == [0]


def test_value_by_seat_takes_the_acting_seats_column():
    rng = np.random.default_rng(3)
    n, N = 321, 4
    agent = rng.integers(0, N, size=n)
    cols = [rng.standard_normal(n).astype(np.float32), None, rng.standard_normal((n, 1)).astype(np.float32), rng.standard_normal(n).astype(np.float32)]
    got = acr.value_by_seat(cols, agent)
    for g in range(n):
        c = cols[agent[g]]
        assert got[g] == (0.0 if c is None else np.asarray(c).reshape(-1)[g])
    assert (got[agent == 1] == 0).all() and (agent == 1).any()


@pytest.mark.parametrize("N,indirect", [(3, True), (4, False), (12, False)], ids=lambda v: str(v))
def test_disjoint_seat_sets_partition_the_unfiltered_selection(N, indirect):
    T, B = 3, 130
    rng = np.random.default_rng(40 + N)
    g = ref.geometry(N, indirect)
    rec = learner_synth.records(T, B, g, rng)
    rec[..., g["mask_offset"] + 26] = rng.integers(0, N, size=(T, B))   # every row has a seat below N
    agent = rec[..., g["mask_offset"] + 26].reshape(-1)
    flags = learner_synth.select_flags(T * B, "random", rng)
    adv = learner_synth.select_advantages(T * B, rng)
    for require in (1, 2, 3):
        everything = np.flatnonzero((flags & require) == require)
        index, count, mom = acr.select_by_seat(flags, require, agent, range(N), adv)
        assert np.array_equal(index, everything) and count == everything.size
        parts = [acr.select_by_seat(flags, require, agent, (s,), adv) for s in range(N)]
        assert sum(p[1] for p in parts) == count
        assert np.array_equal(np.sort(np.concatenate([p[0] for p in parts])), everything)
        for p, q in itertools.combinations(parts, 2):
            assert np.intersect1d(p[0], q[0]).size == 0
        for k in (0, 1):                                   # the sums add up (float64 sums of a few hundred terms: to rounding)
            total = sum(p[2][k] for p in parts)
            assert abs(total - mom[k]) <= 4 * count * 2.0 ** -53 * float(np.abs(adv.astype(np.float64) ** (k + 1))[everything].sum())
        for p, s in zip(parts, range(N)):
            assert (agent[p[0]] == s).all() and np.array_equal(p[0], np.sort(p[0]))
        # a mixed set is the union of its seats
        mixed = (0, N - 1)
        idx, cnt, _ = acr.select_by_seat(flags, require, agent, mixed, adv)
        assert np.array_equal(idx, np.sort(np.concatenate([parts[s][0] for s in set(mixed)]))) and cnt == idx.size
    assert acr.seat_mask((0, N - 1)) == 1 | 1 << (N - 1) and acr.seat_mask(range(N)) == (1 << N) - 1


def test_planar_record_numbers_skip_the_padding_slots():
    """Row r of a [T, B] buffer is record (r // B) * tiles * 64 + r % B of the planar buffer: read through ``planar_address`` the agent
    bytes are the row-major ones, although the padding slots of the partial tile hold other (non-zero) bytes."""
    T, B, (N, indirect) = 3, 130, (4, False)
    rng = np.random.default_rng(7)
    g = ref.geometry(N, indirect)
    rec = learner_synth.records(T, B, g, rng)
    planar = learner_synth.to_planar_dirty(rec, rng)
    rb, off = g["record_bytes"], g["mask_offset"] + 26
    tiles = (B + 63) // 64
    flat = planar.reshape(T, -1)
    r = np.arange(T * B)
    got = flat[r // B, ref.planar_address(r % B, off, rb)]
    assert np.array_equal(got, rec[..., off].reshape(-1))
    assert flat.shape[1] == tiles * 64 * rb and tiles * 64 > B
