"""Learner targets (``skyjo_vec_rollout_targets``) without a GPU: the two restatements of
tests/rollout_targets_ref.py against the worked example, against each other on columns the oracle engine generates, against the
rule of ``examples.ppo.compute_returns`` and against the counting identity; and the ABI carries the entry point.

The bound between the float32 recursion (a) and the float64 textbook (b),  4 L 2^-24 M  (L: longest seat trajectory of the sample,
M: largest |value| or |reward|):  with gamma, lambda in [0, 1] an advantage is  -V_k  plus a combination of later values / the
final reward whose non-negative weights sum to at most 1, so |A| <= 2 M, and an error e_{k+1} of the next advantage enters A_k with
the factor gamma lambda <= 1: the errors of a trajectory's rows ADD, they are not amplified.  A row of (a) makes four float32 roundings
(gamma nv, ... - V, gl na, d + ...; gl itself and the float32 reward are rounded once more per trajectory), each of relative size at
most 2^-24 of a quantity of magnitude <= M (the products) or <= 2 M (the two sums).  The bound charges every one of them as
2^-24 M - four per row, L rows - which is BELOW the worst case of that analysis (2^-24 (1 + 2 + 2 + 2) M per row and more for gl):
it asks (a) to stay within what roundings of typical magnitude and sign add up to, not merely within the worst case.  (b)'s own
float64 error is 2^-29 of that and is ignored.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import rollout_targets_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ST_OK, ST_ILLEGAL = 0, 1


def test_worked_example():
    """N = 2, one game, T = 4: seats 0, 1, 0, 1, the last step ends the episode with rewards (2, -1), gamma = lambda = 0.5."""
    agent = np.array([[0], [1], [0], [1], [0]], dtype=np.uint8)
    done = np.array([[0], [0], [0], [0], [1]], dtype=np.uint8)
    end = np.array([[0], [0], [0], [1]], dtype=np.uint8)
    values = np.array([[0.5], [0.25], [1.0], [0.0], [7.0]], dtype=np.float32)
    rew = np.zeros((4, 1, 2))
    rew[3, 0] = (2.0, -1.0)
    adv, tgt, ret, flags = ref.targets_f32(agent, done, end, values, rew, 0.5, 0.5)
    assert adv[:, 0].tolist() == [0.25, -0.5, 1.0, -1.0]
    assert tgt[:, 0].tolist() == [0.75, -0.25, 2.0, -1.0]
    assert ret[:, 0].tolist() == [2.0, -1.0, 2.0, -1.0]
    assert flags[:, 0].tolist() == [3, 3, 3, 3]
    adv64, tgt64, has, info = ref.targets_f64(agent, done, end, values, rew, 0.5, 0.5)
    assert adv64[:, 0].tolist() == [0.25, -0.5, 1.0, -1.0] and tgt64[:, 0].tolist() == [0.75, -0.25, 2.0, -1.0]
    assert has.all() and info == {"longest": 2, "lost": 0}


def oracle_columns(N, B, T, seed):
    """Columns of T steps of B oracle games (auto-reset on) under random legal actions and a few illegal ones, random values."""
    from tests.oracle_engine import OracleEngine

    rng = np.random.default_rng(seed)
    eng = OracleEngine(B, num_players=N, auto_reset=True)
    eng.seed(None, 100 + seed)
    o = eng.reset_host()
    agent, done = np.zeros((T + 1, B), np.uint8), np.zeros((T + 1, B), np.uint8)
    end = np.zeros((T, B), np.uint8)
    rew = np.zeros((T, B, N))
    for t in range(T):
        agent[t], done[t] = o.agent, o.done
        mask = np.asarray(o.action_mask) > 0
        score = rng.random((B, 26))
        illegal = rng.random(B) < 0.004
        score = np.where(mask ^ illegal[:, None], score, -1.0)   # a legal action, or - rarely - one the mask forbids
        o = eng.step_host(score.argmax(1).astype(np.int32))
        e = (np.asarray(o.done) != 0) & np.isin(np.asarray(o.status), (ST_OK, ST_ILLEGAL))  # the rule of k_episode_ends
        end[t] = e
        rew[t][e] = np.asarray(eng.rewards_host()[0])[e]
    agent[T], done[T] = o.agent, o.done
    values = (rng.standard_normal((T + 1, B)) * 20.0).astype(np.float32)
    return dict(agent=agent, done=done, episode_end=end, values=values, final_rewards=rew)


@pytest.mark.parametrize("N", [1, 2, 3, 4, 8])
@pytest.mark.parametrize("gamma,lam", [(0.99, 0.95), (1.0, 1.0)])
def test_recursion_against_textbook_and_rules(N, gamma, lam):
    B, T = 24, 40 * N + 90
    c = oracle_columns(N, B, T, seed=N)
    valid = c["done"][:T] == 0
    assert c["episode_end"].sum() >= B // 2 and (~valid).sum() > 0    # the sample has episode ends, re-deal rows ...
    assert (c["done"][T] == 0).any()                                   # ... and games to bootstrap
    # the streams are well formed: a row that is no transition follows an episode end (or another such row)
    for t in range(1, T):
        assert (valid[t] | (c["episode_end"][t - 1] != 0) | ~valid[t - 1]).all()
    adv, tgt, ret, flags = ref.targets_f32(gamma=gamma, lam=lam, **c)
    adv64, tgt64, has, info = ref.targets_f64(gamma=gamma, lam=lam, **c)
    has32 = (flags & ref.HAS_TARGET) != 0
    assert np.array_equal(has32, has)
    M = max(float(np.abs(c["values"]).max()), float(np.abs(c["final_rewards"]).max()))
    bound = 4 * info["longest"] * 2.0 ** -24 * M
    err = max(float(np.abs(adv - adv64).max()), float(np.abs(tgt - tgt64).max()))
    print(f"N={N} gamma={gamma} lam={lam}: L={info['longest']} M={M:.3f} bound={bound:.3e} max error={err:.3e}")
    assert err <= bound
    assert not adv[~has32].any() and not tgt[~has32].any()
    # bit 1 and `returns`: the rule of examples.ppo.compute_returns
    returns, mask = ref.returns_rule(c["agent"], c["done"], c["episode_end"], c["final_rewards"])
    known = (flags & ref.EPISODE_KNOWN) != 0
    assert np.array_equal(known, mask) and np.array_equal(ret[mask], returns[mask]) and not ret[~mask].any()
    # the counting identity, its right side from (b)'s episode cut
    assert (has32 <= valid).all()
    assert int(has32.sum()) == int(valid.sum()) - info["lost"]
    assert int(has32.sum()) >= int(valid.sum()) - N * B
    assert info["lost"] > 0 or N == 1   # (a single seat is the bootstrapped one wherever an episode is open at T)


def test_abi_has_rollout_targets():
    """include/skyjo_vec.h declares the entry point and its flags, the library exports it, the ctypes table has it."""
    from skyjo_rl_amd import _lib, build

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "skyjo_vec.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+skyjo_vec_rollout_targets\s*\(", text)
    assert re.search(r"#define\s+SKYJO_TGT_HAS_TARGET\s+1\b", text) and re.search(r"#define\s+SKYJO_TGT_EPISODE_KNOWN\s+2\b", text)
    assert hasattr(ctypes.CDLL(build.build()), "skyjo_vec_rollout_targets")
    res, args = _lib.SIGNATURES["skyjo_vec_rollout_targets"]
    assert res is ctypes.c_int and len(args) == 15 and args[8] is ctypes.c_float and args[9] is ctypes.c_float
    assert (_lib.TGT_HAS_TARGET, _lib.TGT_EPISODE_KNOWN) == (1, 2)
