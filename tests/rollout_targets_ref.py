"""Two restatements of ``skyjo_vec_rollout_targets`` (include/skyjo_vec.h) for the tests - neither shares code with the
package (TEST INFRASTRUCTURE):

(a) ``targets_f32``: the recursion of the definition in numpy float32, operation for operation, vectorised over the games.  numpy
    rounds every ufunc call on its own, so this is bit-for-bit what the kernel must give.
(b) ``targets_f64``: a textbook GAE in float64.  Every game is cut into episodes, every seat's trajectory is taken out of its
    episode and the ordinary recursion  A_k = delta_k + gamma lambda A_{k+1},  delta_k = r_k + gamma V_{k+1} - V_k  is run on it.
    A trajectory whose episode did not end inside the buffer is truncated at the seat's last action there: that action is the
    bootstrap of the ones before it and has no target itself - unless the seat is the one ``records[T]`` expects, whose bootstrap
    is ``values[T]``.

Inputs (numpy): agent, done uint8 [T+1, B] (the meta bytes of the records), episode_end uint8 [T, B], values float32 [T+1, B],
final_rewards float64 [T, B, N].  gamma / lambda are taken as the float32 numbers the C ABI receives.
"""
import numpy as np

HAS_TARGET, EPISODE_KNOWN = 1, 2


def targets_f32(agent, done, episode_end, values, final_rewards, gamma, lam):
    """(advantages, value_targets, returns) float32 [T, B], flags uint8 [T, B]."""
    f = np.float32
    T, B = episode_end.shape
    N = final_rewards.shape[2]
    values = np.asarray(values, dtype=f)
    g = f(gamma)
    gl = f(f(gamma) * f(lam))
    UNKNOWN, TERMINAL, NEXT = 0, 1, 2
    state = np.full((B, N), UNKNOWN, dtype=np.int8)
    R, nv, na = (np.zeros((B, N), dtype=f) for _ in range(3))
    known = np.zeros(B, dtype=bool)
    rows = np.arange(B)
    boot = done[T] == 0
    s = agent[T].astype(np.int64)
    state[rows[boot], s[boot]] = NEXT
    nv[rows[boot], s[boot]] = values[T][boot]
    adv, tgt, ret = (np.zeros((T, B), dtype=f) for _ in range(3))
    flags = np.zeros((T, B), dtype=np.uint8)
    for t in range(T - 1, -1, -1):
        e = episode_end[t] != 0                                  # 1.
        state[e] = TERMINAL
        R[e] = final_rewards[t][e].astype(f)
        known = known | e
        inv = done[t] != 0                                       # 2.
        s = np.where(inv, 0, agent[t]).astype(np.int64)
        V = values[t]
        st, Rs = state[rows, s], R[rows, s]
        a_term = Rs - V                                          # 3. TERMINAL
        d = g * nv[rows, s] - V                                  #    NEXT: two roundings ...
        a_next = d + gl * na[rows, s]                            #    ... and two more
        A = np.where(st == TERMINAL, a_term, np.where(st == NEXT, a_next, f(0))).astype(f)
        has = (st != UNKNOWN) & ~inv
        A = np.where(inv, f(0), A).astype(f)
        adv[t] = A
        tgt[t] = np.where(has, A + V, f(0))                      # 4.
        ret[t] = np.where(known & ~inv, Rs, f(0))                # 5.
        flags[t] = has * HAS_TARGET + (known & ~inv) * EPISODE_KNOWN
        state[inv] = UNKNOWN
        ok = ~inv                                                # 6.
        state[rows[ok], s[ok]] = NEXT
        nv[rows[ok], s[ok]] = V[ok]
        na[rows[ok], s[ok]] = A[ok]
    return adv, tgt, ret, flags


def cut_episodes(done, episode_end, b):
    """Episodes of game b as (rows, end): ``rows`` a maximal run of transitions (done == 0), closed by the row whose step ended the
    episode (end = that t), by a row that is no transition (end = None), or by the end of the buffer (end = 'T')."""
    T = episode_end.shape[0]
    episodes, cur = [], []
    for t in range(T):
        if done[t, b]:
            if cur:
                episodes.append((cur, None))
            cur = []
            continue
        cur.append(t)
        if episode_end[t, b]:
            episodes.append((cur, t))
            cur = []
    if cur:
        episodes.append((cur, "T"))
    return episodes


def targets_f64(agent, done, episode_end, values, final_rewards, gamma, lam):
    """Textbook GAE per (episode, seat) trajectory in float64: advantages, value_targets float64 [T, B], has bool [T, B], and
    ``info`` = {"longest": longest seat trajectory, "lost": the (game, seat) pairs of the counting identity}."""
    T, B = episode_end.shape
    N = final_rewards.shape[2]
    g, l = float(np.float32(gamma)), float(np.float32(lam))
    V = np.asarray(values, dtype=np.float64)
    adv, tgt = np.zeros((T, B)), np.zeros((T, B))
    has = np.zeros((T, B), dtype=bool)
    longest, lost = 0, 0
    for b in range(B):
        for rows, end in cut_episodes(done, episode_end, b):
            for seat in range(N):
                tr = [t for t in rows if agent[t, b] == seat]
                if not tr:
                    continue
                longest = max(longest, len(tr))
                if end is not None and end != "T":          # finished: reward on the seat's last action, nothing after it
                    next_v, next_a, first = 0.0, 0.0, len(tr) - 1
                    last_r = float(final_rewards[end, b, seat])
                elif end == "T" and done[T, b] == 0 and agent[T, b] == seat:  # the seat records[T] expects: values[T] bootstraps
                    next_v, next_a, first, last_r = V[T, b], 0.0, len(tr) - 1, 0.0
                else:                                        # truncated at the seat's last action: it is the bootstrap
                    next_v, next_a, first, last_r = V[tr[-1], b], 0.0, len(tr) - 2, 0.0
                    # the counting identity's pairs: an episode still open at T, not the bootstrapped seat, no invalid row
                    # after the seat's last action
                    if end == "T" and not done[tr[-1] + 1:T, b].any():
                        lost += 1
                for k in range(first, -1, -1):
                    t = tr[k]
                    r = last_r if k == len(tr) - 1 else 0.0
                    delta = r + g * next_v - V[t, b]
                    a = delta + g * l * next_a
                    adv[t, b], tgt[t, b], has[t, b] = a, a + V[t, b], True
                    next_v, next_a = V[t, b], a
    return adv, tgt, has, {"longest": longest, "lost": lost}


def returns_rule(agent, done, episode_end, final_rewards):
    """``examples.ppo.compute_returns`` restated in numpy: returns float32 [T, B] (the carried final reward of the acting seat,
    whatever the mask) and mask bool [T, B] (a transition whose episode ended inside the buffer)."""
    T, B = episode_end.shape
    N = final_rewards.shape[2]
    carry = np.zeros((B, N))
    known = np.zeros(B, dtype=bool)
    returns = np.zeros((T, B), dtype=np.float32)
    mask = np.zeros((T, B), dtype=bool)
    for t in range(T - 1, -1, -1):
        e = episode_end[t] != 0
        carry = np.where(e[:, None], final_rewards[t], carry)
        known = known | e
        returns[t] = np.take_along_axis(carry, agent[t].astype(np.int64)[:, None], 1)[:, 0].astype(np.float32)
        mask[t] = known & (done[t] == 0)
    return returns, mask


def columns_from_buffer(buf):
    """The numpy inputs of the functions above from a filled ``skyjo_rl_amd.rollout.RolloutBuffer``."""
    v = buf.views()
    return dict(agent=v.agent.cpu().numpy(), done=v.done.cpu().numpy(), episode_end=buf.episode_end.cpu().numpy(),
                values=buf.values[..., 0].cpu().numpy(), final_rewards=buf.final_rewards.cpu().numpy())
