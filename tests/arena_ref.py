"""numpy restatements of what the arena adds (TEST INFRASTRUCTURE; include/skyjo_vec.h: skyjo_vec_arena_*, skyjo_vec_episode_stats).

``greedy_actions``: SKYJO_SEAT_GREEDY - m = logits + (legal ? 0 : FLOAT_MIN) in float32, the m the masked draw forms
(rlskyjo/models/action_mask_model.py:70-71), and ``np.argmax``, which returns the FIRST maximum.

``episode_sums`` / ``episode_stats``: the statistics of the episode-end columns in float64 - the count, per seat the sum of the final
reward, the sum of its squares (each square one rounded float64 product) and the number of rows in which the seat's reward equals the
row's maximum, over the rows with ``episode_end``.  The sums are ``math.fsum``: the correctly rounded value that any order of
double additions approximates.
"""
import math

import numpy as np

FLOAT_MIN = np.float32(np.finfo(np.float32).min)  # torch.finfo(torch.float32).min == ray's FLOAT_MIN


def masked_logits(logits, mask):
    """float32 [n, 26]: logits where the mask byte is non-zero, logits + FLOAT_MIN (one float32 addition) elsewhere."""
    logits = np.asarray(logits, dtype=np.float32)
    legal = np.asarray(mask) != 0
    return np.where(legal, logits, (logits + FLOAT_MIN).astype(np.float32)).astype(np.float32)


def greedy_actions(logits, mask):
    """int32 [n]: the smallest k that maximises the masked logits."""
    return np.argmax(masked_logits(logits, mask), axis=-1).astype(np.int32)


def episode_sums(final_rewards, episode_end):
    """(count, sums [N], squares [N], wins [N]) over the rows with episode_end != 0; ``final_rewards`` [..., N], ``episode_end`` [...]."""
    fr = np.asarray(final_rewards, dtype=np.float64)
    N = fr.shape[-1]
    fr = fr.reshape(-1, N)
    end = np.asarray(episode_end).reshape(-1) != 0
    x = fr[end]
    count = int(end.sum())
    sums = np.array([math.fsum(x[:, s]) for s in range(N)])
    squares = np.array([math.fsum(x[:, s] * x[:, s]) for s in range(N)])
    wins = (x == x.max(axis=1, keepdims=True)).sum(axis=0).astype(np.int64) if count else np.zeros(N, dtype=np.int64)
    return count, sums, squares, wins


def episode_stats(final_rewards, episode_end):
    """(episodes, mean [N], std [N] - unbiased, 0 for fewer than two episodes -, win_rate [N]) from ``episode_sums``."""
    n, s, q, w = episode_sums(final_rewards, episode_end)
    N = len(s)
    if n == 0:
        return 0, np.zeros(N), np.zeros(N), np.zeros(N)
    mean = s / n
    std = np.sqrt(np.maximum(q - s * s / n, 0.0) / (n - 1)) if n > 1 else np.zeros(N)
    return n, mean, std, w / n
