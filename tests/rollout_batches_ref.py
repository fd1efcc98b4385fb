"""``skyjo_vec_rollout_select`` / ``skyjo_vec_rollout_gather`` (include/skyjo_vec.h) restated in numpy for the tests - shares
no code with the package (TEST INFRASTRUCTURE).

Records are a flat uint8 array; ``byte(r, k, rec_bytes, planar)`` is the position of byte k of record r in it and restates the
header's formula for either layout - the gather below goes through it, never through ``rows_from_planar``:

    row-major     r * rec_bytes + k
    tile-planar   (r // 64) * 64 * rec_bytes + (k // 16) * 1024 + (r % 64) * 16 + k % 16

A buffer of S steps holds ``stride`` records per step (B row-major; tiles * 64 tile-planar), so row id ``t * B + b`` of the learner
is record ``t * stride + b``.
"""
import numpy as np

FLOAT_MIN = -np.finfo(np.float32).max   # action_mask_model.FLOAT_MIN: what clamp(log(0), min=FLOAT_MIN) yields


def byte(r, k, rec_bytes, planar):
    r, k = np.asarray(r, dtype=np.int64), np.asarray(k, dtype=np.int64)
    if planar:
        return (r // 64) * (64 * rec_bytes) + (k // 16) * 1024 + (r % 64) * 16 + k % 16
    return r * rec_bytes + k


def to_planar(rows):
    """Row-major records [S, B, rec_bytes] re-laid as tile-planar [S, tiles, P, 64, 16], zero in the padding slots of a partial
    last tile."""
    S, B, rb = rows.shape
    assert rb % 16 == 0
    tiles, P = (B + 63) // 64, rb // 16
    out = np.zeros((S, tiles, P, 64, 16), dtype=np.uint8)
    for b in range(B):
        out[:, b // 64, :, b % 64, :] = rows[:, b].reshape(S, P, 16)
    return out


def select(flags, require):
    """Ascending ids of the rows whose flags have every bit of ``require`` (int64)."""
    f = np.asarray(flags).reshape(-1)
    return np.flatnonzero((f & require) == require).astype(np.int64)


def moments(advantages, index):
    """(sum a, sum a * a) in float64 over the selected rows; (0.0, 0.0) for none."""
    a = np.asarray(advantages).reshape(-1)[index].astype(np.float64)
    return float(a.sum()), float((a * a).sum())


def mean_std(s, q, n):
    """Mean and unbiased standard deviation from the two sums, as ``rollout.select_rows`` forms them."""
    mean = s / n if n else 0.0
    std = float(np.sqrt(max(q - s * s / n, 0.0) / (n - 1))) if n > 1 else 0.0
    return mean, std


def normalise(adv, mean, std):
    """``(a - mean) / std``: two float32 operations, each rounded."""
    f = np.float32
    return ((np.asarray(adv, dtype=f) - f(mean)).astype(f) / f(std)).astype(f)


def gather(records, planar, rec_bytes, D, B, T, stride, index, actions, logp, values, advantages, value_targets, mean=0.0, std=1.0):
    """The eight outputs of the gather for the row ids ``index``: a dict of numpy arrays named like ``rollout.Minibatch``.
    ``records``: any uint8 array holding the buffer's records in the given layout; ``values``: [T (+ 1), B] (component 0; row id r is its flat position too)."""
    flat = np.ascontiguousarray(records).reshape(-1)
    Dp = (D + 3) & ~3
    idx = np.asarray(index, dtype=np.int64)
    m = idx.size
    ok = (idx >= 0) & (idx < T * B)
    r = np.where(ok, idx, 0)
    rec = (r // B) * stride + r % B
    col = lambda k: flat[byte(rec[:, None], np.asarray(k)[None, :], rec_bytes, planar)]
    obs = col(np.arange(D)).view(np.int8).astype(np.float32)
    mask = col(Dp + np.arange(26))
    lm = np.where(mask != 0, np.float32(0), np.float32(FLOAT_MIN)).astype(np.float32)
    seats = col(np.array([Dp + 26]))[:, 0]
    take = lambda c: np.asarray(c).reshape(-1)[r]
    out = dict(observations=obs, log_mask=lm, actions=take(actions).astype(np.int64), logp=take(logp).astype(np.float32),
               advantages=normalise(take(advantages), mean, std), value_targets=take(value_targets).astype(np.float32),
               values=take(values).astype(np.float32), seats=seats.astype(np.uint8))
    for k, v in out.items():   # a row id outside [0, T * B) gives an all-zero row
        v[~ok] = 0
    assert all(v.shape[0] == m for v in out.values())
    return out
