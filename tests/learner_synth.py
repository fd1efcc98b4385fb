"""Synthetic inputs for the three learner kernels (``k_rollout_targets``, ``k_select_*``, ``k_gather_rows``): record buffers and
columns that a game cannot produce although the definitions (include/skyjo_vec.h) cover them - every byte of a record
random, mask bytes other than 0 / 1, observation bytes at -128 and 127, dirty padding, episode ends on re-deal rows and on the first
and the last row, rewards where no episode ended, values spread over six orders of magnitude.  numpy only, nothing from the package,
deterministic from a seed (TEST INFRASTRUCTURE).  tests/test_learner_synth.py asserts without a GPU that what is generated here
reaches what it is meant to reach; tests/test_gpu_learner_synthetic.py feeds it to the kernels.
"""
import numpy as np

OBS_EDGES = (0x80, 0x7F)
MASK_EDGES = (0, 1, 2, 0x80, 0xFF)
SCALES = (1e-3, 1.0, 1e3)
PARAMS = [(1.0, 1.0), (0.99, 1.0), (0.99, 0.95), (0.5, 0.5), (0.0, 0.0)]   # the (gamma, lambda) pairs of test_gpu_rollout_targets.py


def geometry(N, indirect=True):
    """The record geometry of include/skyjo_vec.h as plain integers (the GPU test checks the engine's own numbers against it)."""
    D = 31 if indirect else 19 + 12 * N
    Dp = (D + 3) & ~3
    rb = (Dp + 32 + 15) & ~15
    return dict(num_players=N, obs_dim=D, mask_offset=Dp, record_bytes=rb)


def records(S, B, env_geometry, rng):
    """Row-major records uint8 [S, B, record_bytes], every byte random; then the done byte 0 with probability 0.85, the agent byte
    < N where done == 0 and anywhere in 0 .. 255 elsewhere, and up to ten rows forced to the edge values of OBS_EDGES / MASK_EDGES."""
    N, D, Dp, rb = (env_geometry[k] for k in ("num_players", "obs_dim", "mask_offset", "record_bytes"))
    rec = rng.integers(0, 256, size=(S, B, rb), dtype=np.uint8)
    done = np.where(rng.random((S, B)) < 0.85, 0, rng.integers(1, 256, size=(S, B))).astype(np.uint8)
    rec[..., Dp + 28] = done
    rec[..., Dp + 26] = np.where(done == 0, rng.integers(0, N, size=(S, B)), rng.integers(0, 256, size=(S, B))).astype(np.uint8)
    flat = rec.reshape(S * B, rb)
    for j, r in enumerate(rng.choice(S * B, size=min(S * B, 10), replace=False)):
        flat[r, :D] = np.array(OBS_EDGES, dtype=np.uint8)[(np.arange(D) + j) % 2]
        flat[r, Dp:Dp + 26] = np.array(MASK_EDGES, dtype=np.uint8)[(np.arange(26) + j) % 5]
    return rec


def meta(rec, env_geometry):
    """(agent, done) uint8 [S, B]: the two meta bytes the targets read."""
    Dp = env_geometry["mask_offset"]
    return np.ascontiguousarray(rec[..., Dp + 26]), np.ascontiguousarray(rec[..., Dp + 28])


def to_planar_dirty(rows, rng):
    """``rollout_batches_ref.to_planar`` - [S, B, rec_bytes] re-laid as [S, tiles, P, 64, 16] - with random NON-ZERO bytes in the
    padding slots of a partial last tile: a kernel that reads a padding slot does not pass by luck."""
    S, B, rb = rows.shape
    assert rb % 16 == 0
    tiles, P = (B + 63) // 64, rb // 16
    out = rng.integers(1, 256, size=(S, tiles, P, 64, 16), dtype=np.uint8)
    for b in range(B):
        out[:, b // 64, :, b % 64, :] = rows[:, b].reshape(S, P, 16)
    return out


def target_columns(T, B, N, rng, scale=None, done=None, force_last=True):
    """``episode_end`` uint8 [T, B] (density 0.15, set at (0, b0) and - unless ``force_last`` is off - (T - 1, b1); with ``done``
    [T + 1, B] also on about a third of the rows that are no transition), ``final_rewards`` float64 [T, B, N] random on EVERY row with fractions float32 cannot hold,
    ``values`` float32 [T + 1, B] = normal * scale, scale per game from SCALES (or the given one).  Returns the three and (b0, b1)."""
    end = (rng.random((T, B)) < 0.15).astype(np.uint8)
    b0, b1 = int(rng.integers(0, B)), int(rng.integers(0, B))
    end[0, b0] = 1
    if force_last:
        end[T - 1, b1] = 1
    if done is not None:
        end[(done[:T] != 0) & (rng.random((T, B)) < 0.35)] = 1
    sc = np.asarray(SCALES)[rng.integers(0, 3, size=B)] if scale is None else np.full(B, float(scale))
    rewards = rng.standard_normal((T, B, N)) * 4.0 * sc[None, :, None] + rng.random((T, B, N)) * 2.0 ** -30
    values = (rng.standard_normal((T + 1, B)) * sc[None, :]).astype(np.float32)
    return dict(episode_end=end, final_rewards=rewards, values=values), (b0, b1)


# Seeds per (T, B, N) of the targets cases: 1000 T + 10 B + N unless listed.  A single game is either bootstrapped or not, so B = 1 has
# two seeds, and what tests/test_learner_synth.py asks of a case it asks of the case's seeds together.  An episode end on the last
# row of a single game leaves no row to bootstrap, so with B = 1 only the first seed forces that end.
TARGET_SEEDS = {(17, 1, 4): (1, 5)}


def target_seeds(T, B, N):
    return TARGET_SEEDS.get((T, B, N), (1000 * T + 10 * B + N,))


def targets_case(T, B, N, seed, indirect=True):
    """Everything one targets case feeds the kernel: ``geometry``, row-major ``records`` [T + 1, B, rec_bytes], ``planar`` (dirty), and
    ``cols`` = the five inputs of ``rollout_targets_ref.targets_*``.  The two forced episode ends sit on transitions."""
    rng = np.random.default_rng(seed)
    g = geometry(N, indirect)
    rec = records(T + 1, B, g, rng)
    agent, done = meta(rec, g)
    force_last = B > 1 or seed == target_seeds(T, B, N)[0]
    cols, (b0, b1) = target_columns(T, B, N, rng, done=done, force_last=force_last)
    for t, b in ((0, b0), (T - 1, b1))[:2 if force_last else 1]:
        rec[t, b, g["mask_offset"] + 28] = 0
        rec[t, b, g["mask_offset"] + 26] = rng.integers(0, N)
    agent, done = meta(rec, g)
    return dict(geometry=g, records=rec, planar=to_planar_dirty(rec, rng), cols=dict(agent=agent, done=done, **cols))


TARGET_CASES = sorted(set([(T, 65, 3) for T in (1, 2, 15, 16, 17, 33, 48)] + [(17, B, 4) for B in (1, 63, 64, 65, 200)] +
                          [(33, 65, N) for N in range(1, 13)]))


# ---- select ----
SEL_ROWS = 4096                                               # rows per block of k_select_pass
SELECT_SIZES = [(nb - 1) * SEL_ROWS + 1 for nb in (1024, 1025, 2049)] + [1024 * SEL_ROWS]
WORKLOAD_ROWS = 65536 * 320                                   # 5 120 blocks: five per thread of the scan
SELECT_PATTERNS = ("random", "all", "none", "first", "last", "islands")
ISLAND_BLOCKS = (0, 1023, 1024)                               # and the last block


def island_blocks(n):
    nb = (n + SEL_ROWS - 1) // SEL_ROWS
    return sorted(set(b for b in ISLAND_BLOCKS + (nb - 1,) if b < nb))


def select_flags(n, pattern, rng):
    """A flags column uint8 [n].  Bits 2 .. 7 are random everywhere (the definition looks at ``require`` only); bits 0 / 1:
    random / both set / both clear / both clear but row 0 / but row n - 1 / both clear outside ISLAND_BLOCKS and the last block."""
    f = rng.integers(0, 256, size=n, dtype=np.uint8)
    if pattern == "random":
        return f
    if pattern == "all":
        return f | 3
    low = f & 3
    f &= 0xFC
    if pattern == "first":
        f[0] |= 3
    elif pattern == "last":
        f[n - 1] |= 3
    elif pattern == "islands":
        for b in island_blocks(n):
            f[b * SEL_ROWS:(b + 1) * SEL_ROWS] |= low[b * SEL_ROWS:(b + 1) * SEL_ROWS]
            f[b * SEL_ROWS] |= 3                              # (the last block may hold this one row only)
    else:
        assert pattern == "none", pattern
    return f


def select_advantages(n, rng):
    return (rng.standard_normal(n, dtype=np.float32) * np.float32(25.0)).astype(np.float32)


# ---- gather ----
GATHER_B, GATHER_T = 200, 3
GATHER_M = (1, 63, 64, 65, 128, 129, 600)
# (N, indirect): the issue's player counts in both observation modes, and the direct records of 6, 8, 10 and 11 players - without
# them the piece counts 8, 10, 11 and 12 (record_bytes / 16) are never gathered
GATHER_GEOMETRIES = [(N, ind) for N in (1, 2, 3, 4, 7, 12) for ind in (True, False)] + [(N, False) for N in (6, 8, 10, 11)]
GATHER_NORMS = ((0.0, 1.0), (0.1, 0.7))                       # (0, 1), and a pair float32 holds only rounded


def gather_case(N, indirect, seed=None):
    """Records of GATHER_T + 1 steps x GATHER_B games (row-major and dirty tile-planar), the five columns, and the index lists."""
    rng = np.random.default_rng(7000 + 10 * N + indirect if seed is None else seed)
    g = geometry(N, indirect)
    B, T = GATHER_B, GATHER_T
    n = T * B
    rec = records(T + 1, B, g, rng)
    sc = np.asarray(SCALES)[rng.integers(0, 3, size=(T + 1) * B)]
    cols = dict(actions=rng.integers(-2 ** 31, 2 ** 31, size=n).astype(np.int32), logp=-rng.random(n, dtype=np.float32),
                values=(rng.standard_normal((T + 1) * B) * sc).astype(np.float32),
                advantages=(rng.standard_normal(n) * 9 * sc[:n]).astype(np.float32), value_targets=rng.standard_normal(n, dtype=np.float32))
    perm = rng.permutation(n).astype(np.int64)
    lists = {f"perm-{m}": perm[:m].copy() for m in GATHER_M}
    first = (B // 64) * 64                                    # every row of the partial last tile, in every step
    lists["partial-tile"] = np.concatenate([t * B + np.arange(first, B) for t in range(T)]).astype(np.int64)
    bad = np.array([-1, n, 2 ** 63 - 1, -2 ** 63, n + 1, -n, 2 ** 32, -2 ** 32 + 5, 2 ** 31, (T + 1) * B - 1], dtype=np.int64)
    lists["out-of-range"] = np.resize(bad, 65)
    mixed = perm[:129].copy()
    mixed[::2] = np.resize(bad, 65)
    lists["interleaved"] = mixed
    lists["copies"] = np.full(64, perm[5], dtype=np.int64)
    return dict(geometry=g, records=rec, planar=to_planar_dirty(rec, rng), cols=cols, lists=lists)
