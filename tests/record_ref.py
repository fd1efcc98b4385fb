"""numpy references for the kernels that read the engine's records on the caller's side - ``k_episode_ends``, ``k_unpack``, ``k_sample``
(csrc/skyjo_callers.h), the pair draw in the net's epilogue and ``k_arena`` (csrc/skyjo_arena.h) - and synthetic records for
them at EVERY record geometry: the indirect observation and the direct one with 1 .. 12 players (record_bytes 64 .. 208, 4 .. 13
16-byte pieces), in both layouts.  numpy only, nothing from the package, deterministic from seeds (TEST INFRASTRUCTURE).  Written from
include/skyjo_vec.h (the record, skyjo_vec_episode_ends, skyjo_vec_unpack, skyjo_vec_*_layout); it shares no code with the library.
tests/test_record_ref.py asserts without a GPU that the cases reach what they claim and that the comparisons reject two restated wrong
kernels; tests/test_gpu_record_consumers.py feeds the same cases to the kernels.  Not collected: a helper.

The record (include/skyjo_vec.h): bytes 0 .. D - 1 the observation (int8), byte D the action the writing step applied (int8, -1: none),
bytes Dp .. Dp + 25 the action mask, Dp + 26 agent, Dp + 27 phase, Dp + 28 done, Dp + 29 status, Dp + 30 / 31 the episode's steps.
Dp + 26 = 58 for the indirect observation and 46 + 12 N for the direct one - 14 mod 16 for N = 4, 8, 12 (STRADDLE): there agent / phase
lie in one 16-byte piece and done / status in the next, which the tile-planar layout puts 1 KiB apart.
"""
import numpy as np

from tests import learner_synth, net_ref

OBS_EDGES, MASK_EDGES = learner_synth.OBS_EDGES, learner_synth.MASK_EDGES

# (N, indirect)
GEOMETRIES = [(3, True), (12, True)] + [(N, False) for N in range(1, 13)]
STRADDLE = [(4, False), (8, False), (12, False)]
DONE_VALUES = (1, 2, 0x80, 0xFF)


def geometry(N, indirect):
    return learner_synth.geometry(N, indirect)


def gid(N, indirect):
    return "%s-N%d" % ("indirect" if indirect else "direct", N)


# ---------------------------------------------------------------- the two layouts
def planar_address(r, k, record_bytes):
    """Byte k of record r in the tile-planar layout (include/skyjo_vec.h, skyjo_vec_*_layout: piece p of game 64 t + l at block
    t * 64 * record_bytes + p * 1024 + l * 16), as an offset into one iteration's block."""
    r, k = np.asarray(r, dtype=np.int64), np.asarray(k, dtype=np.int64)
    return (r // 64) * 64 * record_bytes + (k // 16) * 1024 + (r % 64) * 16 + k % 16


def to_planar(rows, rng):
    """[n, record_bytes] -> [tiles, P, 64, 16] with random non-zero bytes in the padding of a partial last tile."""
    return learner_synth.to_planar_dirty(rows[None], rng)[0]


def rows_from_planar(planar, n):
    """The first n records of tile-planar blocks [tiles, P, 64, 16] as rows [n, record_bytes], through ``planar_address``."""
    rb = planar.shape[-3] * 16
    flat = np.ascontiguousarray(planar).reshape(-1)
    return flat[planar_address(np.arange(n)[:, None], np.arange(rb)[None, :], rb)]


def _fetch(buf, n, k, record_bytes, planar, plus=0):
    """Byte k (+ ``plus`` bytes in MEMORY, which is what a pointer does) of records 0 .. n - 1 of a buffer in either layout."""
    flat = np.ascontiguousarray(buf).reshape(-1)
    r = np.arange(n, dtype=np.int64)
    return flat[(planar_address(r, k, record_bytes) if planar else r * record_bytes + k) + plus]


# ---------------------------------------------------------------- records
def consumer_records(n, g, rng):
    """Row-major records uint8 [n, record_bytes], every byte random; then: the done byte 0 in about half the rows and elsewhere one of
    1, 2, 0x80, 0xFF or a random non-zero byte; byte D (the action) 0xFF = -1 in about a quarter of the rows and 0 .. 25 elsewhere; the
    agent byte < N; and up to ten rows with the observation and the mask at OBS_EDGES / MASK_EDGES."""
    N, D, Dp, rb = (g[k] for k in ("num_players", "obs_dim", "mask_offset", "record_bytes"))
    rec = rng.integers(0, 256, size=(n, rb), dtype=np.uint8)
    pick = rng.integers(0, len(DONE_VALUES) + 1, size=n)
    nonzero = np.where(pick < len(DONE_VALUES), np.array(DONE_VALUES + (0,))[pick], rng.integers(1, 256, size=n))
    rec[:, Dp + 28] = np.where(rng.random(n) < 0.5, 0, nonzero).astype(np.uint8)
    rec[:, D] = np.where(rng.random(n) < 0.25, 0xFF, rng.integers(0, 26, size=n)).astype(np.uint8)
    rec[:, Dp + 26] = rng.integers(0, N, size=n).astype(np.uint8)
    for j, r in enumerate(rng.choice(n, size=min(n, 10), replace=False)):
        rec[r, :D] = np.array(OBS_EDGES, dtype=np.uint8)[(np.arange(D) + j) % 2]
        rec[r, Dp:Dp + 26] = np.array(MASK_EDGES, dtype=np.uint8)[(np.arange(26) + j) % 5]
    return rec


def case_seeds(n, N, indirect):
    """The seeds of one (n, geometry) case.  One record either ends an episode or does not, so n = 1 has three seeds - an end, and a
    running game that was given an action (done = 0: the record whose flag a done byte read from elsewhere turns) among the others -
    and what tests/test_record_ref.py asks of a case it asks of the case's seeds together."""
    base = 52000 + 1000 * n + 20 * N + int(indirect)
    return (base, base + 1, base + 2) if n == 1 else (base,)


def consumer_case(n, N, indirect, seed):
    """geometry, row-major ``rows`` [n, record_bytes] and the same records tile-planar with dirty padding."""
    rng = np.random.default_rng(seed)
    g = geometry(N, indirect)
    rows = consumer_records(n, g, rng)
    return dict(geometry=g, n=n, rows=rows, planar=to_planar(rows, rng))


def synthetic_rewards(n, N, rng):
    """float64 [n, N] with no zero row and fractions float32 cannot hold (the GPU test takes the engine's own rewards instead)."""
    return rng.standard_normal((n, N)) * 4.0 + (rng.random((n, N)) + 1.0) * 2.0 ** -30


EPISODE_B = 130
EPISODE_EDGE_B = (1, 63, 64, 65, 256, 257, 321)      # the tile edge and the edge of the kernel's 256-lane block
EPISODE_EDGE_GEOMETRIES = [(4, False), (3, True)]
EPISODE_CASES = [(EPISODE_B, N, ind) for N, ind in GEOMETRIES] + [(B, N, ind) for N, ind in EPISODE_EDGE_GEOMETRIES for B in EPISODE_EDGE_B]


# ---------------------------------------------------------------- episode ends
def episode_ends_ref(rows, g, rewards):
    """skyjo_vec_episode_ends on row-major records: end = (done != 0) and (int8 byte D != -1); the rewards row where end holds and
    + 0.0 elsewhere.  (final_rewards float64 [n, N], episode_end uint8 [n])"""
    D, Dp = g["obs_dim"], g["mask_offset"]
    end = (rows[:, Dp + 28] != 0) & (rows[:, D].view(np.int8) != -1)
    rewards = np.asarray(rewards, dtype=np.float64)
    return np.where(end[:, None], rewards, 0.0), end.astype(np.uint8)


def episode_ends_neighbour_pointer(buf, n, g, rewards, planar):
    """The WRONG kernel: a pointer to record byte Dp + 26 and the done byte read two bytes past it in memory."""
    D, Dp, rb = g["obs_dim"], g["mask_offset"], g["record_bytes"]
    done = _fetch(buf, n, Dp + 26, rb, planar, plus=2)
    end = (done != 0) & (_fetch(buf, n, D, rb, planar).view(np.int8) != -1)
    return np.where(end[:, None], np.asarray(rewards, dtype=np.float64), 0.0), end.astype(np.uint8)


def same_episode_ends(got, want):
    """The comparison the GPU test makes: final_rewards as int64 bits, episode_end byte for byte."""
    (fr, ee), (wfr, wee) = got, want
    fr, wfr = np.ascontiguousarray(fr, dtype=np.float64), np.ascontiguousarray(wfr, dtype=np.float64)
    return fr.shape == wfr.shape and np.array_equal(fr.view(np.int64), wfr.view(np.int64)) and np.array_equal(np.asarray(ee, dtype=np.uint8), wee)


# ---------------------------------------------------------------- unpack
UNPACK_NAMES = ("obs", "mask", "agent", "phase", "done", "status")


def unpack_ref(rows, g):
    """skyjo_vec_unpack: the six dense arrays - obs int8 [n, D], mask int8 [n, 26], agent / phase / done / status uint8 [n]."""
    D, Dp = g["obs_dim"], g["mask_offset"]
    i8 = rows.view(np.int8)
    return dict(obs=np.ascontiguousarray(i8[:, :D]), mask=np.ascontiguousarray(i8[:, Dp:Dp + 26]), agent=rows[:, Dp + 26].copy(),
                phase=rows[:, Dp + 27].copy(), done=rows[:, Dp + 28].copy(), status=rows[:, Dp + 29].copy())


def unpack_status_from_done(rows, g):
    """The WRONG kernel: ``status`` taken from the done offset."""
    out = unpack_ref(rows, g)
    out["status"] = out["done"].copy()
    return out


def unpack_mismatches(got, want):
    """The names of the arrays of ``got`` (those given) that differ from ``want`` in dtype, shape or any byte."""
    return [k for k in UNPACK_NAMES if k in got and not (got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]))]


UNPACK_ROWS, UNPACK_TILES = 257, 5
UNPACK_EXTRA = dict(rows=(1, 63, 65, 4099), tiles=(1, 3))           # direct N = 4 only
# past the grid cap of 4096 x 256 elements of k_unpack's launch: (N, indirect, tiles)
UNPACK_SECOND_ROUND = [(3, True, 300), (12, False, 88)]
UNPACK_GRID_ELEMENTS = 4096 * 256


# ---------------------------------------------------------------- the draw away from 31 / 32 / 64
def draw_case(n, seed, ticket, g, **kw):
    """``net_ref.draw_case`` laid out for the geometry ``g``."""
    return net_ref.draw_case(n, seed, ticket, record_bytes=g["record_bytes"], mask_offset=g["mask_offset"], obs_dim=g["obs_dim"], **kw)


PAIR_GEOMETRIES = [(N, False) for N in (2, 3, 4)]                   # mask offsets 44 / 56 / 68, 5 / 6 / 7 pieces
DRAW_EDGE_ROWS = (1, 255, 256, 257, 513)                             # direct N = 4: a partial block, an odd number of rows in the last one


# ---------------------------------------------------------------- arena
ARENA_N, ARENA_B = (2, 4, 12), 321


def arena_records(n, g, rng):
    """(records uint8 [n, record_bytes], mask uint8 [n, 26], agent [n]): every byte random, the mask families of ``net_ref.mask_rows``,
    the agent byte uniform in 0 .. N - 1."""
    N, Dp, rb = g["num_players"], g["mask_offset"], g["record_bytes"]
    mask, _ = net_ref.mask_rows(n, rng)
    rec = rng.integers(0, 256, size=(n, rb), dtype=np.uint8)
    rec[:, Dp:Dp + 26] = mask
    agent = rng.integers(0, N, size=n).astype(np.uint8)
    rec[:, Dp + 26] = agent
    return rec, mask, agent
