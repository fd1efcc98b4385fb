"""Row counts past 2^31 and 2^32: the plans, windows and checks of tests/test_gpu_big_rows.py (numpy and torch expressions only, nothing
from the package; tests/test_big_rows.py holds them without a GPU).  Not collected: a helper.

include/skyjo_vec.h takes row counts as int64_t.  A 32-bit product in a kernel's addressing or in a grid computation shows only where
a byte offset, an element index or a row id passes 2^31 or 2^32, so every case here is the smallest row count that carries one of its
arrays across such a mark, plus POOL rows - never a multiple of 64 or 256.

Content is periodic with the prime period POOL = 4099 (tests/net_ref.py): row r of every input is pool row r % POOL.  A row read from
an offset that wrapped lands on another pool row, because no mark divided by a stride is a multiple of POOL (``wrap_is_visible``).
A kernel whose output row depends on the input row's content alone is then checked in two steps: its first POOL output rows against
the CPU reference, and the WHOLE output on the device against its own first period tiled (``periodic_mismatches``) - full coverage
that does not depend on the kernel's indexing.  What depends on the row id is checked in ``windows``: 512 rows (two 256-row blocks,
eight tiles) at the first rows, the last rows and around every mark of every array of the call.
"""
from collections import namedtuple

import numpy as np

from tests import learner_synth, net_ref

POOL = net_ref.POOL
WIDTH = 512
GIB = 1 << 30
CAP = 16 * GIB                # max_memory_allocated of one test: twice what the suite's largest case held before
CHUNK_BYTES = 64 << 20        # no temporary of a fill or a check is larger
GUARD, FILL = 256, 0xA5       # as tests/test_gpu_record_consumers.py

# (label, position, unit): the byte or element of an array whose row a window must cover
MARKS = (("byte 2^31", 2 ** 31, "byte"), ("byte 2^32", 2 ** 32, "byte"), ("element 2^31", 2 ** 31, "element"))

Arr = namedtuple("Arr", ["name", "stride", "elem", "out"])   # bytes per row, bytes per element, written by the call


def rows_to_reach(stride, position):
    """The smallest n with n * stride >= position, plus POOL."""
    return -(-position // stride) + POOL


def mark_rows(n, arrays, marks=MARKS):
    """[(array, label, row)]: the row of each array that holds the byte / the element of each mark, where n rows reach it."""
    out = []
    for a in arrays:
        for label, pos, unit in marks:
            byte = pos if unit == "byte" else pos * a.elem
            if byte < n * a.stride:
                out.append((a.name, label, byte // a.stride))
    return out


def windows(n, arrays, marks=MARKS, width=WIDTH):
    """Sorted, distinct row ranges (lo, hi), ``width`` rows each (fewer only when n is smaller): the first rows, the last rows, and per
    mark of ``mark_rows`` a range with the mark's row in its middle, moved inside [0, n)."""
    w = min(width, n)
    los = {0, n - w}
    for _, _, row in mark_rows(n, arrays, marks):
        los.add(min(max(row - w // 2, 0), n - w))
    return [(lo, lo + w) for lo in sorted(los)]


def window_rows(wins):
    """The rows of the windows, ascending, each once: int64."""
    return np.unique(np.concatenate([np.arange(lo, hi, dtype=np.int64) for lo, hi in wins]))


def wrap_is_visible(arrays, marks=MARKS):
    """No mark of any array, in rows, is a multiple of POOL: a row read `mark` bytes too low holds another pool row."""
    for a in arrays:
        for _, pos, unit in marks:
            byte = pos if unit == "byte" else pos * a.elem
            if byte % a.stride == 0 and (byte // a.stride) % POOL == 0:
                return False
    return True


def repeat_counts(n):
    """How often each pool row occurs among rows 0 .. n - 1: int64 [POOL]."""
    c = np.full(POOL, n // POOL, dtype=np.int64)
    c[:n % POOL] += 1
    return c


# ---------------------------------------------------------------- fills and checks (torch; the same code runs on the CPU toy)
def fill_periodic(buf, pool):
    """buf[r] = pool[r % len(pool)] for every row of ``buf`` ([n, ...] contiguous), by copies of a chunk of whole periods that is no
    larger than CHUNK_BYTES."""
    import torch

    n, period = buf.shape[0], pool.shape[0]
    row_bytes = max(1, pool[0].numel() * pool.element_size())
    reps = max(1, min(CHUNK_BYTES // (period * row_bytes), -(-n // period)))
    chunk = torch.cat([pool] * reps) if reps > 1 else pool
    for start in range(0, n, reps * period):
        k = min(reps * period, n - start)
        buf[start:start + k].copy_(chunk[:k])
    return buf


def _bits(t):
    import torch

    t = t.reshape(t.shape[0], -1)
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def periodic_mismatches(out, period=POOL, first=None):
    """The number of rows r >= period of ``out`` ([n, ...]) whose bits differ from row r % period of ``first`` (default: out's own first
    period), with torch expressions in chunks of at most CHUNK_BYTES.  (count, first bad row or -1)"""
    x = _bits(out)
    n, width = x.shape
    head = x[:period] if first is None else _bits(first)
    reps = max(1, CHUNK_BYTES // (period * width * x.element_size()))
    bad, where = 0, -1
    for start in range(period if first is None else 0, n, reps * period):
        k = min(reps * period, n - start)
        whole = k // period
        diff = []
        if whole:
            diff.append((x[start:start + whole * period].view(whole, period, width) != head[None]).any(-1).reshape(-1))
        if k > whole * period:
            diff.append((x[start + whole * period:start + k] != head[:k - whole * period]).any(-1))
        for j, d in enumerate(diff):
            c = int(d.sum())
            if c and where < 0:
                where = start + j * whole * period + int(d.nonzero()[0, 0])
            bad += c
    return bad, where


def window_mismatches(out, wins, reference, sentinel=None):
    """The rows of the windows whose bits differ from ``reference(rows)`` (rows int64 numpy -> array of out's row shape and dtype),
    and how many elements of ``out`` still hold ``sentinel`` (a scalar of out's bit type; None: not looked at).  (bad rows, sentinels)"""
    import torch

    x = _bits(out)
    bad = []
    for lo, hi in wins:
        rows = np.arange(lo, hi, dtype=np.int64)
        want = _bits(torch.as_tensor(np.ascontiguousarray(reference(rows))).to(out.device))
        d = (x[lo:hi] != want).any(-1)
        bad += [lo + int(i) for i in d.nonzero().reshape(-1)]
    left = 0
    if sentinel is not None:
        step = max(1, CHUNK_BYTES // (x.shape[1] * x.element_size()))
        for start in range(0, x.shape[0], step):
            left += int((x[start:start + step] == sentinel).sum())
    return bad, left


# ---------------------------------------------------------------- the toy: one restated row kernel with its addressing slips
TOY_ROWS, TOY_STRIDE, TOY_BLOCK = 3 * POOL, 8, 256
TOY_WRAP = 5000 * TOY_STRIDE  # the toy's "2^32 bytes": 5000 rows, no multiple of POOL
TOY_MARKS = (("byte wrap / 2", TOY_WRAP // 2, "byte"), ("byte wrap", TOY_WRAP, "byte"))
TOY_SENTINEL = -(2 ** 62)
SLIPS = ("wrapped-offset", "signed-product", "dropped-last-block", "shifted-output")


def toy_pool():
    return np.random.default_rng(4).integers(0, 2 ** 40, size=(POOL, 1), dtype=np.int64)


def toy_reference(rows):
    """out[r] = 3 * in[r] + 1 with in[r] = pool[r % POOL]: int64 [len(rows), 1]."""
    return 3 * toy_pool()[np.asarray(rows) % POOL] + 1


def toy_kernel(n, slip=None, wrap=TOY_WRAP):
    """The toy on rows 0 .. n - 1 into a sentinel-filled output, right or with one slip:
      wrapped-offset      the input's byte offset r * stride taken modulo ``wrap``
      signed-product      r * stride as a signed integer of log2(wrap) bits: from wrap / 2 on it is negative and the lane leaves
      dropped-last-block  n / 256 blocks launched, rounded down
      shifted-output      row r written to out[r + 1]"""
    assert slip is None or slip in SLIPS
    r = np.arange(n, dtype=np.int64)
    src = r.copy()
    live = np.ones(n, dtype=bool)
    dst = r.copy()
    if slip == "wrapped-offset":
        src = (r * TOY_STRIDE % wrap) // TOY_STRIDE
    elif slip == "signed-product":
        live &= (r * TOY_STRIDE) % wrap < wrap // 2
    elif slip == "dropped-last-block":
        live &= r < n // TOY_BLOCK * TOY_BLOCK
    elif slip == "shifted-output":
        dst = r + 1
        live &= dst < n
    out = np.full((n, 1), TOY_SENTINEL, dtype=np.int64)
    out[dst[live]] = toy_reference(src[live])
    return out


# ---------------------------------------------------------------- the GPU cases
def _geometry(N, indirect):
    g = learner_synth.geometry(N, indirect)
    return g["obs_dim"], g["mask_offset"], g["record_bytes"]


def _plan():
    """name -> dict(n, arrays, extra): ``n`` rows, the arrays of the call with their strides, and the bytes the test holds besides them
    (guards, pools, the fills' and checks' chunks, scratch).  Tile-planar records count by their row stride too: byte b of the buffer
    lies in tile b // (64 record_bytes), the tile of row b // record_bytes."""
    cases = {}
    slack = 6 * CHUNK_BYTES

    def add(name, n, arrays, extra=0):
        cases[name] = dict(n=n, arrays=arrays, extra=extra + slack)

    # 1. unpack: direct observation, 12 players
    D, Dp, rb = _geometry(12, False)
    unpack = [Arr("records", rb, 1, False), Arr("obs", D, 1, True), Arr("mask", 26, 1, True)] + [Arr(k, 1, 1, True) for k in ("agent", "phase", "done", "status")]
    n = rows_to_reach(D, 2 ** 32)
    add("unpack-rows", n, unpack)
    add("unpack-tiles", (n + 63) // 64 * 64, unpack)          # whole tiles: the call counts tiles
    # 2. the net's forward: indirect records, 26 outputs
    D, Dp, rb = _geometry(3, True)
    n = 2 ** 26 + POOL
    forward = [Arr("records", rb, 1, False), Arr("out", 26 * 4, 4, True)]
    add("forward-rows-fp32", n, forward)
    add("forward-planar-bf16", n, forward)
    # 3. the one-lane draw
    draw = [Arr("records", rb, 1, False), Arr("logits", 26 * 4, 4, False)] + [Arr(k, 4, 4, True) for k in ("actions", "logp", "uniform")]
    add("sample-rows", rows_to_reach(26, 2 ** 31), draw)
    add("sample-planar", 2 ** 26 + POOL, draw)
    # 6. select: one flag byte per row, the index as long as the islands
    n = 2 ** 31 + POOL
    add("select", n, [Arr("flags", 1, 1, False), Arr("advantages", 4, 4, False)], extra=64 * WIDTH * 8)
    # 8. gather_logits: (a) a short index into a long column, (b) a long periodic index
    n = rows_to_reach(26 * 4, 2 ** 32)
    add("gather-logits-column", n, [Arr("column", 26 * 4, 4, False)], extra=1 << 20)
    add("gather-logits-index", n, [Arr("column", 26 * 4, 4, False), Arr("index", 8, 8, False), Arr("out", 26 * 4, 4, True)])
    # 9. the loss head
    head = [Arr(k, 26 * 4, 4, False) for k in ("logits", "log_mask")] + [Arr("actions", 8, 8, False)] + \
           [Arr(k, 4, 4, False) for k in ("value", "logp_old", "advantages", "value_targets", "values_old")] + \
           [Arr("grad_logits", 26 * 4, 4, True), Arr("grad_value", 4, 4, True)]
    add("ppo-loss", n, head, extra=(n + 127) // 128 * 64)
    n = rows_to_reach(26 * 4, 2 ** 31)
    add("ppo-loss-kl", n, head[:2] + [Arr("old_logits", 26 * 4, 4, False)] + head[2:], extra=(n + 127) // 128 * 64)
    # 10. episode statistics, four players
    n = rows_to_reach(4 * 8, 2 ** 32)
    add("episode-stats", n, [Arr("final_rewards", 4 * 8, 8, False), Arr("episode_end", 1, 1, False)], extra=(n + 1023) // 1024 * 13 * 8)
    # 4. both branches with the draw: indirect records, logits and values out
    n = 2 ** 26 + POOL
    act = [Arr("records", rb, 1, False), Arr("logits", 26 * 4, 4, True)] + [Arr(k, 4, 4, True) for k in ("actions", "logp", "values")]
    add("act-value-rows-fp32", n, act)
    add("act-value-planar-bf16", n, act)
    # 6 / 7 (a). a buffer of WINDOW_T steps of WINDOW_B games: select_seats over its rows, and a short gather out of them
    n = WINDOW_T * WINDOW_B
    columns = [Arr(k, 4, 4, False) for k in ("actions", "logp", "values", "advantages", "value_targets")]
    add("gather-window", n, [Arr("records", rb, 1, False)] + columns, extra=2 * (WINDOW_B + 64) * rb)
    add("select-seats", n, [Arr("records", rb, 1, False), Arr("flags", 1, 1, False), Arr("advantages", 4, 4, False)], extra=2 * (WINDOW_B + 64) * rb)
    # 7 (b). a long gather out of a buffer of one step of POOL games
    n = rows_to_reach(D * 4, 2 ** 32)
    add("gather-index", n, [Arr("index", 8, 8, False), Arr("obs_out", D * 4, 4, True), Arr("lm_out", 26 * 4, 4, True), Arr("actions_out", 8, 8, True)] +
        [Arr(k, 4, 4, True) for k in ("logp_out", "advantages_out", "value_targets_out", "values_out")] + [Arr("seats_out", 1, 1, True)])
    # 5. learner targets: TARGETS_T + 1 steps of TARGETS_B four-player games; the float columns stay below every mark (byte 2^28)
    n = (TARGETS_T + 1) * TARGETS_B
    add("targets", n, [Arr("records", rb, 1, False), Arr("values", 4, 4, False), Arr("final_rewards", 4 * 8, 8, False), Arr("episode_end", 1, 1, False)] +
        [Arr(k, 4, 4, True) for k in ("advantages", "value_targets", "returns")] + [Arr("flags", 1, 1, True)])
    # 11. the collection loop: COLLECT_T + 1 steps of COLLECT_B games in one records buffer
    n = (COLLECT_T + 1) * COLLECT_B
    add("collect", n, [Arr("records", rb, 1, True), Arr("actions", 4, 4, True), Arr("logp", 4, 4, True), Arr("values", 4, 4, True),
                       Arr("final_rewards", 4 * 8, 8, True), Arr("episode_end", 1, 1, True)], extra=2 * GIB)
    return cases


# A buffer whose rows t * B + b cross byte 2^32 of 64-byte records with a game count that is neither a multiple of 64 nor of POOL (row
# content would otherwise repeat from step to step): the smallest T with T * B >= 2^26 + POOL.
WINDOW_B = 16411
WINDOW_T = -(-(2 ** 26 + POOL) // WINDOW_B)
TARGETS_B, TARGETS_T = 65536, 1025
COLLECT_B, COLLECT_T, COLLECT_SLICE = 65536, 1024, 128
# The one case whose reference is the product itself: ``rollout.collect`` into one buffer of COLLECT_T iterations against the same
# iterations collected as COLLECT_T / COLLECT_SLICE calls into a small buffer, at low offsets - the path that
# tests/test_gpu_full_batch.py::test_config5_env_side_every_record already holds to the oracle.
SELF_REFERENCED = ("collect",)
CASES = _plan()


def planned_bytes(case):
    return sum(case["n"] * a.stride + (2 * GUARD if a.out else 0) for a in case["arrays"]) + case["extra"]
