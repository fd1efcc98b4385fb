"""tests/big_rows.py without a GPU: every case of tests/test_gpu_big_rows.py crosses the marks it claims inside a window, with a row count
that is no multiple of a block, under the memory cap; and the two checks those tests rest on - the whole output against its own first
period, the windows against the reference - each reject four restated addressing slips on a toy of 3 x 4099 rows.

Every case listed in ``big_rows.CASES`` is held to a CPU restatement, never to the kernel under test at another size."""
import numpy as np
import pytest

from tests import big_rows as br


# ---------------------------------------------------------------- the plans
@pytest.mark.parametrize("name", sorted(br.CASES))
def test_case_crosses_its_marks_inside_windows(name):
    case = br.CASES[name]
    n, arrays = case["n"], case["arrays"]
    marks = br.mark_rows(n, arrays)
    assert marks, "the case crosses nothing"
    wins = br.windows(n, arrays)
    assert wins[0] == (0, br.WIDTH) and wins[-1] == (n - br.WIDTH, n)
    assert all(0 <= lo and hi <= n and hi - lo == br.WIDTH for lo, hi in wins)
    by_name = {a.name: a for a in arrays}
    for arr, label, row in marks:
        a = by_name[arr]
        _, pos, unit = next(m for m in br.MARKS if m[0] == label)
        byte = pos if unit == "byte" else pos * a.elem
        assert row * a.stride <= byte < (row + 1) * a.stride < n * a.stride + a.stride    # exact integers: the row holds the mark
        assert any(lo <= row < hi for lo, hi in wins), (arr, label, row)
        assert any(lo < row < hi - 1 for lo, hi in wins)      # with a neighbour on either side
    print(name, "n =", n, "marks:", ", ".join("%s %s row %d" % m for m in marks))


EXPECTED_MARKS = {
    "unpack-rows": {("records", "byte 2^31"), ("records", "byte 2^32"), ("records", "element 2^31"), ("obs", "byte 2^31"), ("obs", "byte 2^32"), ("obs", "element 2^31")},
    "forward-rows-fp32": {("records", "byte 2^32"), ("out", "byte 2^32")},
    "forward-planar-bf16": {("records", "byte 2^32"), ("out", "byte 2^32")},
    "sample-rows": {("logits", "element 2^31"), ("records", "byte 2^32"), ("actions", "byte 2^28"), ("logp", "byte 2^28"), ("uniform", "byte 2^28")},   # (4-byte columns of 82.6 M rows: 330 MB)
    "sample-planar": {("records", "byte 2^32"), ("logits", "byte 2^32")},
    "select": {("flags", "byte 2^31"), ("advantages", "byte 2^32"), ("advantages", "element 2^31")},
    "gather-logits-column": {("column", "byte 2^32")},
    "gather-logits-index": {("column", "byte 2^32"), ("out", "byte 2^32"), ("index", "byte 2^28")},
    "ppo-loss": {("logits", "byte 2^32"), ("log_mask", "byte 2^32"), ("grad_logits", "byte 2^32"), ("actions", "byte 2^28")},
    "ppo-loss-kl": {("logits", "byte 2^31"), ("old_logits", "byte 2^31"), ("grad_logits", "byte 2^31")},
    "episode-stats": {("final_rewards", "byte 2^32"), ("episode_end", "byte 2^27")},
}


@pytest.mark.parametrize("name", sorted(EXPECTED_MARKS))
def test_case_reaches_what_the_module_claims(name):
    case = br.CASES[name]
    n = case["n"]
    sizes = {a.name: n * a.stride for a in case["arrays"]}
    got = {(a, l) for a, l, _ in br.mark_rows(n, case["arrays"])}
    for arr, label in EXPECTED_MARKS[name]:
        if label in ("byte 2^28", "byte 2^27"):               # the small columns: stated as they are, below every mark
            assert sizes[arr] >= 2 ** int(label[-2:]), (arr, label)
        else:
            assert (arr, label) in got, (arr, label)


def test_unpack_tiles_is_unpack_rows_rounded_up_to_whole_tiles():
    a, b = br.CASES["unpack-rows"]["n"], br.CASES["unpack-tiles"]["n"]
    assert b % 64 == 0 and 0 < b - a < 64


@pytest.mark.parametrize("name", sorted(br.CASES))
def test_row_counts_strides_and_memory(name):
    case = br.CASES[name]
    n = case["n"]
    if name not in ("unpack-tiles", "collect", "targets"):    # (that call counts tiles; a rollout's rows are steps x 65 536 games)
        assert n % 64 and n % 256 and (n - br.POOL) > 0
    assert br.wrap_is_visible(case["arrays"])
    for a in case["arrays"]:                                  # and a wrap of the row id itself
        assert (2 ** 31) % br.POOL and (2 ** 32) % br.POOL
    total = br.planned_bytes(case)
    print(name, "planned %.2f GiB" % (total / br.GIB))
    assert total <= br.CAP


def test_the_smallest_counts_are_the_smallest():
    for stride, pos in ((163, 2 ** 32), (26, 2 ** 31), (104, 2 ** 32), (32, 2 ** 32)):
        n = br.rows_to_reach(stride, pos) - br.POOL
        assert n * stride >= pos > (n - 1) * stride


def test_the_window_buffer_and_the_self_referenced_case():
    B, T = br.WINDOW_B, br.WINDOW_T
    assert B % 64 and B % br.POOL and (T * B) % 64 and ((T + 1) * B) % 64
    assert (T - 1) * B < 2 ** 26 + br.POOL <= T * B           # the smallest T that reaches it
    assert T * B * 64 > 2 ** 32 + br.WIDTH * 64               # rows on either side of byte 2^32 are rows of steps 0 .. T - 1
    tiles = (B + 63) // 64
    assert (2 ** 32 // 64) % br.POOL and (tiles * 64) % br.POOL   # tile-planar slots: a step's stride is no multiple of POOL either
    # rollout.collect is compared with the product itself at low offsets, and with nothing else: it is the only such case
    assert br.SELF_REFERENCED == ("collect",) and set(br.SELF_REFERENCED) <= set(br.CASES)
    assert br.COLLECT_T % br.COLLECT_SLICE == 0 and (br.COLLECT_SLICE + 1) * br.COLLECT_B * 64 < 2 ** 31 < 2 ** 32 < br.CASES["collect"]["n"] * 64


def test_repeat_counts():
    for n in (1, br.POOL, br.POOL + 1, 3 * br.POOL + 17):
        c = br.repeat_counts(n)
        assert c.sum() == n and np.array_equal(c, np.bincount(np.arange(n) % br.POOL, minlength=br.POOL))


# ---------------------------------------------------------------- the checks can fail
def _toy_windows():
    return br.windows(br.TOY_ROWS, [br.Arr("in", br.TOY_STRIDE, 8, False), br.Arr("out", br.TOY_STRIDE, 8, True)], marks=br.TOY_MARKS)


def _periodicity_check(out):
    """What the GPU tests do for a content-only kernel: the first period against the reference, the whole against its first period."""
    import torch

    t = torch.from_numpy(out)
    first_ok = np.array_equal(out[:br.POOL], br.toy_reference(np.arange(br.POOL)))
    return first_ok and br.periodic_mismatches(t)[0] == 0


def _window_check(out):
    import torch

    bad, left = br.window_mismatches(torch.from_numpy(out), _toy_windows(), br.toy_reference, sentinel=br.TOY_SENTINEL)
    return not bad and left == 0


def test_toy_windows_cover_the_toy_marks():
    wins = _toy_windows()
    assert len(wins) == 4
    for row in (br.TOY_WRAP // 2 // br.TOY_STRIDE, br.TOY_WRAP // br.TOY_STRIDE):
        assert any(lo < row < hi - 1 for lo, hi in wins)


def test_the_right_toy_passes_both_checks():
    out = br.toy_kernel(br.TOY_ROWS)
    assert _periodicity_check(out) and _window_check(out)
    import torch

    assert br.periodic_mismatches(torch.from_numpy(out)) == (0, -1)


@pytest.mark.parametrize("slip", br.SLIPS)
def test_each_check_rejects_each_slip(slip):
    out = br.toy_kernel(br.TOY_ROWS, slip)
    assert not np.array_equal(out, br.toy_kernel(br.TOY_ROWS))
    assert not _periodicity_check(out), "the periodicity check accepts " + slip
    assert not _window_check(out), "the window check accepts " + slip


def test_periodic_mismatches_counts_and_locates():
    import torch

    out = br.toy_kernel(br.TOY_ROWS)
    out[2 * br.POOL + 5] += 1
    out[br.POOL + 7] += 1
    assert br.periodic_mismatches(torch.from_numpy(out)) == (2, br.POOL + 7)
    # against a given first period, rows below POOL count too
    out[3] += 1
    first = torch.from_numpy(br.toy_reference(np.arange(br.POOL)))
    assert br.periodic_mismatches(torch.from_numpy(out), first=first) == (3, 3)


def test_fill_periodic_is_the_modulo():
    import torch

    pool = torch.arange(7 * 3, dtype=torch.int16).view(7, 3)
    for n in (1, 6, 7, 8, 30):
        buf = br.fill_periodic(torch.full((n, 3), -1, dtype=torch.int16), pool)
        assert torch.equal(buf, pool[torch.arange(n) % 7])
