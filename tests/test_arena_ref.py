"""The arena's surface without a GPU: the numpy restatements of tests/arena_ref.py on hand-made cases, the new symbols and the seat
struct against include/skyjo_vec.h, the ctypes table, and ``arena.seat_policies``' validation on a stub engine."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from tests import arena_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("skyjo_vec_arena_workspace_bytes", "skyjo_vec_arena_select", "skyjo_vec_arena_rollout",
       "skyjo_vec_episode_stats_scratch_bytes", "skyjo_vec_episode_stats")


# ---------------------------------------------------------------- the restatements
def test_greedy_is_the_first_maximum_of_the_masked_logits():
    logits = np.zeros((5, 26), dtype=np.float32)
    mask = np.zeros((5, 26), dtype=np.int8)
    logits[0, [3, 7]] = 2.0, 2.0          # a tie among legal actions: the smaller index
    mask[0, [3, 7, 9]] = 1
    logits[1, 4] = 9.0                    # the largest logit is illegal
    logits[1, 20] = -5.0
    mask[1, [20, 25]] = 1                 # 25 has logit 0 > -5
    mask[2, [11, 12]] = 1                 # all logits equal: the smallest legal index
    logits[3] = np.arange(26)             # an empty mask: every m is FLOAT_MIN (the logits are absorbed) - index 0
    logits[4] = -np.arange(26)
    mask[4, 25] = 1                       # one legal action with the lowest logit
    assert arena_ref.greedy_actions(logits, mask).tolist() == [3, 25, 11, 0, 25]
    m = arena_ref.masked_logits(logits, mask)
    assert m.dtype == np.float32 and m[3, 5] == arena_ref.FLOAT_MIN and m[0, 3] == np.float32(2.0)


def test_masked_logits_round_in_float32():
    # 1e32 + FLOAT_MIN is not FLOAT_MIN in float32: the addition is made, and made in float32
    logits = np.full((1, 26), 1e32, dtype=np.float32)
    mask = np.zeros((1, 26), dtype=np.int8)
    want = np.float32(1e32) + arena_ref.FLOAT_MIN
    assert want != arena_ref.FLOAT_MIN and arena_ref.masked_logits(logits, mask)[0, 0] == want


def test_episode_statistics_restatement():
    fr = np.array([[1.0, 2.0, 2.0], [9.0, 9.0, 9.0], [-1.5, -0.25, -3.0], [0.5, 0.5, 0.5], [4.0, 1.0, 0.0]])
    end = np.array([1, 0, 1, 1, 1], dtype=np.uint8)
    n, s, q, w = arena_ref.episode_sums(fr, end)
    assert n == 4
    assert s.tolist() == [4.0, 3.25, -0.5]
    assert q.tolist() == [1.0 + 2.25 + 0.25 + 16.0, 4.0 + 0.0625 + 0.25 + 1.0, 4.0 + 9.0 + 0.25]
    assert w.tolist() == [2, 3, 2]        # row 0: seats 1 and 2 tie, row 3: all three tie
    n, mean, std, win = arena_ref.episode_stats(fr, end)
    assert np.array_equal(mean, s / 4) and np.array_equal(win, np.array([0.5, 0.75, 0.5]))
    assert np.allclose(std, np.std(fr[end != 0], axis=0, ddof=1), rtol=1e-14)
    n, mean, std, win = arena_ref.episode_stats(fr, np.zeros(5, dtype=np.uint8))
    assert n == 0 and not mean.any() and not std.any() and not win.any()
    n, mean, std, win = arena_ref.episode_stats(fr, np.array([0, 0, 1, 0, 0], dtype=np.uint8))
    assert n == 1 and mean.tolist() == [-1.5, -0.25, -3.0] and not std.any() and win.tolist() == [0.0, 1.0, 0.0]


def test_stats_from_sums_matches_the_restatement():
    from skyjo_rl_amd import arena

    rng = np.random.default_rng(3)
    fr = rng.normal(size=(40, 4)) * 3.0
    end = (rng.random(40) < 0.6).astype(np.uint8)
    n, s, q, w = arena_ref.episode_sums(fr, end)
    flat = [float(n)]
    for k in range(4):
        flat += [s[k], q[k], float(w[k])]
    got = arena.stats_from_sums(flat, 4)
    rn, rmean, rstd, rwin = arena_ref.episode_stats(fr, end)
    assert got.episodes == rn and isinstance(got.episodes, int)
    assert np.array_equal(got.mean_reward, rmean) and np.array_equal(got.win_rate, rwin)
    assert np.allclose(got.std_reward, rstd, rtol=1e-15, atol=0.0)
    one = arena.stats_from_sums([1.0, 2.0, 4.0, 1.0, -1.0, 1.0, 0.0], 2)
    assert one == arena.EpisodeStats(1, (2.0, -1.0), (0.0, 0.0), (1.0, 0.0))
    none = arena.stats_from_sums([0.0] * 7, 2)
    assert none == arena.EpisodeStats(0, (0.0, 0.0), (0.0, 0.0), (0.0, 0.0))
    assert math.isclose(arena.stats_from_sums([2.0, 4.0, 10.0, 1.0], 1).std_reward[0], math.sqrt(2.0))


# ---------------------------------------------------------------- the C surface
def test_header_declares_the_arena_and_the_library_exports_it():
    from skyjo_rl_amd import build

    text = open(os.path.join(ROOT, "include", "skyjo_vec.h")).read()
    lib = ctypes.CDLL(build.build())
    for name in NEW:
        assert name + "(" in text.replace(" (", "("), name
        assert hasattr(lib, name), name


def test_python_declares_the_five_functions():
    from skyjo_rl_amd import _lib

    for name in NEW:
        assert name in _lib.SIGNATURES, name
    I32, I64, U64, VP = ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64, ctypes.c_void_p
    SP, RB = ctypes.POINTER(_lib.SeatPolicy), ctypes.POINTER(_lib.RolloutBuffers)
    assert _lib.SIGNATURES["skyjo_vec_arena_workspace_bytes"] == (I64, [VP, I32])
    assert _lib.SIGNATURES["skyjo_vec_arena_select"] == (ctypes.c_int, [VP, SP, VP, I32, U64, U64, VP, VP, I64, VP])
    assert _lib.SIGNATURES["skyjo_vec_arena_rollout"] == (ctypes.c_int, [VP, SP, I32, U64, U64, RB, VP, I64, VP])
    assert _lib.SIGNATURES["skyjo_vec_episode_stats_scratch_bytes"] == (I64, [I64, I32])
    assert _lib.SIGNATURES["skyjo_vec_episode_stats"] == (ctypes.c_int, [VP, VP, I64, I32, VP, VP, I64, VP])


def test_seat_struct_and_constants_match_the_header(tmp_path):
    from skyjo_rl_amd import _lib

    src = tmp_path / "seat.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "skyjo_vec.h"\nint main(){printf("%zu %zu %zu %zu %d %d %d %d\\n",'
                   "sizeof(skyjo_vec_seat_policy),offsetof(skyjo_vec_seat_policy,net),offsetof(skyjo_vec_seat_policy,kind),"
                   "offsetof(skyjo_vec_seat_policy,reserved),SKYJO_SEAT_SAMPLE,SKYJO_SEAT_GREEDY,SKYJO_SEAT_RANDOM,"
                   "SKYJO_ABI_VERSION);return 0;}\n")
    exe = tmp_path / "seat"
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    S = _lib.SeatPolicy
    assert got == [ctypes.sizeof(S), S.net.offset, S.kind.offset, S.reserved.offset, _lib.SEAT_SAMPLE, _lib.SEAT_GREEDY,
                   _lib.SEAT_RANDOM, _lib.ABI_VERSION]
    assert _lib.ABI_VERSION == 4   # the arena only adds functions


# ---------------------------------------------------------------- seat_policies on a stub
class _Env:
    num_players = 3


class _Net:
    def __init__(self, h):
        self._h = ctypes.c_void_p(h) if h else None


def test_seat_policies_builds_the_array_and_keeps_the_nets():
    import skyjo_rl_amd
    from skyjo_rl_amd import _lib, arena

    assert skyjo_rl_amd.arena is arena
    a, b = _Net(0x1000), _Net(0x2000)
    sp = arena.seat_policies(_Env, [("greedy", a), ("sample", b), "random"])
    assert len(sp) == 3 and isinstance(sp[0], _lib.SeatPolicy)
    assert [(s.net, s.kind, s.reserved) for s in sp] == [(0x1000, _lib.SEAT_GREEDY, 0), (0x2000, _lib.SEAT_SAMPLE, 0), (None, _lib.SEAT_RANDOM, 0)]
    assert sp.nets == [a, b]
    sp = arena.seat_policies(_Env, [("sample", a), ("greedy", a), ("random", None)])
    assert sp.nets == [a] and [s.net for s in sp] == [0x1000, 0x1000, None]
    sp = arena.seat_policies(_Env, ["random"] * 3)
    assert sp.nets == [] and all(s.net is None and s.kind == _lib.SEAT_RANDOM for s in sp)


@pytest.mark.parametrize("seats,what", [
    (["random", "random"], "entries"),
    (["random"] * 4, "entries"),
    (["random", "random", "argmax"], "is not"),
    (["random", "random", ("argmax", _Net(1))], "is not"),
    (["random", "random", 7], "is not"),
    (["random", "random", ("greedy", _Net(0))], "closed"),
    (["random", "random", ("sample", None)], "needs a FusedNet"),
    (["random", "random", "greedy"], "needs a FusedNet"),
    (["random", "random", ("random", _Net(1))], "takes no net"),
], ids=["short", "long", "unknown_kind", "unknown_kind_with_net", "not_a_seat", "closed_net", "no_net", "bare_greedy", "net_with_random"])
def test_seat_policies_rejects(seats, what):
    from skyjo_rl_amd import arena

    with pytest.raises(ValueError, match=what):
        arena.seat_policies(_Env, seats)
