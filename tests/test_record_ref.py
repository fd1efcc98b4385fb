"""tests/record_ref.py without a GPU: the geometries are what the header says, ``planar_address`` is the inverse of the planar re-layout,
the generated cases reach what they claim, and the comparisons of tests/test_gpu_record_consumers.py reject two restated wrong kernels -
the episode-end kernel that reads the done byte through a pointer to the agent byte exactly where that pointer leaves the 16-byte piece,
and an unpack that takes ``status`` from the done offset everywhere."""
import numpy as np
import pytest

from tests import learner_synth, net_ref
from tests import record_ref as ref

IDS = [ref.gid(N, ind) for N, ind in ref.GEOMETRIES]


def test_geometries_are_the_headers():
    assert ref.GEOMETRIES == [(3, True), (12, True)] + [(N, False) for N in range(1, 13)]
    for N in range(1, 13):
        g = ref.geometry(N, True)
        assert (g["obs_dim"], g["mask_offset"], g["record_bytes"]) == (31, 32, 64) and (g["mask_offset"] + 26) % 16 == 10
        g = ref.geometry(N, False)
        D = 19 + 12 * N
        assert g["obs_dim"] == D and D % 2 == 1 and g["mask_offset"] == D + 1 and g["mask_offset"] + 26 == 46 + 12 * N
        assert g["record_bytes"] == -(-(g["mask_offset"] + 32) // 16) * 16
        # agent .. status in one 16-byte piece, but for N = 4, 8, 12: agent at 14 mod 16, done in the next piece
        assert ((g["mask_offset"] + 26) % 16 == 14) == ((N, False) in ref.STRADDLE)
        assert ((g["mask_offset"] + 26) // 16 != (g["mask_offset"] + 28) // 16) == ((N, False) in ref.STRADDLE)
    assert [ref.geometry(N, False)["record_bytes"] // 16 for N in (2, 3, 4)] == [5, 6, 7]
    assert [ref.geometry(N, False)["mask_offset"] for N in (2, 3, 4)] == [44, 56, 68]
    assert ref.geometry(4, False) == dict(num_players=4, obs_dim=67, mask_offset=68, record_bytes=112)
    assert sorted({ref.geometry(N, ind)["record_bytes"] // 16 for N, ind in ref.GEOMETRIES}) == [4, 5, 6, 7, 8, 9, 10, 11, 12, 13]


@pytest.mark.parametrize("N,indirect", ref.GEOMETRIES, ids=IDS)
def test_planar_address_inverts_to_planar_dirty(N, indirect):
    g = ref.geometry(N, indirect)
    rb = g["record_bytes"]
    for n in (1, 64, 130):
        rng = np.random.default_rng(n + N)
        rows = rng.integers(0, 256, size=(n, rb), dtype=np.uint8)
        planar = learner_synth.to_planar_dirty(rows[None], rng)[0]
        assert planar.shape == ((n + 63) // 64, rb // 16, 64, 16)
        addr = ref.planar_address(np.arange(n)[:, None], np.arange(rb)[None, :], rb)
        assert np.unique(addr).size == n * rb and addr.max() < planar.size
        assert np.array_equal(planar.reshape(-1)[addr], rows)
        assert np.array_equal(ref.rows_from_planar(planar, n), rows)
        pad = np.ones(planar.size, dtype=bool)
        pad[addr.reshape(-1)] = False
        assert pad.sum() == (-n % 64) * rb and (planar.reshape(-1)[pad] != 0).all()      # dirty padding
    # the header's own example: piece p of game 64 t + l at block t * 64 * record_bytes + p * 1024 + l * 16
    assert int(ref.planar_address(64 * 3 + 5, 16 * 2 + 7, rb)) == 3 * 64 * rb + 2 * 1024 + 5 * 16 + 7


def _cases():
    return [(n, N, ind, ref.case_seeds(n, N, ind)) for n, N, ind in ref.EPISODE_CASES]


def test_the_cases_are_the_issues():
    assert len(ref.EPISODE_CASES) == len(set(ref.EPISODE_CASES)) == len(ref.GEOMETRIES) + 2 * len(ref.EPISODE_EDGE_B)
    assert ref.EPISODE_EDGE_B == (1, 63, 64, 65, 256, 257, 321) and ref.EPISODE_B == 130
    # the second round of k_unpack's grid-stride loop: more elements than 4096 blocks of 256 threads
    for N, ind, tiles in ref.UNPACK_SECOND_ROUND:
        g = ref.geometry(N, ind)
        total = tiles * 64 * (g["obs_dim"] + 26)
        assert ref.UNPACK_GRID_ELEMENTS < total < 2 * ref.UNPACK_GRID_ELEMENTS
    assert [(t * 64) for _, _, t in ref.UNPACK_SECOND_ROUND] == [19200, 5632]


def test_every_case_has_ends_non_ends_and_done_rows_without_an_action():
    for n, N, ind, seeds in _cases():
        ends, rows_total, skipped_done, running_acted, done_values = 0, 0, 0, 0, set()
        for seed in seeds:
            c = ref.consumer_case(n, N, ind, seed)
            g, rows = c["geometry"], c["rows"]
            D, Dp = g["obs_dim"], g["mask_offset"]
            _, end = ref.episode_ends_ref(rows, g, np.ones((n, N)))
            ends += int(end.sum())
            rows_total += n
            skipped_done += int(((rows[:, Dp + 28] != 0) & (rows[:, D] == 0xFF)).sum())
            running_acted += int(((rows[:, Dp + 28] == 0) & (rows[:, D] != 0xFF)).sum())
            done_values |= set(rows[:, Dp + 28].tolist())
            assert (rows[:, Dp + 26] < N).all()
            assert set(rows[:, D].tolist()) <= set(range(26)) | {0xFF}
        if n == 1:
            assert ends >= 1 and running_acted >= 1 and rows_total == 3, (n, N, ind)
        else:
            assert ends * 4 >= rows_total and (rows_total - ends) * 4 >= rows_total, (n, N, ind, ends)
            assert skipped_done >= 1, (n, N, ind)
            assert {0, 1, 2, 0x80, 0xFF} <= done_values or n < 130, (n, N, ind)
            if n >= 10:
                edge = np.array(learner_synth.OBS_EDGES, dtype=np.uint8)
                assert sum(set(r[:D].tolist()) == set(edge.tolist()) for r in rows) >= 10


@pytest.mark.parametrize("N,indirect", ref.GEOMETRIES, ids=IDS)
def test_the_neighbour_pointer_is_rejected_exactly_where_it_straddles(N, indirect):
    n = ref.EPISODE_B
    c = ref.consumer_case(n, N, indirect, ref.case_seeds(n, N, indirect)[0])
    g = c["geometry"]
    rewards = ref.synthetic_rewards(n, N, np.random.default_rng(N))
    want = ref.episode_ends_ref(c["rows"], g, rewards)
    assert want[0].dtype == np.float64 and want[1].dtype == np.uint8
    assert (want[0][want[1] == 0].view(np.int64) == 0).all() and (want[0][want[1] != 0] != 0).all()      # + 0.0, and no zero row
    assert ref.same_episode_ends(ref.episode_ends_ref(ref.rows_from_planar(c["planar"], n), g, rewards), want)
    assert ref.same_episode_ends(ref.episode_ends_neighbour_pointer(c["rows"], n, g, rewards, planar=False), want)
    wrong = ref.episode_ends_neighbour_pointer(c["planar"], n, g, rewards, planar=True)
    if (N, indirect) in ref.STRADDLE:
        bad = int((wrong[1] != want[1]).sum())
        print("direct N = %d: %d of %d rows flagged wrongly" % (N, bad, n))
        assert not ref.same_episode_ends(wrong, want) and bad * 8 >= n
    else:
        assert ref.same_episode_ends(wrong, want)
    if (N, indirect) == (4, False):                                                      # one record: the dirty padding beside it gives it away
        rejected = 0
        for seed in ref.case_seeds(1, N, indirect):
            c1 = ref.consumer_case(1, N, indirect, seed)
            w1 = ref.episode_ends_ref(c1["rows"], g, rewards[:1])
            assert ref.same_episode_ends(ref.episode_ends_neighbour_pointer(c1["rows"], 1, g, rewards[:1], planar=False), w1)
            rejected += not ref.same_episode_ends(ref.episode_ends_neighbour_pointer(c1["planar"], 1, g, rewards[:1], planar=True), w1)
        assert rejected >= 1
    # the comparison itself: a - 0.0 where + 0.0 belongs, one flag, one reward bit
    for change in ("sign", "flag", "bit"):
        fr, ee = want[0].copy(), want[1].copy()
        if change == "sign":
            fr[np.flatnonzero(ee == 0)[0], 0] = -0.0
        elif change == "flag":
            ee[n - 1] ^= 1
        else:
            fr.view(np.int64)[np.flatnonzero(ee)[0], N - 1] ^= 1
        assert not ref.same_episode_ends((fr, ee), want), change


@pytest.mark.parametrize("N,indirect", ref.GEOMETRIES, ids=IDS)
def test_the_status_from_done_unpack_is_rejected_everywhere(N, indirect):
    n = ref.UNPACK_ROWS
    c = ref.consumer_case(n, N, indirect, 100 + N)
    g = c["geometry"]
    want = ref.unpack_ref(c["rows"], g)
    assert [want[k].dtype for k in ref.UNPACK_NAMES] == [np.int8, np.int8] + [np.uint8] * 4
    assert want["obs"].shape == (n, g["obs_dim"]) and want["mask"].shape == (n, 26) and all(want[k].shape == (n,) for k in ref.UNPACK_NAMES[2:])
    assert ref.unpack_mismatches(ref.unpack_ref(ref.rows_from_planar(c["planar"], n), g), want) == []
    assert ref.unpack_mismatches(ref.unpack_status_from_done(c["rows"], g), want) == ["status"]
    assert ref.unpack_mismatches({"mask": want["mask"]}, want) == []                     # (a NULL output is not compared)
    # every field is its own bytes: the four meta bytes of a row differ somewhere, and so do the edges of the observation and the mask
    meta = np.stack([want[k] for k in ref.UNPACK_NAMES[2:]])
    assert all((meta[i] != meta[j]).any() for i in range(4) for j in range(i))
    assert want["obs"].min() == -128 and want["obs"].max() == 127 and {0, 1, 2, -128, -1} <= set(want["mask"].reshape(-1).tolist())


def test_draw_cases_of_every_geometry_are_the_64_byte_case():
    """``record_bytes`` / ``mask_offset`` change where the mask lies, not the masks, the logits or the uniforms: the share of ambiguous
    rows is the one tests/test_net_ref.py bounds (at most 26 steps x 2e-5 of the rows for a uniform u; the cap 2e-3)."""
    seed, ticket = 77, 5
    base = net_ref.draw_case(6553, seed, ticket)
    share = float(base["ref"]["ambiguous"].mean())
    assert share <= 2e-3
    for N, indirect in ref.GEOMETRIES:
        g = ref.geometry(N, indirect)
        c = ref.draw_case(6553, seed, ticket, g)
        Dp = g["mask_offset"]
        assert c["records"].shape == (6553, g["record_bytes"]) and (c["mask_offset"], c["obs_dim"]) == (Dp, g["obs_dim"])
        assert np.array_equal(c["records"][:, Dp:Dp + 26], c["mask"])
        for k in ("mask", "mask_family", "logits", "logit_family", "u"):
            assert np.array_equal(c[k], base[k]), (N, indirect, k)
        assert np.array_equal(c["ref"]["ambiguous"], base["ref"]["ambiguous"]) and np.array_equal(c["ref"]["action"], base["ref"]["action"])
        assert float(c["ref"]["ambiguous"].mean()) == share
        if g["record_bytes"] != 64:                                                      # the other bytes are random, not a copy
            assert not np.array_equal(c["records"][:, :32], base["records"][:, :32])


def test_arena_records_carry_every_seat_and_mask_family():
    for N in ref.ARENA_N:
        g = ref.geometry(N, True)
        rec, mask, agent = ref.arena_records(ref.ARENA_B, g, np.random.default_rng(N))
        assert rec.shape == (ref.ARENA_B, 64) and np.array_equal(rec[:, 32:58], mask) and np.array_equal(rec[:, 58], agent)
        assert set(agent.tolist()) == set(range(N)) and set(mask.reshape(-1).tolist()) == {0, 1}
        fam = np.arange(ref.ARENA_B) % len(net_ref.MASK_FAMILIES)
        for s in range(N):
            assert (agent == s).sum() >= 10
            if N <= 4:                                                                   # every seat meets every family, the empty mask included
                assert {0, 26} <= set(mask[agent == s].sum(1).tolist()) and len(set(fam[agent == s].tolist())) == len(net_ref.MASK_FAMILIES)
