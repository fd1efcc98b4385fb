"""Learner minibatches (``skyjo_vec_rollout_select`` / ``_gather``) without a GPU: the numpy restatement of
tests/rollout_batches_ref.py against a hand-worked example of the tile-planar address and the gather, its re-layout helper against
the address function, the float32 normalisation with (0, 1), and the ABI carries the two entry points."""
import ctypes
import os
import re

import numpy as np

from tests import rollout_batches_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _counting_records(S=2, B=70, rb=64):
    """Byte k of record (s, b) is its row-major position modulo 251 (a prime: no two neighbouring pieces look alike)."""
    return (np.arange(S * B * rb, dtype=np.int64) % 251).astype(np.uint8).reshape(S, B, rb)


def test_worked_example_address_and_gather():
    """2 steps x 70 games of 64-byte records (indirect observation: D = 31, mask at 32, seat at 58): two tiles per step, the second
    one partial, so a step holds 128 record slots.  Row id 137 = step 1, game 67 is record 1 * 128 + 67 = 195: tile 3, lane 3.  Its
    byte 37 lies in piece 2 at 3 * 4096 + 2 * 1024 + 3 * 16 + 5 = 14 389; row-major it is at 137 * 64 + 37 = 8 805."""
    rows = _counting_records()
    planar = ref.to_planar(rows)
    assert planar.shape == (2, 2, 4, 64, 16)
    assert int(ref.byte(195, 37, 64, True)) == 14389 and int(ref.byte(137, 37, 64, False)) == 8805
    assert planar.reshape(-1)[14389] == rows[1, 67, 37] == 8805 % 251
    assert int(ref.byte(0, 0, 64, True)) == 0 and int(ref.byte(1, 0, 64, True)) == 16 and int(ref.byte(0, 16, 64, True)) == 1024
    assert int(ref.byte(64, 63, 64, True)) == 4096 + 3 * 1024 + 15
    # the slots of the partial tile beyond game 69 stay zero
    assert not planar[:, 1, :, 6:, :].any() and planar[:, 1, :, :6, :].any()

    T, B = 2, 70
    n = T * B
    cols = dict(actions=np.arange(n, dtype=np.int32) % 26, logp=-np.arange(n, dtype=np.float32) / 8, values=np.arange(n, dtype=np.float32),
                advantages=np.arange(n, dtype=np.float32) - 60, value_targets=np.arange(n, dtype=np.float32) * 2)
    index = np.array([137, 0, 69, 70, 137], dtype=np.int64)
    got = [ref.gather(rows, False, 64, 31, B, T, B, index, **cols), ref.gather(planar, True, 64, 31, B, T, 128, index, **cols)]
    for g in got:
        base = 137 * 64
        assert g["observations"].dtype == np.float32 and g["observations"].shape == (5, 31)
        want = ((base + np.arange(31)) % 251).astype(np.uint8).view(np.int8).astype(np.float32)
        assert np.array_equal(g["observations"][0], want) and np.array_equal(g["observations"][4], want)
        assert (want < 0).any()   # bytes above 127 are negative observations
        mask = (base + 32 + np.arange(26)) % 251
        assert np.array_equal(g["log_mask"][0], np.where(mask != 0, 0.0, ref.FLOAT_MIN).astype(np.float32))
        assert g["seats"].tolist() == [(r * 64 + 58) % 251 for r in index]
        assert g["actions"].tolist() == [137 % 26, 0, 69 % 26, 70 % 26, 137 % 26] and g["actions"].dtype == np.int64
        assert g["logp"].tolist() == [-137 / 8, 0.0, -69 / 8, -70 / 8, -137 / 8]
        assert g["advantages"].tolist() == [77.0, -60.0, 9.0, 10.0, 77.0] and g["value_targets"].tolist() == [274.0, 0.0, 138.0, 140.0, 274.0]
    # a mask byte that IS zero: row 58 starts at 3 712 = 14 * 251 + 198, so its byte 53 - mask entry 21 - is 0
    g = got[1]
    one = ref.gather(planar, True, 64, 31, B, T, 128, np.array([58]), **cols)
    assert one["log_mask"][0, 21] == np.float32(ref.FLOAT_MIN) and (np.delete(one["log_mask"][0], 21) == 0).all()
    for k in got[0]:
        assert np.array_equal(got[0][k], g[k]), k
    # rows out of range are all zero
    z = ref.gather(rows, False, 64, 31, B, T, B, np.array([n, -1, 0]), **cols)
    assert all(not v[:2].any() for v in z.values()) and z["observations"][2, 1] == 1.0


def test_relayout_round_trips_through_the_address():
    rng = np.random.default_rng(3)
    for B, rb in ((70, 64), (104, 112), (200, 208), (64, 80)):
        rows = rng.integers(0, 256, size=(3, B, rb), dtype=np.uint8)
        planar = ref.to_planar(rows)
        stride = planar.shape[1] * 64
        s, b, k = np.meshgrid(np.arange(3), np.arange(B), np.arange(rb), indexing="ij")
        back = planar.reshape(-1)[ref.byte(s * stride + b, k, rb, True)]
        assert np.array_equal(back, rows)
        assert np.array_equal(rows.reshape(-1)[ref.byte(s * B + b, k, rb, False)], rows)
        assert int(planar.astype(np.int64).sum()) == int(rows.astype(np.int64).sum())   # nothing but zeros was added


def test_normalisation_identity_and_moments():
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.standard_normal(4096).astype(np.float32) * 30, np.array([0.0, -0.0, 1e-45, -1e-45, 1.1754942e-38, -3e-42,
                                                                                   3.4028235e38, -3.4028235e38], dtype=np.float32)])
    y = ref.normalise(x, 0.0, 1.0)
    assert y.dtype == np.float32 and np.array_equal(y.view(np.uint32), x.view(np.uint32))   # bit for bit, the sign of zero too
    assert ref.normalise(np.float32([3.0]), 1.0, 4.0).tolist() == [0.5]
    flags = np.array([[1, 3, 0], [2, 1, 3]], dtype=np.uint8)
    assert ref.select(flags, 1).tolist() == [0, 1, 4, 5] and ref.select(flags, 3).tolist() == [1, 5] and ref.select(flags, 2).tolist() == [1, 3, 5]
    adv = np.array([[1, 2, 100], [100, 3, 6]], dtype=np.float32)
    s, q = ref.moments(adv, ref.select(flags, 1))
    assert (s, q) == (12.0, 50.0) and ref.mean_std(s, q, 4) == (3.0, float(np.std([1, 2, 3, 6], ddof=1)))
    assert ref.moments(adv, ref.select(flags * 0, 1)) == (0.0, 0.0) and ref.mean_std(0.0, 0.0, 0) == (0.0, 0.0)
    assert ref.mean_std(5.0, 25.0, 1) == (5.0, 0.0)


def test_abi_has_rollout_select_and_gather():
    """include/skyjo_vec.h declares both entry points, the library exports them, the ctypes table has them."""
    from skyjo_rl_amd import _lib, build

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "skyjo_vec.h")).read(), flags=re.S)
    lib = ctypes.CDLL(build.build())
    for name, nargs in (("skyjo_vec_rollout_select", 9), ("skyjo_vec_rollout_gather", 23)):
        assert re.search(r"\bint\s+%s\s*\(" % name, text)
        assert hasattr(lib, name)
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == nargs
    args = _lib.SIGNATURES["skyjo_vec_rollout_gather"][1]
    assert args[12] is ctypes.c_float and args[13] is ctypes.c_float and args[5] is ctypes.c_int64
    assert _lib.SIGNATURES["skyjo_vec_rollout_select"][1][2] is ctypes.c_int64
    assert _lib.ABI_VERSION == 4 and re.search(r"#define\s+SKYJO_ABI_VERSION\s+4\b", text)
