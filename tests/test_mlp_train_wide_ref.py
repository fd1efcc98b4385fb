"""The wide training branches' helper (tests/mlp_train_wide_ref.py): the padded-width rule and the workspace size against the figures
the header states, the inputs' promised properties, the recorded float32 deviation that tests/test_gpu_mlp_train_wide.py bounds the
kernels with - measured afresh by the host-independent evaluation - and the new names' presence in the header, the signature table,
``learner`` and the example.  No GPU needed."""
import os
import re

import numpy as np
import pytest

from tests import mlp_train_ref, mlp_train_wide_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("skyjo_vec_mlp_train_wide_workspace_bytes", "skyjo_vec_mlp_train_wide_forward", "skyjo_vec_mlp_train_wide_backward")


def test_padded_width_and_record_size():
    assert [ref.padded_width(d) for d in (32, 39, 40, 43, 67, 163)] == [40, 40, 48, 48, 72, 168]
    assert ref.padded_width(31) == 32                                     # the rule gives the narrow kernels' width at their limit
    assert ref.PART_FIXED == 74016 and ref.PART_FIXED + 256 * 32 == 82208  # ... and their record
    for d in range(ref.MIN_OBS, ref.MAX_OBS + 1):
        k = ref.padded_width(d)
        assert k % 8 == 0 and d < k <= d + 8                              # a multiple of the k-group, at least one free column
        assert ref.part_floats(d) == 74016 + 256 * k
    assert ref.workspace_bytes(43, 26, 1) == 4 * (4 * 256 + 74016 + 256 * 48)
    assert ref.workspace_bytes(163, 32, 257) == 4 * (4 * 257 * 256 + 2 * (74016 + 256 * 168))
    assert ref.workspace_bytes(67, 1, 256) == 4 * (4 * 256 * 256 + 74016 + 256 * 72)
    for bad in ((31, 26, 5), (164, 26, 5), (0, 26, 5), (43, 0, 5), (43, 33, 5), (43, 26, 0), (43, 26, -1), (43, 26, (1 << 30) + 1)):
        assert ref.workspace_bytes(*bad) == 0
    x = np.arange(6, dtype=np.float32).reshape(2, 3) + 1
    assert ref.padded_x(x).tolist() == [[1, 2, 3, 0, 0, 0, 0, 1], [4, 5, 6, 0, 0, 0, 0, 1]]
    x39 = np.full((1, 39), 7, dtype=np.float32)
    assert ref.padded_x(x39).shape == (1, 40) and (ref.padded_x(x39)[0, :39] == 7).all() and ref.padded_x(x39)[0, 39] == 1  # no zero column


def test_cases_are_the_issue_s():
    assert ref.SHAPES_WIDE == ((32, 26), (39, 26), (40, 1), (43, 26), (67, 26), (67, 1), (163, 26), (163, 32))
    assert ref.ROW_COUNTS_WIDE == (1, 2, 63, 64, 65, 255, 256, 257, 1025)
    assert ref.WEIGHT_SETS == ("A", "S")
    assert ref.FLOAT_X_CASE_WIDE[0] in ref.SHAPES_WIDE and ref.FLOAT_X_CASE_WIDE[1] in ref.ROW_COUNTS_WIDE


def test_inputs_are_what_they_promise():
    from skyjo_rl_amd import learner

    assert (ref.TILE_ROWS, ref.CHUNK_ROWS) == (learner.TRAIN_TILE_ROWS, learner.TRAIN_CHUNK_ROWS)
    for n in (learner.TRAIN_TILE_ROWS, learner.TRAIN_CHUNK_ROWS):
        assert {n - 1, n, n + 1} <= set(ref.ROW_COUNTS_WIDE)
    assert max(ref.ROW_COUNTS_WIDE) > 4 * learner.TRAIN_CHUNK_ROWS
    for shape in ref.SHAPES_WIDE:
        assert ref.MIN_OBS <= shape[0] <= ref.MAX_OBS
        for m in ref.ROW_COUNTS_WIDE:
            x, g = ref.inputs(shape, m)
            assert x.dtype == g.dtype == np.float32 and x.shape == (m, shape[0]) and g.shape == (m, shape[1])
            integer = bool((x == np.round(x)).all())
            assert integer != ((shape, m) == ref.FLOAT_X_CASE_WIDE)
            if integer:
                assert x.min() >= -2 and x.max() <= 12
            assert (g[4::5] == 0).all() and g[4::5].shape[0] == m // 5
            assert np.abs(g).max() > 0                                  # no case is all zero: every output has a scale
            if shape[1] == 26:
                assert (g[:, list(ref.ZERO_COLUMNS)] == 0).all()
        # set S saturates a good share of layer 1 in float32 - tanh rounds to +-1, so 1 - h^2 is exactly 0 - and set A less: torch's init
        # scales W1 by 1 / sqrt(obs_dim), so the pre-activation's spread does not depend on the width
        x, _ = ref.inputs(shape, 1025)
        share, spread = {}, {}
        for ws in ref.WEIGHT_SETS:
            w1, b1 = ref.weights(shape, ws)[:2]
            z = (x @ w1.T + b1).astype(np.float32)
            share[ws], spread[ws] = float((np.abs(np.tanh(z)) == 1.0).mean()), float(z.std())
        print(shape, "saturated", share, "spread of z", spread)
        assert share["S"] > 0.2 and share["A"] < share["S"]


def test_weights_are_the_narrow_recipe():
    for shape in ref.SHAPES_WIDE:
        a, s = ref.weights(shape, "A"), ref.weights(shape, "S")
        assert [t.shape for t in a] == [(256, shape[0]), (256,), (256, 256), (256,), (shape[1], 256), (shape[1],)]
        assert (s[0] == a[0] * np.float32(mlp_train_ref.SATURATE)).all() and all((p == q).all() for p, q in zip(a[1:], s[1:]))


def test_float32_restatement_is_close_to_the_definition():
    """``numpy_float32`` is the definition: on a small case in which every sum is exact (integers, powers of two) it equals float64."""
    rng = np.random.default_rng(0)
    p = [rng.integers(-2, 3, s).astype(np.float32) / 4 for s in ((256, 32), (256,), (256, 256), (256,), (3, 256), (3,))]
    x, g = rng.integers(-2, 3, (5, 32)).astype(np.float32), rng.integers(-2, 3, (5, 3)).astype(np.float32)
    got, want = ref.numpy_float32(p, x, g), mlp_train_ref.forward_backward(p, x, g)
    for k in ref.OUTPUTS:
        assert got[k].dtype == np.float32 and got[k].shape == want[k].shape
        assert mlp_train_ref.normalised_deviation(got[k], want[k]) <= 1e-5, k
    assert (got["b3"] == want["b3"]).all() and (got["w1"] != 0).any()


def test_recorded_float32_deviation():
    """(b) afresh: it must not exceed the record, and no entry may be 0.  (a), torch on this host's CPU, is printed, never asserted."""
    fresh = ref.float32_deviation()
    for ws in ref.WEIGHT_SETS:
        print("(b)", ws, " ".join("%s %.3e" % kv for kv in fresh[ws].items()))
        assert set(ref.F32_DEVIATION_WIDE[ws]) == set(ref.OUTPUTS)
        for k in ref.OUTPUTS:
            assert ref.F32_DEVIATION_WIDE[ws][k] > 0.0, (ws, k)
            assert fresh[ws][k] <= ref.F32_DEVIATION_WIDE[ws][k], (ws, k, fresh[ws][k])
            assert fresh[ws][k] > 0.0, (ws, k)   # (a case that float32 evaluates exactly would bound nothing)
    torch_dev = ref.torch_float32_deviation(1)
    for ws in ref.WEIGHT_SETS:
        print("(a), one thread", ws, " ".join("%s %.3e" % kv for kv in torch_dev[ws].items()))


def test_abi_names_in_header_and_table():
    from skyjo_rl_amd import _lib

    raw = open(os.path.join(ROOT, "include", "skyjo_vec.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for n in NAMES:
        assert re.search(r"\b" + n + r"\s*\(", text), n + " is not declared in include/skyjo_vec.h"
        assert n in _lib.SIGNATURES
        assert _lib.SIGNATURES[n] == _lib.SIGNATURES[n.replace("_wide", "")]     # the same parameter lists as the narrow entries
    assert _lib.ABI_VERSION == 4 and "#define SKYJO_ABI_VERSION 4" in raw          # the ABI only gained functions
    assert "K = 8 (obs_dim / 8 + 1)" in raw and "74 016 + 256 K" in raw


def test_wide_branch_imports_and_flag_values():
    from examples.ppo import ppo_update
    from skyjo_rl_amd import learner

    assert issubclass(learner.NativeWideBranch, learner.NativeBranch) and callable(learner.native_branch)
    assert learner.NativeBranch.OBS_RANGE == (1, 31) and learner.NativeWideBranch.OBS_RANGE == (ref.MIN_OBS, ref.MAX_OBS)
    assert set(learner.NativeWideBranch._ENTRIES) == set(NAMES)
    with pytest.raises(ValueError, match="native_loss"):
        ppo_update(None, None, None, native_nets="auto")
    with pytest.raises(ValueError, match="native_nets"):
        ppo_update(None, None, None, gae=(0.99, 1.0), native_batches=True, native_loss=True, native_nets="wide")
    with pytest.raises(ValueError, match="NativeAdam"):          # "auto" satisfies native_update's need for native nets: the optimizer is what is missing
        ppo_update(None, None, None, gae=(0.99, 1.0), native_batches=True, native_loss=True, native_nets="auto", shuffle="native",
                   native_update=True)
