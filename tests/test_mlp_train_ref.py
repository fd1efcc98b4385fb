"""The float64 restatement of a branch's training forward and backward (tests/mlp_train_ref.py) against torch's autograd, the
recorded float32 deviation that tests/test_gpu_mlp_train.py bounds the kernels with, the inputs' promised properties, and the new
names' presence in the header, the signature table, ``learner`` and the example - no GPU needed."""
import os
import re

import numpy as np
import pytest

from tests import mlp_train_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("skyjo_vec_mlp_train_workspace_bytes", "skyjo_vec_mlp_train_forward", "skyjo_vec_mlp_train_backward")


@pytest.mark.parametrize("wset", ref.WEIGHT_SETS)
@pytest.mark.parametrize("shape", ref.SHAPES)
def test_restatement_equals_autograd_in_float64(shape, wset):
    import torch

    for m in (1, 65, 257):
        x, g = ref.inputs(shape, m)
        want = ref.torch_forward_backward(ref.weights(shape, wset), x, g, torch.float64)
        got = ref.reference(shape, wset, m)
        for k in ref.OUTPUTS:
            assert got[k].shape == want[k].shape
            assert ref.normalised_deviation(got[k], want[k]) <= 1e-12, (k, m)


def test_recorded_float32_deviation():
    fresh = ref.float32_deviation()
    for ws in ref.WEIGHT_SETS:
        print(ws, " ".join("%s %.3e" % kv for kv in fresh[ws].items()))
        assert set(ref.F32_DEVIATION[ws]) == set(ref.OUTPUTS)
        for k in ref.OUTPUTS:
            assert ref.F32_DEVIATION[ws][k] > 0.0, (ws, k)
            assert fresh[ws][k] <= ref.F32_DEVIATION[ws][k], (ws, k, fresh[ws][k])
            assert fresh[ws][k] > 0.0, (ws, k)   # (a case that float32 evaluates exactly would bound nothing)


def test_inputs_are_what_they_promise():
    from skyjo_rl_amd import learner

    assert (ref.TILE_ROWS, ref.CHUNK_ROWS) == (learner.TRAIN_TILE_ROWS, learner.TRAIN_CHUNK_ROWS)
    for n in (learner.TRAIN_TILE_ROWS, learner.TRAIN_CHUNK_ROWS):
        assert {n - 1, n, n + 1} <= set(ref.ROW_COUNTS)
    assert {1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1025, 4097} <= set(ref.ROW_COUNTS)
    for shape in ref.SHAPES:
        for m in ref.ROW_COUNTS:
            x, g = ref.inputs(shape, m)
            assert x.dtype == g.dtype == np.float32 and x.shape == (m, shape[0]) and g.shape == (m, shape[1])
            integer = bool((x == np.round(x)).all())
            assert integer != ((shape, m) == ref.FLOAT_X_CASE)
            if integer:
                assert x.min() >= -128 and x.max() <= 127
            assert (g[4::5] == 0).all() and g[4::5].shape[0] == m // 5
            assert np.abs(g).max() > 0                                  # no case is all zero: every output has a scale
            if shape[1] == 26:
                assert (g[:, list(ref.ZERO_COLUMNS)] == 0).all()
        # set S saturates a good share of layer 1 in float32 - tanh rounds to +-1, so 1 - h^2 is exactly 0 - and set A does not
        x, _ = ref.inputs(shape, 1025)
        share = {}
        for ws in ref.WEIGHT_SETS:
            w1, b1 = ref.weights(shape, ws)[:2]
            h1 = np.tanh((x @ w1.T + b1).astype(np.float32))
            share[ws] = float((np.abs(h1) == 1.0).mean())
        print(shape, share)
        assert share["S"] > 0.2 and share["A"] < share["S"]


def test_abi_names_in_header_and_table():
    from skyjo_rl_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "skyjo_vec.h")).read(), flags=re.S)
    for n in NAMES:
        assert re.search(r"\b" + n + r"\s*\(", text), n + " is not declared in include/skyjo_vec.h"
        assert n in _lib.SIGNATURES
    assert _lib.ABI_VERSION == 4 and "#define SKYJO_ABI_VERSION 4" in open(os.path.join(ROOT, "include", "skyjo_vec.h")).read()
    assert len(_lib.SIGNATURES["skyjo_vec_mlp_train_forward"][1]) == 9 and len(_lib.SIGNATURES["skyjo_vec_mlp_train_backward"][1]) == 10


def test_native_branch_imports_and_flag_order():
    from examples.ppo import ppo_update
    from skyjo_rl_amd import learner

    assert callable(learner.NativeBranch) and hasattr(learner.NativeBranch, "apply")
    with pytest.raises(ValueError):
        ppo_update(None, None, None, gae=(0.99, 1.0), native_batches=True, native_loss=False, native_nets=True)
    with pytest.raises(ValueError):
        ppo_update(None, None, None, native_nets=True)
