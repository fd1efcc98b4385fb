"""The epoch order and the one-call PPO update, as far as a machine without a GPU can check them: the numpy restatement of the
permutation (tests/epoch_order_ref.py) against the values pinned when it was designed, its bijectivity, walk lengths and mixing; the three
new symbols in the header and in ``_lib.SIGNATURES``, the argument struct's size against the C compiler's; the argument checks of
``skyjo_vec_rollout_shuffle`` and ``skyjo_vec_ppo_update``, which precede every device call; and ``ppo_update``'s new keywords."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import epoch_order_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "skyjo_vec.h")
NEW_SYMBOLS = ("skyjo_vec_rollout_shuffle", "skyjo_vec_ppo_update_workspace_bytes", "skyjo_vec_ppo_update")

# what tests/test_gpu_ppo_update_native.py runs the kernel on
GPU_COUNTS = (1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 65537)
GPU_SEEDS = (0, 1, 2 ** 63 + 5, 2 ** 64 - 1)
GPU_EPOCHS = (0, 1, 2 ** 31)


def test_pinned_keys_and_permutations():
    assert ["%08x" % k for k in ref.keys(11, 0)] == "93a0fe04 48785e94 fb8122da 5893358f 20901c40 98cafc16".split()
    assert ref.perm(10, 11, 0).tolist() == [5, 6, 3, 2, 0, 1, 7, 8, 9, 4]
    assert ref.perm(10, 11, 1).tolist() == [5, 1, 0, 4, 9, 7, 3, 8, 6, 2]
    assert ref.perm(17, 2 ** 63 + 5, 2 ** 31).tolist() == [15, 7, 6, 13, 12, 5, 8, 16, 9, 0, 10, 11, 2, 1, 14, 3, 4]
    assert ref.perm(5, 2 ** 64 - 1, 0).tolist() == [2, 4, 0, 3, 1]


def _is_bijection(p):
    return p.min() >= 0 and np.array_equal(np.sort(p), np.arange(p.size))


def test_bijection_for_every_small_count_and_short_walks():
    longest = 0
    for count in range(1, 2049):
        p, walks = ref.perm(count, 7, 3, walks=True)
        assert _is_bijection(p), count
        longest = max(longest, int(walks.max()))
    print("longest walk, counts 1 .. 2048 at (7, 3):", longest)
    assert longest <= 64


def test_bijection_for_the_gpu_tests_inputs_and_short_walks():
    longest = 0
    for count in GPU_COUNTS:
        for seed in GPU_SEEDS:
            for epoch in GPU_EPOCHS:
                p, walks = ref.perm(count, seed, epoch, walks=True)
                assert _is_bijection(p), (count, seed, epoch)
                longest = max(longest, int(walks.max()))
    print("longest walk over the GPU test's inputs:", longest)
    assert longest <= 64


def test_mixing_at_4096():
    """The 16 x 16 table (j >> 8, perm(j) >> 8) against uniform: chi-square with 225 degrees of freedom (mean 225, standard deviation
    21.2) for 32 seeds; few fixed points; two epochs of one seed agree almost nowhere."""
    count, chis = 4096, []
    j = np.arange(count)
    for s in range(1000, 1032):
        p = ref.perm(count, s, s % 4)
        table = np.zeros((16, 16))
        np.add.at(table, (j >> 8, p >> 8), 1)
        expected = count / 256.0
        chis.append(float(((table - expected) ** 2 / expected).sum()))
    print("chi-square min %.1f mean %.1f max %.1f" % (min(chis), sum(chis) / len(chis), max(chis)))
    assert max(chis) < 330
    assert 195 <= sum(chis) / len(chis) <= 255
    p0, p1 = ref.perm(count, 1000, 0), ref.perm(count, 1000, 1)
    fixed, same = int((p0 == j).sum()), int((p0 == p1).sum())
    print("fixed points %d, positions shared by epochs 0 and 1: %d" % (fixed, same))
    assert fixed < 16 and same < 16


def test_order_is_index_of_perm():
    index = 3 * np.arange(17, dtype=np.int64) + 7
    assert np.array_equal(ref.order(index, 5, 2), index[ref.perm(17, 5, 2)])


def test_symbols_in_header_and_signatures():
    from skyjo_rl_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES, name
    assert re.search(r"#define\s+SKYJO_UPDATE_STATS\s+10\b", text) and _lib.UPDATE_STATS == 10


def test_update_args_size_matches_header(tmp_path):
    from skyjo_rl_amd import _lib

    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "skyjo_vec.h"\nint main(){printf("%zu %d\\n",sizeof(skyjo_vec_ppo_update_args),SKYJO_UPDATE_STATS);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, stats = (int(x) for x in subprocess.check_output([str(exe)]).split())
    assert size == C.sizeof(_lib.PPOUpdateArgs) and stats == _lib.UPDATE_STATS


@pytest.fixture(scope="module")
def lib():
    from skyjo_rl_amd import _lib, build

    build.build()
    return _lib.load()


def test_shuffle_refuses_bad_arguments_before_any_device_call(lib):
    """Host memory stands in for device memory: a refused call launches nothing and touches none of it."""
    from skyjo_rl_amd import _lib

    cells = (C.c_int64 * 64)(*range(64))
    base = C.addressof(cells)
    index, order, fault = base, base + 32 * 8, base + 63 * 8
    shuffle = lib.skyjo_vec_rollout_shuffle
    assert shuffle(None, 8, 1, 0, order, fault, None) == _lib.E_INVALID
    assert shuffle(index, 8, 1, 0, None, fault, None) == _lib.E_INVALID
    assert shuffle(index, 8, 1, 0, order, None, None) == _lib.E_INVALID
    assert shuffle(index, -1, 1, 0, order, fault, None) == _lib.E_INVALID
    assert shuffle(index, 2 ** 30 + 1, 1, 0, order, fault, None) == _lib.E_INVALID
    assert shuffle(index, 8, 1, 0, index, fault, None) == _lib.E_INVALID          # the same array
    assert shuffle(index, 8, 1, 0, index + 4 * 8, fault, None) == _lib.E_INVALID  # overlapping
    assert shuffle(index + 4 * 8, 8, 1, 0, index, fault, None) == _lib.E_INVALID
    assert shuffle(index, 8, 1, 0, order + 4, fault, None) == _lib.E_INVALID      # misaligned
    assert b"skyjo_vec_rollout_shuffle" in lib.skyjo_vec_last_error()
    assert list(cells) == list(range(64))


def test_update_refuses_null_handle_and_null_args(lib):
    from skyjo_rl_amd import _lib

    cells = (C.c_int64 * 64)()
    base = C.addressof(cells)
    args = _lib.PPOUpdateArgs()
    assert lib.skyjo_vec_ppo_update(None, C.byref(args), base, 256, base + 256, base + 504, None) == _lib.E_INVALID
    assert lib.skyjo_vec_ppo_update(base, None, base, 256, base + 256, base + 504, None) == _lib.E_INVALID
    assert lib.skyjo_vec_ppo_update_workspace_bytes(None, 10, 4, 0) == 0


@pytest.mark.parametrize("kw", [dict(shuffle="sorted"), dict(shuffle="native"),
                                dict(native_update=True, gae=(0.99, 0.95), native_batches=True, native_loss=True, native_nets=True),
                                dict(native_update=True, gae=(0.99, 0.95), native_batches=True, native_loss=True, shuffle="native"),
                                dict(native_update=True, gae=(0.99, 0.95), native_batches=True, native_loss=True, native_nets=True, shuffle="native")])
def test_ppo_update_keyword_checks_come_first(kw):
    """An unknown shuffle, a native shuffle without native batches, and ``native_update`` without the native shuffle, without the native
    nets, or with a torch optimizer: ``ValueError`` before the buffer (None here) or any native call is touched."""
    import torch

    from examples.ppo import ppo_update
    from skyjo_rl_amd.action_mask_model import ActionMaskModel

    model = ActionMaskModel(obs_dim=31)
    with pytest.raises(ValueError, match="shuffle|native_update"):
        ppo_update(model, None, torch.optim.Adam(model.parameters()), **kw)
