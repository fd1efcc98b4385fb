"""The seam between the library's host-side units: the environment engine (csrc/skyjo_capi.hip) and the packed nets + learner
(csrc/skyjo_learner.hip) share csrc/skyjo_host.h and nothing else - neither sources nor kernels - and fail through one error
message.  No compute call is made here: it runs without a GPU."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "skyjo_rl_amd", "csrc")
DEVICE_PARTS = {"skyjo_device.h", "skyjo_rng.h", "skyjo_transition.h", "skyjo_record.h", "skyjo_step.h", "skyjo_deal.h", "skyjo_cycle.h",
                "skyjo_callers.h"}
LEARNER_HEADERS = {"skyjo_targets.h", "skyjo_batches.h", "skyjo_loss.h", "skyjo_update.h", "skyjo_train.h", "skyjo_arena.h", "skyjo_learner_util.h"}
LEARNER_KERNELS = ("k_rollout_targets", "k_select_pass", "k_select_scan", "k_gather_rows", "k_gather_logits", "k_ppo_loss", "k_ppo_loss_finish",
                   "k_mlp_update", "k_mlp_train_fwd", "k_mlp_train_bwd_rows", "k_mlp_train_bwd_weights", "k_mlp_train_bwd_finish", "k_arena",
                   "k_episode_stats", "k_episode_stats_finish")
ENV_KERNELS = ("k_cycle", "k_step", "k_deal", "k_reset", "k_observe")


@pytest.fixture(scope="module")
def built():
    """The library's path and, per unit, its object file (a tree whose library came without them is compiled once more)."""
    from skyjo_rl_amd import build

    out = build.build()
    objs = {name: os.path.join(build.OBJ_DIR, "libskyjo_vec.%s.o" % name) for name, _, _ in build.UNITS}
    if not all(os.path.exists(o) for o in objs.values()):
        out = build.build(force=True)
    return out, objs


def _includes(name, seen=None):
    """Every file under csrc/ that `name` includes with quotes, directly or through another."""
    seen = set() if seen is None else seen
    for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(os.path.join(CSRC, name)).read(), flags=re.M):
        base = os.path.basename(inc)
        if base not in seen and os.path.exists(os.path.join(CSRC, base)):
            seen.add(base)
            _includes(base, seen)
    return seen


def test_sources_do_not_cross_the_seam():
    learner, env = _includes("skyjo_learner.hip"), _includes("skyjo_capi.hip")
    assert "skyjo_host.h" in learner and "skyjo_host.h" in env
    assert LEARNER_HEADERS <= learner and DEVICE_PARTS <= env
    assert not learner & DEVICE_PARTS, sorted(learner & DEVICE_PARTS)
    assert not env & LEARNER_HEADERS, sorted(env & LEARNER_HEADERS)


def test_objects_hold_their_own_kernels_only(built):
    _, objs = built
    names = {unit: subprocess.check_output(["nm", obj], text=True) for unit, obj in objs.items()}
    for k in LEARNER_KERNELS:
        assert k in names["skyjo_learner"], k
        assert k not in names["skyjo_capi"], k
    for k in ENV_KERNELS:
        assert k in names["skyjo_capi"], k
        assert k not in names["skyjo_learner"], k


def test_one_error_message_for_both_units(built):
    from skyjo_rl_amd import _lib

    L = _lib.load()
    last = lambda: L.skyjo_vec_last_error().decode()
    p = 4096  # aligned and not null; nothing reads it: m is checked first

    def loss_with_no_rows():
        return L.skyjo_vec_ppo_loss(p, p, p, p, p, p, p, p, 0, 0.2, 0.5, 0.01, 0.0, p, p, p, p, 0, None)

    def create_with_wrong_abi():
        cfg = _lib.Config(abi_version=_lib.ABI_VERSION + 1, num_envs=64, num_players=3)
        return L.skyjo_vec_create(ctypes.byref(cfg), ctypes.byref(ctypes.c_void_p()))

    assert loss_with_no_rows() != 0 and last() == "skyjo_vec_ppo_loss: m must be at least 1"
    assert create_with_wrong_abi() != 0 and last() == "abi_version mismatch"
    assert loss_with_no_rows() != 0 and last() == "skyjo_vec_ppo_loss: m must be at least 1"
