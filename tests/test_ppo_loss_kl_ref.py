"""The PPO loss head with the KL penalty (``skyjo_vec_ppo_loss_kl``, ``learner.ppo_loss_kl``) without a GPU: the float64
restatement of tests/ppo_loss_kl_ref.py - its hand-derived gradient included - against torch's autograd, the generator of
tests/ppo_loss_kl_synth.py (every listed situation is reached), the measurement the GPU test's tolerances come from, the adaptive
coefficient's rule, the ABI, and the argument checks that need no device."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from tests import ppo_loss_kl_ref as klref
from tests import ppo_loss_kl_synth as ks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("kl_coeff", ks.KL_COEFFS)
@pytest.mark.parametrize("ent_coef,vf_clip", ks.COEFFS)
def test_restatement_equals_autograd_in_float64(ent_coef, vf_clip, kl_coeff):
    """The bound of tests/test_ppo_loss_ref.py for the head without the penalty: statistics and both gradients to 1e-12 relative."""
    import torch

    for m in (1, 65, 1000):
        b = ks.make(m)
        want = ks.reference(b, ent_coef, vf_clip, kl_coeff)
        stats, gl, gv = ks.torch_head_on(b, torch.float64, ent_coef, vf_clip, kl_coeff)
        for name, s, w in zip(klref.STATS, stats, want["stats"]):
            assert abs(s - w) <= 1e-12 * max(abs(s), 1e-3), (m, name, s, w)
        for name, got, w in (("grad_logits", gl, want["grad_logits"]), ("grad_value", gv, want["grad_value"])):
            assert np.abs(got - w).max() <= 1e-12 * np.abs(got).max(), (m, name, np.abs(got - w).max())
        masked = b.log_mask != 0
        masked[np.arange(m), b.actions] = False
        assert (want["grad_logits"][masked] == 0.0).all() and (gl[masked] == 0.0).all()
        one = (b.log_mask == 0).sum(axis=1) == 1
        assert (want["akl"][one] == 0.0).all() and (want["kl_grad"][one] == 0.0).all()
        assert (want["akl"] >= -1e-12).all()                                    # a divergence
        if kl_coeff == 0.0:
            assert np.array_equal(want["grad_logits"], want["grad_logits_base"]) and np.array_equal(want["stats"][:6], ks.synth.reference(b, ent_coef, vf_clip)["stats"])


def test_generator_reaches_every_situation_and_leaves_the_base_batch_alone():
    for m in ks.ROW_COUNTS:
        b = ks.make(m)
        base = ks.synth.make(m)
        assert all(np.array_equal(x, y) for x, y in zip(b[:8], base[:8]))        # ppo_loss_synth.make(m), the same bits
        assert b.old_logits.shape == (m, ks.K) and b.old_logits.dtype == np.float32 and np.isfinite(b.old_logits).all()
        if m >= 63:                                                               # where ppo_loss_synth promises its own branches
            missing = [k for k, v in ks.branches(b).items() if not v]
            assert not missing, (m, missing)
        assert np.array_equal(ks.make(m).old_logits, b.old_logits)


def test_float32_deviation_is_what_the_gpu_test_allows_for():
    """The tolerance measurement: ``torch_head_kl`` in float32 on the CPU against the restatement, on the GPU test's inputs.  The
    constants in tests/test_gpu_ppo_loss_kl.py (the kernel gets 4 times them) must not be below what is measured now."""
    from tests import test_gpu_ppo_loss_kl as gpu

    dev = ks.float32_deviation()
    print({k: "%.3e" % v for k, v in dev.items()})
    assert set(gpu.F32_DEVIATION) == set(ks.TOL_KEYS)
    for k, v in dev.items():
        assert gpu.F32_DEVIATION[k] >= v, (k, gpu.F32_DEVIATION[k], v)
    assert gpu.MARGIN == 4.0 and gpu.ROWS_PER_WORKGROUP - 1 in ks.ROW_COUNTS and gpu.ROWS_PER_WORKGROUP + 1 in ks.ROW_COUNTS


def test_kl_coeff_rule():
    """Times 1.5 above 2 x target, times 0.5 below 0.5 x target, unchanged in between and ON both edges (strict inequalities)."""
    from skyjo_rl_amd.learner import KLCoeff

    k = KLCoeff()
    assert float(k) == 0.2 and k.target == 0.01
    assert k.update(0.0201) == 0.2 * 1.5 == float(k)          # above
    assert k.update(0.01) == 0.2 * 1.5                         # inside
    assert k.update(0.0049) == 0.2 * 1.5 * 0.5                 # below
    k = KLCoeff(0.5, 0.04)
    assert k.update(0.08) == 0.5 and k.update(0.02) == 0.5     # exactly on the edges
    assert k.update(np.nextafter(0.08, 1.0)) == 0.75 and k.update(np.nextafter(0.02, 0.0)) == 0.375
    assert KLCoeff(0.0).update(1.0) == 0.0
    for bad in ((-0.1, 0.01), (float("nan"), 0.01), (float("inf"), 0.01), (0.2, 0.0), (0.2, -1.0), (0.2, float("nan"))):
        with pytest.raises(ValueError):
            KLCoeff(*bad)


def test_abi_has_the_kl_head_and_the_logits_gather():
    from skyjo_rl_amd import _lib, build

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "skyjo_vec.h")).read(), flags=re.S)
    decl = {}
    for name in ("skyjo_vec_ppo_loss_kl_scratch_bytes", "skyjo_vec_ppo_loss_kl", "skyjo_vec_rollout_gather_logits"):
        mt = re.search(r"\b(int64_t|int)\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert mt, name
        decl[name] = (mt.group(1), [a.strip() for a in mt.group(2).split(",")])
    assert decl["skyjo_vec_ppo_loss_kl_scratch_bytes"] == ("int64_t", ["int64_t m"])
    kind, args = decl["skyjo_vec_ppo_loss_kl"]
    assert kind == "int" and len(args) == 21 and args[2] == "const float *old_logits" and args[9] == "int64_t m" and args[14] == "float kl_coeff"
    assert not any("skyjo_vec *" in a for a in args)
    kind, args = decl["skyjo_vec_rollout_gather_logits"]
    assert kind == "int" and len(args) == 6 and not any("skyjo_vec *" in a for a in args)                 # no engine handle
    res, sig = _lib.SIGNATURES["skyjo_vec_ppo_loss_kl"]
    assert res is ctypes.c_int and len(sig) == 21 and sig[9] is ctypes.c_int64 and sig[10:15] == [ctypes.c_float] * 5 and sig[19] is ctypes.c_int64
    res, sig = _lib.SIGNATURES["skyjo_vec_rollout_gather_logits"]
    assert res is ctypes.c_int and sig == [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
    lib = ctypes.CDLL(build.build())
    fn = lib.skyjo_vec_ppo_loss_kl_scratch_bytes
    fn.restype, fn.argtypes = ctypes.c_int64, [ctypes.c_int64]
    assert fn(0) == 0 and fn(1) == 56 and fn(128) == 56 and fn(129) == 112          # host arithmetic only: no device is touched
    old = lib.skyjo_vec_ppo_loss_scratch_bytes
    old.restype, old.argtypes = ctypes.c_int64, [ctypes.c_int64]
    assert old(129) == 96


def test_python_surface_and_checks_that_need_no_gpu():
    import torch

    import skyjo_rl_amd.learner as learner
    import skyjo_rl_amd.rollout as rollout
    from examples import ppo

    assert learner.STATS_KL == learner.STATS + ("action_kl",) == klref.STATS
    assert issubclass(learner.PPOLossKL, torch.autograd.Function) and issubclass(learner.PPOLossKLBuffers, learner.PPOLossBuffers)
    sig = inspect.signature(learner.ppo_loss_kl)
    assert list(sig.parameters) == ["logits", "value", "mb", "old_logits", "kl_coeff", "clip", "vf_coef", "ent_coef", "vf_clip", "out"]
    assert [sig.parameters[k].default for k in ("kl_coeff", "clip", "vf_coef", "ent_coef", "vf_clip", "out")] == [0.2, 0.3, 1.0, 0.0, None, None]
    assert list(inspect.signature(learner.PPOLossBuffers.__init__).parameters) == ["self", "rows", "device"]
    assert rollout.Minibatch._fields == ("observations", "log_mask", "actions", "logp", "advantages", "value_targets", "values", "seats")
    p = inspect.signature(rollout.minibatches).parameters
    assert p["behaviour"].default is False and list(p)[-1] == "behaviour"
    p = inspect.signature(ppo.ppo_update).parameters
    assert p["kl"].default is None and p["behaviour_net"].default is None
    p = inspect.signature(ppo.ppo_update_per_seat).parameters
    assert p["kls"].default is None and p["behaviour_nets"].default is None

    # CPU tensors and wrong shapes: ValueError before anything is loaded or launched
    b = ks.make(64)
    t = torch.from_numpy
    mb = rollout.Minibatch(None, t(b.log_mask), t(b.actions), t(b.logp), t(b.advantages), t(b.value_targets), t(b.values), None)
    with pytest.raises(ValueError, match="GPU"):
        learner.ppo_loss_kl(t(b.logits), t(b.value), mb, t(b.old_logits))
    with pytest.raises(ValueError):
        learner.ppo_loss_kl(t(b.logits)[:, :25], t(b.value), mb, t(b.old_logits))
    with pytest.raises(ValueError):
        learner.ppo_loss_kl(None, t(b.value), mb, t(b.old_logits))

    class Buf:                                                                     # what gather_behaviour looks at before any native call
        T, B = 2, 32
        actions = torch.zeros((2, 32), dtype=torch.int32)

    idx = torch.arange(4)
    with pytest.raises(ValueError, match="behaviour_logits"):
        rollout.gather_behaviour(Buf(), idx)
    with pytest.raises(ValueError, match="behaviour_logits"):
        next(rollout.minibatches(Buf(), 8, behaviour=True))
    buf = Buf()
    buf.behaviour = torch.zeros((2, 32, 25))
    with pytest.raises(ValueError, match="buf.behaviour"):
        rollout.gather_behaviour(buf, idx)
    buf.behaviour = torch.zeros((2, 32, 26))
    for bad in (idx.int(), idx.view(2, 2), [0, 1]):
        with pytest.raises(ValueError, match="index"):
            rollout.gather_behaviour(buf, bad)
    with pytest.raises(ValueError, match="out"):
        rollout.gather_behaviour(buf, idx, out=torch.zeros((3, 26)))
    with pytest.raises(ValueError, match="out"):
        rollout.gather_behaviour(buf, idx, out=torch.zeros((4, 26), dtype=torch.float64))

    # ppo_update: kl needs the native loss head and the net that played
    for kw in (dict(kl=0.2), dict(kl=0.2, native_batches=True, gae=(0.99, 1.0)), dict(kl=0.2, native_batches=True, native_loss=True, gae=(0.99, 1.0)),
               dict(kl="0.2", native_batches=True, native_loss=True, gae=(0.99, 1.0)), dict(kl=True, native_batches=True, native_loss=True, gae=(0.99, 1.0)),
               dict(kl=learner.KLCoeff(), native_batches=True, native_loss=True, gae=(0.99, 1.0), behaviour_net=object()),
               dict(behaviour_net=object(), native_batches=True, native_loss=True, gae=(0.99, 1.0))):
        with pytest.raises(ValueError):
            ppo.ppo_update(None, None, None, **kw)


def test_ppo_update_validation_matrix():
    """Which combinations of ``ppo_update``'s switches are rejected (``ValueError``) and which get as far as the first use of the
    ``None`` buffer (anything else): the whole product, 768 combinations, against the rule stated here.  Without ``kl``: no
    ``behaviour_net``, ``seats`` => ``native_batches``, ``native_nets`` => ``native_loss`` => ``native_batches`` => ``gae``, and an
    ``ent_coef`` or a ``vf_clip`` => ``native_loss``: 20.  With ``kl`` (a float or a ``KLCoeff``): ``native_batches``, ``native_loss``,
    ``gae`` and a ``FusedNet`` as ``behaviour_net``, everything else free: 32."""
    import itertools

    from examples import ppo
    from skyjo_rl_amd.action_mask_model import FusedNet
    from skyjo_rl_amd.learner import KLCoeff

    def accepted(gae, batches, loss, nets, ent_coef, vf_clip, seats, kl, net):
        if kl is not None:
            return batches and loss and gae is not None and net is not None
        return (net is None and (seats is None or batches) and (not nets or loss) and (not loss or batches)
                and (not batches or gae is not None) and (loss or (ent_coef == 0.0 and vf_clip is None)))

    net = object.__new__(FusedNet)  # (no handle, no library: only its type is looked at before the buffer is)
    product = list(itertools.product((None, (0.99, 1.0)), (False, True), (False, True), (False, True), (0.0, 0.01), (None, 1.0), (None, (0,)),
                                     (None, 0.2, KLCoeff()), (None, net)))
    assert len(product) == 768
    count = {False: 0, True: 0}
    for combo in product:
        gae, batches, loss, nets, ent_coef, vf_clip, seats, kl, bnet = combo
        try:
            ppo.ppo_update(None, None, None, gae=gae, native_batches=batches, native_loss=loss, native_nets=nets, ent_coef=ent_coef,
                           vf_clip=vf_clip, seats=seats, kl=kl, behaviour_net=bnet)
            got = None
        except ValueError:
            got = False
        except Exception:
            got = True
        assert got is bool(accepted(*combo)), (combo, got)
        count[kl is not None] += got
    assert count == {False: 20, True: 32}
