"""Global-norm gradient clipping on the device in front of the native Adam (skyjo_vec_grad_norm, skyjo_vec_mlp_adam_step_clipped,
csrc/skyjo_clip.h and skyjo_update.h): the norm against the float64 restatement of tests/grad_clip_ref.py, the coefficient with torch's
bits, the clipped step byte for byte the EXISTING step on pre-scaled gradients, ``learner.NativeAdam(max_grad_norm=)`` over the twelve
tensors of both branches, and ``examples/ppo.py::ppo_update(grad_clip=)``."""
import copy
import ctypes as C
import math

import numpy as np
import pytest

from . import grad_clip_ref as ref
from . import mlp_pack_ref, mlp_train_ref, ppo_step_ref

pytestmark = pytest.mark.gpu

F32 = np.float32
INF = float("inf")
CASES = ref.cases()  # computed once, read only
SENTINEL = F32(-12345.678)


def _np(t):
    return t.detach().cpu().numpy()


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _segments(views, buf):
    n = len(views)
    ptrs = (C.c_void_p * n)(*[buf.data_ptr() + 4 * s for s, _ in views])
    return ptrs, (C.c_int64 * n)(*[c for _, c in views]), n


def _out2():
    """Two floats between sentinels: (the whole buffer, the address of element 2)."""
    import torch

    guard = torch.full((6,), float(SENTINEL), dtype=torch.float32, device="cuda")
    return guard, guard.data_ptr() + 8


def _guarded(guard):
    g = _np(guard)
    assert (g[[0, 1, 4, 5]] == SENTINEL).all(), g
    return g[2], g[3]


def _same_class(got, want32):
    """A float32 norm against the restatement rounded to float32: within 1 ulp, or the same NaN / inf / zero."""
    if np.isnan(want32):
        return bool(np.isnan(got))
    if np.isinf(want32) or want32 == 0.0:
        return bool(got == want32)
    return bool(np.isfinite(got)) and ref.ulps(got, want32) <= 1


def _same_coef(got, want):
    return (np.isnan(got) and np.isnan(want)) or ref.bits(got) == ref.bits(want)


# ---- 1. the norm and the coefficient on synthetic segment lists ----
@pytest.mark.parametrize("name", sorted(CASES))
def test_norm_and_coefficient(name):
    import torch

    from skyjo_rl_amd import _lib

    L = _lib.load()
    case = CASES[name]
    buf = torch.from_numpy(case["flat"]).cuda()
    assert buf.data_ptr() % 16 == 0
    ptrs, counts, n = _segments(case["views"], buf)
    mx = case["max_norm"]
    want = ref.norm([case["flat"][s:s + c] for s, c in case["views"]])
    with np.errstate(all="ignore"):
        want32 = F32(want)
    pairs = []
    for _ in range(2):
        guard, out = _out2()
        _lib.check(L.skyjo_vec_grad_norm(ptrs, counts, n, mx, out, _stream()))
        pairs.append(_guarded(guard))  # the sentinels around out2 are as they were
    (norm, coef), again = pairs
    print("GRAD_NORM %s: device %r float64 %r coefficient %r" % (name, norm, want, coef))
    assert _same_class(norm, want32), (norm, want)
    assert _same_coef(coef, ref.coef32(norm, mx)), (coef, ref.coef32(norm, mx))  # for the DEVICE's own norm
    assert F32(norm).tobytes() == F32(again[0]).tobytes() and F32(coef).tobytes() == F32(again[1]).tobytes()
    assert _np(buf).tobytes() == case["flat"].tobytes()  # read only
    if name == "e_zeros":
        assert norm == 0.0 and coef == 1.0
    if name == "g_nan":
        assert np.isnan(norm) and np.isnan(coef)
    if name == "h_inf":
        assert np.isposinf(norm) and coef == 0.0
    if name == "i_measure_only":
        assert coef == 1.0 and norm > 1.0
    if name == "a_pair_17":
        assert coef < 1.0
        # the straddle: max_norm at norm + 1e-6 and its float32 neighbours
        at = F32(F32(norm) + F32(1e-6))
        coefs = []
        for m in (np.nextafter(at, F32(0)), at, np.nextafter(at, F32(np.inf))):
            guard, out = _out2()
            _lib.check(L.skyjo_vec_grad_norm(ptrs, counts, n, float(m), out, _stream()))
            n2, c2 = _guarded(guard)
            assert F32(n2).tobytes() == F32(norm).tobytes()
            assert _same_coef(c2, ref.coef32(norm, m)), (m, c2)
            coefs.append(c2)
        assert any(c == 1.0 for c in coefs) and any(c < 1.0 for c in coefs), coefs


def test_python_grad_norm():
    import torch

    from skyjo_rl_amd import learner

    case = CASES["d_32_segments"]
    buf = torch.from_numpy(case["flat"]).cuda()
    tensors = [buf[s:s + c] for s, c in case["views"]]
    want32 = F32(ref.norm([case["flat"][s:s + c] for s, c in case["views"]]))
    got = learner.grad_norm(tensors, max_norm=case["max_norm"])
    assert got.dtype == torch.float32 and tuple(got.shape) == (2,) and got.is_cuda
    norm, coef = _np(got)
    assert _same_class(norm, want32) and _same_coef(coef, ref.coef32(norm, case["max_norm"])) and coef < 1.0
    out = torch.zeros((2,), dtype=torch.float32, device="cuda")
    assert learner.grad_norm(tensors, out=out) is out  # None: measure only
    assert _np(out)[0].tobytes() == norm.tobytes() and _np(out)[1] == 1.0
    shaped = learner.grad_norm([tensors[5].view(3, 100), tensors[6]], 1.0)  # any shapes
    assert _same_class(_np(shaped)[0], F32(ref.norm([case["flat"][s:s + c] for s, c in case["views"][5:7]])))
    for bad in (dict(tensors=[]), dict(tensors=tensors + [tensors[0]]), dict(tensors=[buf.cpu()]), dict(tensors=[buf.double()]),
                dict(tensors=[buf[::2]]), dict(tensors=tensors, max_norm=0.0), dict(tensors=tensors, max_norm=-1.0),
                dict(tensors=tensors, max_norm=float("nan")), dict(tensors=tensors, out=torch.zeros(3, device="cuda")),
                dict(tensors=tensors, out=torch.zeros(2))):
        with pytest.raises(ValueError):
            learner.grad_norm(**bad)


# ---- 2. the clipped step is the old step on pre-scaled gradients, byte for byte ----
class _Net:
    """One branch on the GPU with its FusedNet and a zeroed Adam state, stepped through the C ABI."""

    def __init__(self, weights, precision):
        import torch

        from skyjo_rl_amd import _lib
        from skyjo_rl_amd.action_mask_model import ActionMaskModel, FusedNet

        self.L = _lib.load()
        obs_dim, out_dim = weights[0].shape[1], weights[4].shape[0]
        self.seq = ActionMaskModel(obs_dim=obs_dim, num_outputs=out_dim).policy
        with torch.no_grad():
            for p, w in zip(self.seq.parameters(), weights):
                p.copy_(torch.from_numpy(np.array(w)))
        self.seq = self.seq.cuda()
        self.params = list(self.seq.parameters())
        self.net = FusedNet(self.seq, precision=precision)
        self.n = int(self.L.skyjo_vec_mlp_adam_state_bytes(self.net._h)) // 4
        self.state = torch.zeros((self.n,), dtype=torch.float32, device="cuda")
        self.pp = (C.c_void_p * 6)(*[p.data_ptr() for p in self.params])

    def set_state(self, m, v):
        import torch

        total = sum(a.size for a in m)
        flat = lambda arrays: np.concatenate([np.asarray(a, dtype=F32).reshape(-1) for a in arrays] + [np.zeros(self.n // 2 - total, dtype=F32)])
        self.state.copy_(torch.from_numpy(np.concatenate([flat(m), flat(v)])))

    def step(self, grads, t, hp=mlp_pack_ref.ADAM_HYPER, coef_ptr=None, **change):
        gg = (C.c_void_p * 6)(*[g.data_ptr() for g in grads])
        a = dict(m=self.net._h, state=self.state.data_ptr(), state_bytes=self.n * 4, lr=hp["lr"], beta1=hp["betas"][0], beta2=hp["betas"][1],
                 eps=hp["eps"], step=t)
        a.update(change)
        args = (a["m"], self.pp, gg, a["state"], a["state_bytes"], a["lr"], a["beta1"], a["beta2"], a["eps"], a["step"])
        if coef_ptr is None:
            return self.L.skyjo_vec_mlp_adam_step(*args, _stream())
        return self.L.skyjo_vec_mlp_adam_step_clipped(*args, coef_ptr, _stream())

    def everything(self):
        """The parameters, the state (exp_avg and exp_avg_sq) and the exported blob, as bytes."""
        return [_np(p).tobytes() for p in self.params] + [_np(self.state).tobytes(), _np(self.net.export()).tobytes()]

    def close(self):
        self.net.close()


@pytest.mark.parametrize("precision,obs_dim,out_dim", [(p, o, d) for p in ("fp32", "bf16") for (o, d) in mlp_pack_ref.SHAPES])
def test_clipped_step_is_the_old_step_on_scaled_gradients(precision, obs_dim, out_dim):
    import torch

    from skyjo_rl_amd import _lib

    weights = [np.array(w) for w in mlp_train_ref.weights((obs_dim, out_dim), "A")]
    shapes = [w.shape for w in weights]
    for clip in (True, False):  # max_norm half the norm; max_norm +inf against the raw gradients
        A, B = _Net(weights, precision), _Net(weights, precision)
        assert A.everything() == B.everything()
        out2 = torch.zeros((2,), dtype=torch.float32, device="cuda")
        for t in range(1, mlp_pack_ref.ADAM_STEPS + 1):
            host = mlp_pack_ref.adam_grads(shapes, t)
            grads = [torch.from_numpy(g).cuda() for g in host]
            ptrs = (C.c_void_p * 6)(*[g.data_ptr() for g in grads])
            counts = (C.c_int64 * 6)(*[g.numel() for g in grads])
            mx = 0.5 * ref.norm(host) if clip else INF
            _lib.check(A.L.skyjo_vec_grad_norm(ptrs, counts, 6, mx, out2.data_ptr(), _stream()))
            _lib.check(A.step(grads, t, coef_ptr=out2.data_ptr() + 4))
            coef = out2[1]
            assert (float(coef) < 1.0) == clip and (clip or float(coef) == 1.0)
            scaled = [g * coef for g in grads] if clip else grads  # torch's float32 multiply on the device
            _lib.check(B.step(scaled, t))  # the EXISTING entry point
            assert A.everything() == B.everything(), (clip, t)
            assert all(_np(g).tobytes() == h.tobytes() for g, h in zip(grads, host)), (clip, t)  # the gradients are not rewritten
        A.close(), B.close()


# ---- 3. NativeAdam(max_grad_norm=) ----
def _model_and_optimizer(seed, **kw):
    import torch

    from skyjo_rl_amd.action_mask_model import ActionMaskModel, FusedNet
    from skyjo_rl_amd.learner import NativeAdam

    torch.manual_seed(seed)
    model = ActionMaskModel(obs_dim=31).cuda()
    nets = FusedNet(model.policy), FusedNet(model.value)
    return model, nets, NativeAdam(model, nets[0], nets[1], **mlp_pack_ref.ADAM_HYPER, **kw)


def _twelve(model):
    return list(model.policy.parameters()) + list(model.value.parameters())


def _everything(model, nets, opt):
    return ([_np(p).tobytes() for p in _twelve(model)] + [_np(n.export()).tobytes() for n in nets] +
            [_np(opt.state[p][k]).tobytes() for p in _twelve(model) for k in ("exp_avg", "exp_avg_sq")])


def test_native_adam_clips_by_the_norm_of_both_branches():
    import torch

    from skyjo_rl_amd import _lib

    MAX = 1.0
    host = ref.pair_grads(31)
    # each branch's own norm 0.8 < MAX, the norm of the twelve sqrt(1.28) > MAX: a norm per branch would clip nothing
    host = [(g.astype(np.float64) * (0.8 / ref.norm(host[6 * (i // 6):6 * (i // 6) + 6]))).astype(F32) for i, g in enumerate(host)]
    assert ref.norm(host[:6]) < 0.9 * MAX and ref.norm(host[6:]) < 0.9 * MAX and ref.norm(host) > 1.1 * MAX
    model_a, nets_a, opt_a = _model_and_optimizer(3, max_grad_norm=MAX)
    model_b, nets_b, opt_b = _model_and_optimizer(3)
    assert opt_b.grad_stats is None and opt_a.grad_stats.dtype == torch.float32 and tuple(opt_a.grad_stats.shape) == (2,)
    stats_at = opt_a.grad_stats.data_ptr()
    assert _everything(model_a, nets_a, opt_a) == _everything(model_b, nets_b, opt_b)
    for p, g in zip(_twelve(model_a), host):
        p.grad = torch.from_numpy(g).cuda()
    opt_a.step()
    norm, coef = _np(opt_a.grad_stats)
    assert opt_a.grad_stats.data_ptr() == stats_at and opt_a.steps == 1
    assert _same_class(norm, F32(ref.norm(host))), (norm, ref.norm(host))
    assert _same_coef(coef, ref.coef32(norm, MAX)) and coef < 1.0
    assert all(_np(p.grad).tobytes() == g.tobytes() for p, g in zip(_twelve(model_a), host))  # .grad is not rewritten
    # a second optimizer through the old entry on pre-scaled gradients
    for p, q in zip(_twelve(model_b), _twelve(model_a)):
        p.grad = q.grad * opt_a.grad_stats[1]
    opt_b.step()
    assert opt_b.grad_stats is None
    assert _everything(model_a, nets_a, opt_a) == _everything(model_b, nets_b, opt_b)
    # max_grad_norm is a plain attribute, checked before the first launch: both branches step, or neither
    before = _everything(model_a, nets_a, opt_a)
    for bad in (0.0, -1.0, float("nan"), 1e-60, "1"):
        opt_a.max_grad_norm = bad
        with pytest.raises(ValueError):
            opt_a.step()
    assert opt_a.steps == 1 and _everything(model_a, nets_a, opt_a) == before
    opt_a.max_grad_norm = INF  # measure only
    opt_a.step()
    assert float(opt_a.grad_stats[1]) == 1.0 and _np(opt_a.grad_stats)[0].tobytes() == norm.tobytes()
    for n in nets_a + nets_b:
        n.close()
    # max_grad_norm=None is the parent's step: the existing entry point through the ABI
    model_c, nets_c, opt_c = _model_and_optimizer(4)
    model_d, nets_d, opt_d = _model_and_optimizer(4)
    L = _lib.load()
    for m in (model_c, model_d):
        for p, g in zip(_twelve(m), host):
            p.grad = torch.from_numpy(g).cuda()
    opt_c.step()
    for (net, params, buf, pp) in opt_d._branches:
        gg = (C.c_void_p * 6)(*[p.grad.data_ptr() for p in params])
        hp = mlp_pack_ref.ADAM_HYPER
        _lib.check(L.skyjo_vec_mlp_adam_step(net._h, pp, gg, buf.data_ptr(), buf.numel() * 4, hp["lr"], hp["betas"][0], hp["betas"][1], hp["eps"], 1,
                                             _stream()))
    assert opt_c.grad_stats is None
    assert _everything(model_c, nets_c, opt_c) == _everything(model_d, nets_d, opt_d)
    for n in nets_c + nets_d:
        n.close()


# ---- 4. against torch, with the project's yardstick ----
def test_clipped_step_against_float64_and_torch():
    """One teacher-forced step from ``ppo_step_ref.adam_inputs`` with max_norm half the gradients' norm: d_ours <= MARGIN d_torch per
    tensor on p, exp_avg and exp_avg_sq, d the ``ppo_step_ref.deviation`` from the float64 step (the restatement's coefficient, then
    ``ppo_step_ref.adam`` on the scaled gradients), torch's: ``clip_grad_norm_`` and ``ppo_step_ref.torch_adam`` in float32 on the CPU.
    Where torch's is 0 (the tensor whose gradient and state are zero) ours is 0 - tests/test_gpu_ppo_step.py's rule."""
    import torch

    from skyjo_rl_amd import _lib

    hp, t = ppo_step_ref.ADAM_FAR_HYPER, 7
    p0, g0, m0, v0 = ppo_step_ref.adam_inputs()
    norm64 = ref.norm(g0)
    mx = 0.5 * norm64
    want = ppo_step_ref.adam(p0, [g.astype(np.float64) * ref.coef64(norm64, mx) for g in g0], m0, v0, hp, t)
    leaves = [torch.zeros(g.shape, dtype=torch.float32, requires_grad=True) for g in g0]
    for leaf, g in zip(leaves, g0):
        leaf.grad = torch.from_numpy(g.copy())
    torch.nn.utils.clip_grad_norm_(leaves, mx)
    yard = ppo_step_ref.torch_adam(p0, [leaf.grad.numpy() for leaf in leaves], m0, v0, hp, t)
    A = _Net(p0, "fp32")
    A.set_state(m0, v0)
    grads = [torch.from_numpy(g).cuda() for g in g0]
    out2 = torch.zeros((2,), dtype=torch.float32, device="cuda")
    ptrs, counts = (C.c_void_p * 6)(*[g.data_ptr() for g in grads]), (C.c_int64 * 6)(*[g.numel() for g in grads])
    _lib.check(A.L.skyjo_vec_grad_norm(ptrs, counts, 6, mx, out2.data_ptr(), _stream()))
    _lib.check(A.step(grads, t, hp=hp, coef_ptr=out2.data_ptr() + 4))
    assert _same_class(_np(out2)[0], F32(norm64)) and float(out2[1]) < 1.0
    host = _np(A.state)
    got, at = {"p": [_np(p) for p in A.params], "exp_avg": [], "exp_avg_sq": []}, 0
    for w in p0:
        got["exp_avg"].append(host[at:at + w.size].reshape(w.shape)), got["exp_avg_sq"].append(host[A.n // 2 + at:A.n // 2 + at + w.size].reshape(w.shape))
        at += w.size
    assert ppo_step_ref.same_bits(_np(A.net.export()), mlp_pack_ref.pack(*got["p"], precision="fp32"))
    bad = []
    for what, w3, y3 in zip(ppo_step_ref.ADAM_OUTPUTS, want, yard):
        for k, a, w, y in zip(ppo_step_ref.PARAMS, got[what], w3, y3):
            d_ours, d_torch = ppo_step_ref.deviation(a.astype(np.float64), w), ppo_step_ref.deviation(y, w)
            print("GRAD_CLIP_ADAM %s %s: d_ours %.3e d_torch %.3e ratio %s" % (what, k, d_ours, d_torch, "%.3f" % (d_ours / d_torch) if d_torch else "-"))
            if not d_ours <= ppo_step_ref.MARGIN * d_torch:
                bad.append((what, k, d_ours, d_torch))
    assert bad == []
    A.close()


# ---- 5. validation ----
def test_validation_launches_nothing():
    import torch

    from skyjo_rl_amd import _lib

    L = _lib.load()
    last = lambda: L.skyjo_vec_last_error().decode()
    buf = torch.ones((64,), dtype=torch.float32, device="cuda")
    base = buf.data_ptr()
    guard, out = _out2()

    def norm(ptrs=(base, base + 64), counts=(8, 8), n=2, max_norm=1.0, out2=out, null=None):
        pp = None if null == "tensors" else (C.c_void_p * len(ptrs))(*ptrs)
        cc = None if null == "counts" else (C.c_int64 * len(counts))(*counts)
        return L.skyjo_vec_grad_norm(pp, cc, n, max_norm, None if null == "out2" else out2, _stream())

    assert norm() == 0
    torch.cuda.synchronize()
    assert _guarded(guard)[0] == 4.0
    guard.fill_(float(SENTINEL))
    many = (base,) * 33
    for bad in (dict(null="tensors"), dict(null="counts"), dict(null="out2"), dict(n=0), dict(n=-1), dict(ptrs=many, counts=(1,) * 33, n=33),
                dict(counts=(8, -1)), dict(ptrs=(base, None), counts=(8, 1)), dict(ptrs=(base, base + 2)), dict(ptrs=(base + 1, base)),
                dict(max_norm=float("nan")), dict(max_norm=0.0), dict(max_norm=-1.0), dict(max_norm=-INF), dict(out2=out + 2)):
        assert norm(**bad) != 0, bad
        assert last().startswith("skyjo_vec_grad_norm: "), (bad, last())
    assert norm(ptrs=(base, None), counts=(8, 0)) == 0  # a null pointer with nothing to read is no error
    torch.cuda.synchronize()
    assert _guarded(guard)[0] == F32(math.sqrt(8.0))
    guard.fill_(float(SENTINEL))
    for bad in (dict(n=0), dict(max_norm=0.0)):
        assert norm(**bad) != 0
    torch.cuda.synchronize()
    assert (_np(guard) == SENTINEL).all()  # out2 untouched

    weights = [np.array(w) for w in mlp_train_ref.weights((17, 26), "A")]
    A = _Net(weights, "fp32")
    before = A.everything()
    grads = [torch.ones_like(p) for p in A.params]
    coef = torch.ones((2,), dtype=torch.float32, device="cuda")
    ok = coef.data_ptr()
    misaligned = torch.ones((256 * 256 + 1,), dtype=torch.float32, device="cuda")[1:]  # w2's size, 4 bytes behind a 16-byte boundary
    for bad in (dict(coef_ptr=0), dict(coef_ptr=ok + 2), dict(coef_ptr=ok + 1), dict(m=None), dict(state=None), dict(state_bytes=A.n * 4 - 4), dict(step=0),
                dict(lr=INF), dict(lr=float("nan")), dict(beta1=1.0), dict(beta2=-1e-3), dict(eps=-1.0), dict(state=A.state.data_ptr() + 4)):
        a = dict(dict(coef_ptr=ok), **bad)
        if a["coef_ptr"] == 0:  # (ctypes: a null pointer argument)
            a["coef_ptr"] = C.c_void_p(None)
        assert A.step(grads, 1, **a) != 0, bad
        assert last().startswith("skyjo_vec_mlp_adam_step_clipped: "), (bad, last())
    assert A.step(grads[:2] + [misaligned] + grads[3:], 1, coef_ptr=ok) != 0
    assert last().startswith("skyjo_vec_mlp_adam_step_clipped: ")
    torch.cuda.synchronize()
    assert A.everything() == before
    assert A.step(grads, 0) != 0 and last().startswith("skyjo_vec_mlp_adam_step: ")  # the old entry keeps its name
    A.close()


# ---- 6. ppo_update(grad_clip=) ----
@pytest.fixture(scope="module")
def rollout():
    """A small rollout and the model that played it: 256 games of 4 players, 48 iterations."""
    import torch

    from examples.ppo import repack
    from skyjo_rl_amd import SkyjoVecEnv
    from skyjo_rl_amd.action_mask_model import ActionMaskModel
    from skyjo_rl_amd.rollout import RolloutBuffer, collect

    torch.manual_seed(0)
    env = SkyjoVecEnv(256, num_players=4)
    env.seed(None, 9)
    env.reset()
    model = ActionMaskModel(obs_dim=env.obs_dim).cuda()
    pol, val = repack(model)
    buf = RolloutBuffer(env, 48)
    collect(env, pol, val, buf, seed=1, first_ticket=0)
    pol.close(), val.close()
    yield model, buf
    env.close()


def _update(rollout, native=True, **kw):
    """``ppo_update`` on a copy of the rollout's model from the same start: (result, the parameters' and both blobs' bytes)."""
    import torch

    from examples.ppo import ppo_update, repack
    from skyjo_rl_amd.learner import NativeAdam

    model0, buf = rollout
    model = copy.deepcopy(model0)
    pol, val = repack(model)
    if native:
        opt = NativeAdam(model, pol, val, lr=3e-4)
        out = ppo_update(model, buf, opt, epochs=2, minibatch=2048, gae=(0.99, 0.95), native_batches=True, native_loss=True, native_nets=True, **kw)
        assert opt.max_grad_norm is None and opt.grad_stats is None  # set for the call only
    else:
        out = ppo_update(model, buf, torch.optim.Adam(model.parameters(), lr=3e-4), epochs=2, minibatch=2048, gae=(0.99, 0.95), **kw)
    state = [_np(p).tobytes() for p in model.parameters()] + [_np(pol.export()).tobytes(), _np(val.export()).tobytes()]
    pol.close(), val.close()
    return out, state


def test_ppo_update_grad_clip(rollout):
    plain, state_plain = _update(rollout)
    assert plain["transitions"] > 2048  # (more than one step per epoch)
    keys = {"policy_loss", "vf_loss", "kl", "entropy", "clip_fraction"}
    assert set(plain) == {"first", "last", "transitions"} and set(plain["first"]) == keys and set(plain["last"]) == keys  # today's keys
    wide, state_wide = _update(rollout, grad_clip=1e30)
    assert state_wide == state_plain  # the coefficient is exactly 1: not a bit moves
    for ep in ("first", "last"):
        assert set(wide[ep]) == keys | {"grad_norm", "grad_clipped"}
        assert math.isfinite(wide[ep]["grad_norm"]) and wide[ep]["grad_norm"] > 0.0 and wide[ep]["grad_clipped"] == 0.0
        assert all(wide[ep][k] == plain[ep][k] for k in keys)
    tight, state_tight = _update(rollout, grad_clip=0.1 * wide["first"]["grad_norm"])
    assert tight["first"]["grad_clipped"] == 1.0 and state_tight != state_plain
    print("GRAD_CLIP_UPDATE grad_norm %r / %r, clipped run %r / %r" % (wide["first"]["grad_norm"], wide["last"]["grad_norm"],
                                                                      tight["first"]["grad_norm"], tight["last"]["grad_norm"]))


def test_ppo_update_grad_clip_with_a_torch_optimizer(rollout):
    out, _ = _update(rollout, native=False, grad_clip=0.5)
    for ep in ("first", "last"):
        assert set(out[ep]) == {"policy_loss", "vf_loss", "kl", "grad_norm", "grad_clipped"}
        assert math.isfinite(out[ep]["grad_norm"]) and out[ep]["grad_norm"] > 0.0 and 0.0 <= out[ep]["grad_clipped"] <= 1.0
    plain, _ = _update(rollout, native=False)
    assert set(plain["first"]) == {"policy_loss", "vf_loss", "kl"}


@pytest.mark.parametrize("bad", [0.0, -1.0, float("inf"), float("nan"), "1", True])
def test_ppo_update_rejects_a_bad_grad_clip(rollout, bad):
    from examples.ppo import ppo_update

    model, buf = rollout
    with pytest.raises(ValueError):  # (before anything is looked at: no optimizer is needed to get here)
        ppo_update(model, buf, None, grad_clip=bad)
