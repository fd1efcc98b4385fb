"""``learner.ppo_loss`` / ``PPOLoss`` (``skyjo_vec_ppo_loss``: the PPO loss head in one kernel) on the GPU against the float64
restatement of tests/ppo_loss_ref.py on the rows of tests/ppo_loss_synth.py: gradients and statistics within the recorded float32
deviation, the exact zeros and counts the definition promises, untouched guard tails, bit-identical repeats, a non-default stream,
argument validation, the autograd wrapper and ``examples.ppo.ppo_update(native_loss=True)`` end to end."""
import ctypes

import numpy as np
import pytest

from tests import ppo_loss_synth as synth

pytestmark = pytest.mark.gpu

ROWS_PER_WORKGROUP = 128   # SK_LOSS_ROWS of csrc/skyjo_loss.h: synth.ROW_COUNTS holds it and its two neighbours
# The largest absolute deviation, per output, of the SAME expression evaluated by torch in float32 on the CPU from the float64
# restatement, over every (row count, coefficients) case below (tests/ppo_loss_synth.py::float32_deviation; measured values rounded
# up to two digits; tests/test_ppo_loss_ref.py asserts that a fresh measurement does not exceed them).  The kernel is allowed 4 times
# these: room for another, equally valid float32 operation order and for device exp / log within a couple of ulp - anything beyond
# is a defect.  The gradients carry the factor 1 / m: both their plain bound and the bound on m * gradient hold.
F32_DEVIATION = {
    "grad_logits": 1.6e-07, "grad_logits_times_m": 2.2e-05, "grad_value": 1.3e-08, "grad_value_times_m": 1.3e-06,
    "loss": 4.8e-07, "policy_loss": 1.7e-07, "vf_loss": 3.6e-07, "entropy": 8.2e-08, "kl": 1.4e-07, "clip_fraction": 1.5e-08,
}
MARGIN = 4.0
SENTINEL = 0x7FC0DEAD      # a NaN with a payload: the guard tails' pattern, as float32 bits
GUARD = 64                 # elements before and after every output


def _mb(b, dev):
    import torch

    from skyjo_rl_amd.rollout import Minibatch

    t = lambda x: torch.from_numpy(x).to(dev)
    return (t(b.logits), t(b.value),
            Minibatch(None, t(b.log_mask), t(b.actions), t(b.logp), t(b.advantages), t(b.value_targets), t(b.values), None))


@pytest.fixture(scope="module")
def cases():
    """Every row count once: the batch on the device and, per coefficient pair, the restatement - shared and left unchanged."""
    import torch

    dev = torch.device("cuda", 0)
    out = {}
    for m in synth.ROW_COUNTS:
        b = synth.make(m)
        out[m] = (b, _mb(b, dev), {c: synth.reference(b, *c) for c in synth.COEFFS})
    return out


def _guarded(n, dtype, dev):
    """A tensor of n elements inside a larger one filled with the sentinel: (whole, view).  The view starts 16-byte aligned."""
    import torch

    pad = GUARD
    whole = torch.empty((pad + n + pad,), dtype=dtype, device=dev)
    whole.view(torch.int32).fill_(SENTINEL)
    return whole, whole[pad:pad + n]


def _call_guarded(logits, value, mb, ent_coef, vf_clip):
    """The C entry on guarded outputs: (stats, grad_logits, grad_value) as float64 numpy, after checking the tails."""
    import torch

    from skyjo_rl_amd import _lib

    L = _lib.load()
    dev, m = logits.device, logits.shape[0]
    nbytes = int(L.skyjo_vec_ppo_loss_scratch_bytes(m))
    bufs = [_guarded(m * 26, torch.float32, dev), _guarded(m, torch.float32, dev), _guarded(6, torch.float64, dev),
            _guarded(nbytes // 8, torch.float64, dev)]
    (wl, gl), (wv, gv), (ws, st), (wsc, sc) = bufs
    vp = lambda t: t.data_ptr()
    rc = L.skyjo_vec_ppo_loss(vp(logits), vp(mb.log_mask), vp(value), vp(mb.actions), vp(mb.logp), vp(mb.advantages), vp(mb.value_targets),
                              vp(mb.values), m, synth.CLIP, 1.0, ent_coef, 0.0 if vf_clip is None else vf_clip, vp(gl), vp(gv), vp(st),
                              vp(sc), nbytes, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.skyjo_vec_last_error()
    for whole, view in bufs:
        w = whole.view(torch.int32).cpu().numpy()
        inner = view.numel() * view.element_size() // 4
        pad = (w.size - inner) // 2
        assert (w[:pad] == SENTINEL).all() and (w[pad + inner:] == SENTINEL).all(), "an output's guard tail was written"
    raw = gl.view(torch.int32).cpu().numpy()
    assert not (raw == SENTINEL).any(), "grad_logits has elements the kernel did not write"
    assert not (gv.view(torch.int32).cpu().numpy() == SENTINEL).any()
    return st.cpu().numpy(), gl.view(m, 26).cpu().numpy().astype(np.float64), gv.cpu().numpy().astype(np.float64), gl.view(m, 26).cpu().numpy()


@pytest.mark.parametrize("ent_coef,vf_clip", synth.COEFFS)
@pytest.mark.parametrize("m", synth.ROW_COUNTS)
def test_kernel_against_restatement(cases, m, ent_coef, vf_clip):
    b, (logits, value, mb), wants = cases[m]
    want = wants[(ent_coef, vf_clip)]
    stats, gl, gv, gl32 = _call_guarded(logits, value, mb, ent_coef, vf_clip)
    dl, dv = np.abs(gl - want["grad_logits"]).max(), np.abs(gv - want["grad_value"]).max()
    ds = np.abs(stats - want["stats"])
    print(f"m={m} ent={ent_coef} vf_clip={vf_clip}: grad_logits {dl:.3e} (x m {dl * m:.3e}) grad_value {dv:.3e} (x m {dv * m:.3e}) stats",
          " ".join("%.3e" % x for x in ds))
    T = F32_DEVIATION
    assert dl <= MARGIN * min(T["grad_logits"], T["grad_logits_times_m"] / m)
    assert dv <= MARGIN * min(T["grad_value"], T["grad_value_times_m"] / m)
    for k, name in enumerate(synth.ref.STATS):
        assert ds[k] <= MARGIN * T[name], (name, ds[k])
    assert stats[5] * m == want["clipped_count"] and stats[5] == want["clipped_count"] / m
    masked = b.log_mask != 0
    masked[np.arange(m), b.actions] = False
    assert (gl32[masked] == 0.0).all()                                   # exactly 0.0 at every masked k != a
    if ent_coef == 0.0:
        assert (gl32[want["clipped"]] == 0.0).all()                      # a clipped row moves nothing
        big = np.abs(gl32).max(axis=1).astype(np.float64)
        assert (np.abs(gl32.astype(np.float64).sum(axis=1)) <= 26 * np.spacing(big.astype(np.float32)).astype(np.float64)).all()


def test_deterministic_and_out_reuse(cases):
    import torch

    from skyjo_rl_amd.learner import PPOLossBuffers, ppo_loss

    _, (logits, value, mb), _ = cases[4097]
    _, (l2, v2, mb2), _ = cases[257]
    a = ppo_loss(logits, value, mb, ent_coef=0.01, vf_clip=synth.VF_CLIP)
    first = [t.clone() for t in a]
    b = ppo_loss(logits, value, mb, ent_coef=0.01, vf_clip=synth.VF_CLIP)
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(first, b))
    out = PPOLossBuffers(4097, logits.device)
    ppo_loss(l2, v2, mb2, ent_coef=0.01, vf_clip=synth.VF_CLIP, out=out)
    c = ppo_loss(logits, value, mb, ent_coef=0.01, vf_clip=synth.VF_CLIP, out=out)
    assert c.grad_logits.data_ptr() == out.grad_logits.data_ptr() and c.stats.data_ptr() == out.stats.data_ptr()
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(first, c))
    # value as [m, 1]: the same bits, the gradient in that shape
    d = ppo_loss(logits, value.unsqueeze(1), mb, ent_coef=0.01, vf_clip=synth.VF_CLIP)
    assert d.grad_value.shape == (4097, 1) and torch.equal(d.grad_value.squeeze(1), first[2]) and torch.equal(d.stats, first[0])


def test_non_default_stream(cases):
    import torch

    from skyjo_rl_amd.learner import ppo_loss

    _, (logits, value, mb), _ = cases[1000]
    want = [t.clone() for t in ppo_loss(logits, value, mb, vf_clip=synth.VF_CLIP)]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        x = torch.zeros((1 << 20,), device=logits.device)
        for _ in range(8):
            x = x * 1.0001 + 1.0                       # work queued on the stream ahead of the call
        shifted = logits + x[:1]                       # ... which the call's input depends on (x[0] is finite: logits move by it)
        got = ppo_loss(shifted - x[:1], value, mb, vf_clip=synth.VF_CLIP)
        same_input = torch.equal(shifted - x[:1], logits)
    s.synchronize()
    if same_input:
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(want, got))
    with torch.cuda.stream(s):
        y = x.sum()                                    # queued work again, then the call on the unchanged input
        got = ppo_loss(logits, value, mb, vf_clip=synth.VF_CLIP)
    s.synchronize()
    assert bool(torch.isfinite(y)) and all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(want, got))


def test_validation_launches_nothing(cases):
    import torch

    from skyjo_rl_amd import _lib
    from skyjo_rl_amd.learner import PPOLossBuffers, ppo_loss

    L = _lib.load()
    _, (logits, value, mb), _ = cases[64]
    dev = logits.device
    out = PPOLossBuffers(64, dev)
    for t in (out.stats, out.grad_logits, out.grad_value):
        t.view(torch.int32).fill_(SENTINEL)
    bad = [
        (logits.double(), value, mb), (logits, value.double(), mb), (logits, value, mb._replace(actions=mb.actions.int())),     # dtype
        (logits, value, mb._replace(logp=mb.logp.double())),
        (logits.cpu(), value, mb), (logits, value.cpu(), mb), (logits, value, mb._replace(advantages=mb.advantages.cpu())),    # device
        (logits.t().contiguous().t(), value, mb), (logits, value.repeat(2)[::2], mb),                                           # contiguity
        (logits, value, mb._replace(log_mask=mb.log_mask.t().contiguous().t())),
        (logits[:, :25], value, mb), (logits, value[:63], mb), (logits, value, mb._replace(values=mb.values[:10])),             # shape
    ]
    for args in bad:
        with pytest.raises(ValueError):
            ppo_loss(*args, out=out)
    # a slice that starts at an odd row is not 16-byte aligned
    sub = lambda c, k: type(c)(*(None if x is None else x[k:] for x in c))
    with pytest.raises(ValueError):
        ppo_loss(logits[1:], value[1:], sub(mb, 1), out=out)
    with pytest.raises(ValueError):
        ppo_loss(logits, value, mb, clip=0.0, out=out)
    with pytest.raises(ValueError):
        ppo_loss(logits, value, mb, out=PPOLossBuffers(63, dev))
    # the C entry: SKYJO_E_INVALID (-1) with a message
    vp = lambda t: t.data_ptr()
    nbytes = int(L.skyjo_vec_ppo_loss_scratch_bytes(64))
    good = [vp(logits), vp(mb.log_mask), vp(value), vp(mb.actions), vp(mb.logp), vp(mb.advantages), vp(mb.value_targets), vp(mb.values), 64,
            0.3, 1.0, 0.0, 0.0, vp(out.grad_logits), vp(out.grad_value), vp(out.stats), vp(out.scratch), nbytes, None]
    ch = lambda k, v: good[:k] + [v] + good[k + 1:]
    cases_c = [ch(k, None) for k in (0, 1, 2, 3, 4, 5, 6, 7, 13, 14, 15, 16)]
    cases_c += [ch(8, 0), ch(8, -5), ch(9, 0.0), ch(9, -0.3), ch(9, float("inf")), ch(9, float("nan"))]
    cases_c += [ch(0, good[0] + 8), ch(1, good[1] + 4), ch(13, good[13] + 8), ch(17, nbytes - 1), ch(17, 0)]
    for args in cases_c:
        assert L.skyjo_vec_ppo_loss(*args) == -1, args
        assert b"skyjo_vec_ppo_loss" in L.skyjo_vec_last_error()
    torch.cuda.synchronize()
    for t in (out.stats, out.grad_logits, out.grad_value):
        assert bool((t.view(torch.int32) == SENTINEL).all()), "a refused call wrote an output"
    # the aligned slice two rows in is fine, and so is the whole call
    ppo_loss(logits[2:], value[2:], sub(mb, 2), out=out)
    assert L.skyjo_vec_ppo_loss(*good) == 0
    torch.cuda.synchronize()


def test_autograd_function(cases):
    import torch

    from skyjo_rl_amd.learner import PPOLoss, ppo_loss

    _, (logits, value, mb), _ = cases[257]
    want = [t.clone() for t in ppo_loss(logits, value, mb, ent_coef=0.01, vf_clip=synth.VF_CLIP)]
    for scale in (1.0, 0.5):
        lg, v = logits.clone().requires_grad_(), value.clone().requires_grad_()
        loss, stats = PPOLoss.apply(lg, v, mb, 0.3, 1.0, 0.01, synth.VF_CLIP)
        assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.requires_grad and not stats.requires_grad
        assert torch.equal(stats, want[0]) and float(loss) == float(want[0][0].float())
        (loss * scale).backward()
        assert torch.equal(lg.grad, want[1] * scale) and torch.equal(v.grad, want[2] * scale)    # a power of two: bitwise


def test_ppo_update_native_loss_end_to_end():
    import torch

    from examples.ppo import ppo_update, repack
    from skyjo_rl_amd import SkyjoVecEnv, _lib
    from skyjo_rl_amd.action_mask_model import ActionMaskModel
    from skyjo_rl_amd.learner import ppo_loss
    from skyjo_rl_amd.rollout import RolloutBuffer, collect, compute_targets, minibatches, select_rows

    torch.manual_seed(0)
    B, N, T = 256, 3, 64
    env = SkyjoVecEnv(B, num_players=N)
    env.seed(None, 9)
    env.reset()
    model = ActionMaskModel(obs_dim=env.obs_dim).cuda()
    pol, val = repack(model)
    buf = RolloutBuffer(env, T)
    collect(env, pol, val, buf, seed=1, first_ticket=0)

    # the first minibatch under the seed: parameter gradients through the kernel and through the torch expression, against the
    # float32-vs-float64 deviation of the torch expression's own parameter gradients (measured here, the model run once in float64)
    compute_targets(buf, gamma=0.99, lam=1.0)
    sel = select_rows(buf, _lib.TGT_HAS_TARGET)
    gen = torch.Generator(device="cuda").manual_seed(0)
    mb = next(iter(minibatches(buf, 2048, generator=gen, normalize=(sel.mean, max(sel.std, 1e-6)), selection=sel)))
    mb = type(mb)(*(c.clone() for c in mb))
    params = list(model.parameters())

    def torch_grads(mdl, dtype):
        c = lambda x: x.to(dtype)
        loss, _ = synth.torch_head(mdl.policy(c(mb.observations)), c(mb.log_mask), mdl.value(c(mb.observations)).squeeze(-1), mb.actions,
                                   c(mb.logp), c(mb.advantages), c(mb.value_targets), c(mb.values), clip=0.3)
        return [g.double() for g in torch.autograd.grad(loss, list(mdl.parameters()))]

    import copy

    g32 = torch_grads(model, torch.float32)
    g64 = torch_grads(copy.deepcopy(model).double(), torch.float64)
    logits, value = model.policy(mb.observations), model.value(mb.observations)
    res = ppo_loss(logits, value, mb, clip=0.3)
    gk = [g.double() for g in torch.autograd.grad([logits, value], params, [res.grad_logits, res.grad_value])]
    for p, a, b, k in zip(params, g32, g64, gk):
        dev32 = float((a - b).abs().max())
        got = float((k - a).abs().max())
        print(f"param {tuple(p.shape)}: torch f32 vs f64 {dev32:.3e}, kernel vs torch f32 {got:.3e}, scale {float(b.abs().max()):.3e}")
        assert got <= MARGIN * dev32, (tuple(p.shape), got, dev32)

    opt = torch.optim.Adam(model.parameters(), lr=3e-4)
    before = [p.detach().clone() for p in model.policy.parameters()]
    out = ppo_update(model, buf, opt, epochs=3, minibatch=2048, gae=(0.99, 1.0), native_batches=True, native_loss=True)
    keys = ("policy_loss", "vf_loss", "kl", "entropy", "clip_fraction")
    assert all(set(out[k]) == set(keys) for k in ("first", "last"))
    assert all(np.isfinite([out[k][j] for k in ("first", "last") for j in keys]))
    assert out["transitions"] == sel.count
    assert out["last"]["vf_loss"] < out["first"]["vf_loss"]
    assert abs(out["last"]["kl"]) < 0.05
    assert any(float((p.detach() - q).abs().max()) > 0 for p, q in zip(model.policy.parameters(), before))
    pol.close(), val.close(), env.close()
