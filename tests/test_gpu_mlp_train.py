"""``skyjo_vec_mlp_train_forward`` / ``_backward`` and ``learner.NativeBranch`` (csrc/skyjo_train.h: a branch's training forward and
backward on the float32 matrix instruction) on the GPU against the float64 restatement of tests/mlp_train_ref.py: every output within
the recorded float32 deviation, untouched guard tails around every output and an exactly sized workspace, exact zeros, bit-identical
repeats and reuse, a non-default stream, argument validation, the autograd wrapper and the hand-off to ``ppo_loss``, ``NativeAdam``
and ``examples.ppo.ppo_update(native_nets=True)``."""
import ctypes

import numpy as np
import pytest

from tests import mlp_train_ref as ref

pytestmark = pytest.mark.gpu

# The kernels are allowed MARGIN times the deviation torch's own float32 evaluation shows on the same cases (ref.F32_DEVIATION, scale-
# normalised per output): room for another, equally valid float32 summation order and for a device tanhf within a couple of ulp.
MARGIN = 4.0
SENTINEL = 0x7FC0DEAD      # a NaN with a payload: the guard tails' pattern, as float32 bits
GUARD = 64                 # elements before and after every output and the workspace
H = ref.H


def _guarded(n, dev):
    """float32 [n] inside a larger tensor filled with the sentinel: (whole, view); the view starts 16-byte aligned."""
    import torch

    whole = torch.empty((GUARD + n + GUARD,), dtype=torch.float32, device=dev)
    whole.view(torch.int32).fill_(SENTINEL)
    return whole, whole[GUARD:GUARD + n]


def _tails_intact(bufs):
    import torch

    for whole, view in bufs:
        w = whole.view(torch.int32)
        assert bool((w[:GUARD] == SENTINEL).all()) and bool((w[GUARD + view.numel():] == SENTINEL).all()), "a guard tail was written"


def _ptrs(tensors):
    return (ctypes.c_void_p * 6)(*[t.data_ptr() for t in tensors])


def _device_case(shape, wset, m, dev):
    import torch

    x, g = ref.inputs(shape, m)
    t = lambda a: torch.from_numpy(np.array(a)).to(dev)
    return [t(p) for p in ref.weights(shape, wset)], t(x), t(g)


def _run_guarded(shape, wset, m, grad_out=None, stream_ptr=None):
    """The two C entries on guarded outputs and a workspace of exactly workspace_bytes: the dict of ``ref.OUTPUTS`` as float32 numpy.
    The tails are checked after the forward and again after the backward."""
    import torch

    from skyjo_rl_amd import _lib

    L = _lib.load()
    dev = torch.device("cuda", 0)
    D, O = shape
    params, x, g = _device_case(shape, wset, m, dev)
    if grad_out is not None:
        g = grad_out
    nbytes = int(L.skyjo_vec_mlp_train_workspace_bytes(D, O, m))
    chunks = (m + ref.CHUNK_ROWS - 1) // ref.CHUNK_ROWS
    assert nbytes == 4 * (4 * m * H + chunks * 82208)
    out, ws = _guarded(m * O, dev), _guarded(nbytes // 4, dev)
    grads = [_guarded(p.numel(), dev) for p in params]
    bufs = [out, ws] + grads
    stream = torch.cuda.current_stream().cuda_stream if stream_ptr is None else stream_ptr
    rc = L.skyjo_vec_mlp_train_forward(D, O, _ptrs(params), x.data_ptr(), m, out[1].data_ptr(), ws[1].data_ptr(), nbytes, stream)
    assert rc == 0, L.skyjo_vec_last_error()
    _tails_intact(bufs)
    assert all(bool((gr[1].view(torch.int32) == SENTINEL).all()) for gr in grads), "the forward wrote a gradient"
    bits = lambda t: t.view(torch.int32)
    assert not bool((bits(out[1]) == SENTINEL).any()) and not bool((bits(ws[1][:2 * m * H]) == SENTINEL).any())
    assert bool((bits(ws[1][2 * m * H:]) == SENTINEL).all()), "the forward wrote beyond h1 and h2"
    rc = L.skyjo_vec_mlp_train_backward(D, O, _ptrs(params), x.data_ptr(), g.data_ptr(), m, _ptrs([gr[1] for gr in grads]), ws[1].data_ptr(),
                                        nbytes, stream)
    assert rc == 0, L.skyjo_vec_last_error()
    _tails_intact(bufs)
    assert not any(bool((bits(gr[1]) == SENTINEL).any()) for gr in grads), "a gradient has elements the kernels did not write"
    assert not bool((bits(ws[1][2 * m * H:4 * m * H]) == SENTINEL).any())
    res = {"out": out[1].view(m, O), "h1": ws[1][:m * H].view(m, H), "h2": ws[1][m * H:2 * m * H].view(m, H)}
    res.update({k: gr[1].view(p.shape) for k, gr, p in zip(ref.PARAMS, grads, params)})
    return {k: v.cpu().numpy() for k, v in res.items()}


@pytest.mark.parametrize("m", ref.ROW_COUNTS)
@pytest.mark.parametrize("wset", ref.WEIGHT_SETS)
@pytest.mark.parametrize("shape", ref.SHAPES)
def test_kernel_against_restatement(shape, wset, m):
    want = ref.reference(shape, wset, m)
    got = _run_guarded(shape, wset, m)
    devs = {k: ref.normalised_deviation(got[k], want[k]) for k in ref.OUTPUTS}
    print(f"shape={shape} set={wset} m={m}: " + " ".join("%s %.3e" % kv for kv in devs.items()))
    for k in ref.OUTPUTS:
        assert got[k].shape == want[k].shape
        assert devs[k] <= MARGIN * ref.F32_DEVIATION[wset][k], (k, devs[k], ref.F32_DEVIATION[wset][k])
    if shape[1] == 26:  # a column of grad_out that is zero in every row: exactly zero rows of dW3 and entries of db3
        assert (got["w3"][list(ref.ZERO_COLUMNS)] == 0.0).all() and (got["b3"][list(ref.ZERO_COLUMNS)] == 0.0).all()
    if wset == "S":     # the saved activation of a saturated unit is +-1 exactly
        assert (np.abs(got["h1"]) == 1.0).mean() > 0.2


@pytest.mark.parametrize("shape,m", [((31, 26), 257), ((1, 32), 4097)])
def test_zero_grad_out_gives_exact_zeros(shape, m):
    import torch

    got = _run_guarded(shape, "A", m, grad_out=torch.zeros((m, shape[1]), dtype=torch.float32, device="cuda:0"))
    for k in ref.PARAMS:
        assert (got[k] == 0.0).all(), k


def _seq(shape, wset, dev):
    import torch
    from torch import nn

    D, O = shape
    seq = nn.Sequential(nn.Linear(D, H), nn.Tanh(), nn.Linear(H, H), nn.Tanh(), nn.Linear(H, O)).to(dev)
    with torch.no_grad():
        for p, w in zip(seq.parameters(), ref.weights(shape, wset)):
            p.copy_(torch.from_numpy(np.array(w)))
    return seq


def _branch_bits(br, seq, x, g):
    """forward and backward through a NativeBranch: clones of out and of the six .grad, as int32 bits."""
    import torch

    out = br.forward(x).clone()
    br.backward(g)
    assert all(p.grad is gr for p, gr in zip(seq.parameters(), br.grads))
    return [t.clone().view(torch.int32) for t in [out] + list(br.grads)]


def test_deterministic_and_reusable():
    import torch

    from skyjo_rl_amd.learner import NativeBranch

    dev = torch.device("cuda", 0)
    shape = (31, 26)
    seq = _seq(shape, "A", dev)
    t = lambda a: torch.from_numpy(np.array(a)).to(dev)
    (xa, ga), (xb, gb) = ([t(a) for a in ref.inputs(shape, m)] for m in (4097, 33))
    fresh_a = _branch_bits(NativeBranch(seq, 4097), seq, xa, ga)
    fresh_b = _branch_bits(NativeBranch(seq, 33), seq, xb, gb)
    br = NativeBranch(seq, 4097)
    first = _branch_bits(br, seq, xa, ga)
    again = _branch_bits(br, seq, xa, ga)
    small = _branch_bits(br, seq, xb, gb)            # fewer rows, chunks and tiles in the same workspace ...
    back = _branch_bits(br, seq, xa, ga)             # ... and the large batch again: stale partials or tail rows would show
    for got, want in ((first, fresh_a), (again, fresh_a), (small, fresh_b), (back, fresh_a)):
        assert all(torch.equal(a, b) for a, b in zip(got, want))
    out = br.forward(xb)
    assert out.data_ptr() == br.out.data_ptr() and out.shape == (33, 26)
    for p in seq.parameters():                       # zero_grad(set_to_none=True) between steps changes nothing
        p.grad = None
    br.backward(gb)
    assert all(p.grad is gr for p, gr in zip(seq.parameters(), br.grads))
    assert all(torch.equal(a.view(torch.int32), b) for a, b in zip(br.grads, small[1:]))


def test_non_default_stream():
    import torch

    from skyjo_rl_amd.learner import NativeBranch

    dev = torch.device("cuda", 0)
    shape = (17, 26)
    seq = _seq(shape, "A", dev)
    x, g = (torch.from_numpy(np.array(a)).to(dev) for a in ref.inputs(shape, 1025))
    want = _branch_bits(NativeBranch(seq, 1025), seq, x, g)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    br = NativeBranch(seq, 1025)
    with torch.cuda.stream(s):
        y = torch.zeros((1 << 20,), device=dev)
        for _ in range(8):
            y = y * 1.0001 + 1.0                     # work queued on the stream ahead of the calls
        x2 = x + y[:1] - y[:1]                       # ... which their input depends on (integer-valued x: the sum is exact)
        got = _branch_bits(br, seq, x2, g)
        same_input = torch.equal(x2, x)
    s.synchronize()
    assert same_input and all(torch.equal(a, b) for a, b in zip(got, want))


def test_validation_launches_nothing():
    import torch

    from skyjo_rl_amd import _lib
    from skyjo_rl_amd.learner import NativeBranch

    L = _lib.load()
    dev = torch.device("cuda", 0)
    shape, m = (31, 26), 65
    D, O = shape
    params, x, g = _device_case(shape, "A", m, dev)
    nbytes = int(L.skyjo_vec_mlp_train_workspace_bytes(D, O, m))
    fill = lambda n: torch.full((n,), SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)
    out, ws, grads = fill(m * O), fill(nbytes // 4 + 4), [fill(p.numel()) for p in params]
    for bad in ((0, O, m), (32, O, m), (D, 0, m), (D, 33, m), (D, O, 0), (D, O, -3)):
        assert L.skyjo_vec_mlp_train_workspace_bytes(*bad) == 0
    vp = lambda t: t.data_ptr()
    pp, gg = _ptrs(params), _ptrs(grads)

    def with_null(tensors, i):
        a = _ptrs(tensors)
        a[i] = None
        return a

    shifted = lambda i: (ctypes.c_void_p * 6)(*[vp(p) + (4 if k == i else 0) for k, p in enumerate(params)])
    fwd = [D, O, pp, vp(x), m, vp(out), vp(ws), nbytes, None]
    bwd = [D, O, pp, vp(x), vp(g), m, gg, vp(ws), nbytes, None]
    ch = lambda base, k, v: base[:k] + [v] + base[k + 1:]
    bad_f = [ch(fwd, k, None) for k in (2, 3, 5, 6)] + [ch(fwd, 2, with_null(params, i)) for i in range(6)]
    bad_f += [ch(fwd, 0, 0), ch(fwd, 0, 32), ch(fwd, 1, 0), ch(fwd, 1, 33), ch(fwd, 4, 0), ch(fwd, 4, -1), ch(fwd, 7, nbytes - 1), ch(fwd, 7, 0),
              ch(fwd, 2, shifted(2)), ch(fwd, 2, shifted(4)), ch(fwd, 6, vp(ws) + 4)]
    bad_b = [ch(bwd, k, None) for k in (2, 3, 4, 6, 7)] + [ch(bwd, 2, with_null(params, i)) for i in range(6)]
    bad_b += [ch(bwd, 6, with_null(grads, i)) for i in range(6)]
    bad_b += [ch(bwd, 0, 0), ch(bwd, 0, 32), ch(bwd, 1, 0), ch(bwd, 1, 33), ch(bwd, 5, 0), ch(bwd, 5, -1), ch(bwd, 8, nbytes - 1), ch(bwd, 8, 0),
              ch(bwd, 2, shifted(2)), ch(bwd, 2, shifted(4)), ch(bwd, 7, vp(ws) + 4)]
    for args in bad_f:
        assert L.skyjo_vec_mlp_train_forward(*args) == -1, args
        assert b"skyjo_vec_mlp_train_forward" in L.skyjo_vec_last_error()
    for args in bad_b:
        assert L.skyjo_vec_mlp_train_backward(*args) == -1, args
        assert b"skyjo_vec_mlp_train_backward" in L.skyjo_vec_last_error()

    # NativeBranch: ValueError before any launch
    seq = _seq(shape, "A", dev)
    br = NativeBranch(seq, m)
    br.out.view(torch.int32).fill_(SENTINEL), br.workspace.view(torch.int32).fill_(SENTINEL)
    for gr in br.grads:
        gr.view(torch.int32).fill_(SENTINEL)
    with pytest.raises(ValueError):
        br.backward(g)                                                   # no forward yet
    for bad_x in (x.double(), x.cpu(), x[:, :30], x.t().contiguous().t(), torch.cat([x, x]), x[:0], x.reshape(-1)):
        with pytest.raises(ValueError):
            br.forward(bad_x)
    for args in ((seq, 0), (seq[:3], m), (_seq(shape, "A", dev).double(), m), (_seq(shape, "A", dev).cpu(), m)):
        with pytest.raises(ValueError):
            NativeBranch(*args)
    torch.cuda.synchronize()
    for t_ in [out, ws, br.out, br.workspace] + grads + br.grads:
        assert bool((t_.view(torch.int32) == SENTINEL).all()), "a refused call wrote an output"
    br.forward(x)
    for bad_g in (g.double(), g.cpu(), g[:64], g[:, :25], g.t().contiguous().t()):
        with pytest.raises(ValueError):
            br.backward(bad_g)
    torch.cuda.synchronize()
    assert all(bool((gr.view(torch.int32) == SENTINEL).all()) for gr in br.grads)
    seq[2].weight.data = seq[2].weight.data.t().contiguous().t()        # a parameter that stopped being contiguous
    with pytest.raises(ValueError):
        br.forward(x)
    # and the good calls are good
    assert L.skyjo_vec_mlp_train_forward(*fwd) == 0 and L.skyjo_vec_mlp_train_backward(*bwd) == 0
    torch.cuda.synchronize()


def test_autograd_function():
    import torch

    from skyjo_rl_amd.learner import NativeBranch

    dev = torch.device("cuda", 0)
    shape, m = (31, 26), 257
    seq = _seq(shape, "A", dev)
    x, g = (torch.from_numpy(np.array(a)).to(dev) for a in ref.inputs(shape, m))
    c = g * m                                         # the incoming gradient of out in (out * c).sum()
    br = NativeBranch(seq, m)
    want = _branch_bits(br, seq, x, c)
    for p in seq.parameters():
        p.grad = None
    out = br.apply(x)
    assert out.requires_grad and torch.equal(out.detach().view(torch.int32), want[0])
    (out * c).sum().backward()
    first = [p.grad.clone() for p in seq.parameters()]
    assert all(p.grad is not gr for p, gr in zip(seq.parameters(), br.grads))
    assert all(torch.equal(a.view(torch.int32), b) for a, b in zip(first, want[1:]))
    (br.apply(x) * c).sum().backward()                # a second backward accumulates: twice the gradient, exactly
    assert all(torch.equal(p.grad, 2.0 * a) for p, a in zip(seq.parameters(), first))
    stale = br.apply(x)
    br.forward(x)
    with pytest.raises(RuntimeError):
        (stale * c).sum().backward()                  # the workspace has served another forward since


def test_hand_off_to_loss_head_and_optimizer():
    import copy

    import torch

    from examples.ppo import ppo_update, repack
    from skyjo_rl_amd import SkyjoVecEnv, _lib
    from skyjo_rl_amd.action_mask_model import ActionMaskModel, FusedNet
    from skyjo_rl_amd.learner import NativeAdam, NativeBranch, ppo_loss
    from skyjo_rl_amd.rollout import RolloutBuffer, collect, compute_targets, minibatches, select_rows
    from tests import ppo_loss_synth as synth

    torch.manual_seed(0)
    B, N, T = 256, 3, 8
    env = SkyjoVecEnv(B, num_players=N)
    env.seed(None, 9)
    env.reset()
    model = ActionMaskModel(obs_dim=env.obs_dim).cuda()
    pol, val = repack(model)
    buf = RolloutBuffer(env, T)
    collect(env, pol, val, buf, seed=1, first_ticket=0)
    compute_targets(buf, gamma=0.99, lam=0.95)
    sel = select_rows(buf, _lib.TGT_HAS_TARGET)
    gen = torch.Generator(device="cuda").manual_seed(0)
    mb = next(iter(minibatches(buf, 1 << 15, generator=gen, normalize=(sel.mean, max(sel.std, 1e-6)), selection=sel)))
    mb = type(mb)(*(c.clone() for c in mb))
    m = mb.actions.numel()
    assert m == sel.count and 256 < m <= B * T

    # torch autograd on the same inputs in float64
    m64 = copy.deepcopy(model).double()
    c = lambda t: t.double()
    loss, _ = synth.torch_head(m64.policy(c(mb.observations)), c(mb.log_mask), m64.value(c(mb.observations)).squeeze(-1), mb.actions,
                               c(mb.logp), c(mb.advantages), c(mb.value_targets), c(mb.values), clip=0.3)
    branches = (list(m64.policy.parameters()), list(m64.value.parameters()))
    want = [torch.autograd.grad(loss, ps, retain_graph=True) for ps in branches]

    bp, bv = NativeBranch(model.policy, m), NativeBranch(model.value, m)
    logits, value = bp.forward(mb.observations), bv.forward(mb.observations)
    res = ppo_loss(logits, value, mb, clip=0.3)
    bp.backward(res.grad_logits), bv.backward(res.grad_value)
    for name, seq, w in (("policy", model.policy, want[0]), ("value", model.value, want[1])):
        for k, p, g64 in zip(ref.PARAMS, seq.parameters(), w):
            d = ref.normalised_deviation(p.grad.cpu().numpy(), g64.cpu().numpy())
            print(f"{name} {k}: {d:.3e} (bound {MARGIN * ref.F32_DEVIATION['A'][k]:.3e})")
            assert d <= MARGIN * ref.F32_DEVIATION["A"][k], (name, k, d)

    out = ppo_update(model, buf, NativeAdam(model, pol, val, lr=3e-4), epochs=2, minibatch=1024, gae=(0.99, 0.95), native_batches=True,
                     native_loss=True, native_nets=True)
    keys = ("policy_loss", "vf_loss", "kl", "entropy", "clip_fraction")
    assert all(set(out[k]) == set(keys) for k in ("first", "last")) and out["transitions"] == sel.count
    assert all(np.isfinite([out[k][j] for k in ("first", "last") for j in keys]))
    for net, seq in ((pol, model.policy), (val, model.value)):
        fresh = FusedNet(seq)
        assert torch.equal(net.export(), fresh.export())
        fresh.close()
    pol.close(), val.close(), env.close()
