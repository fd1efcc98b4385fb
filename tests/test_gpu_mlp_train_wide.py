"""``skyjo_vec_mlp_train_wide_forward`` / ``_backward`` and ``learner.NativeWideBranch`` (csrc/skyjo_train_wide.h: a branch's training
forward and backward at 32 to 163 inputs, on the float32 matrix instruction) on the GPU against the float64 definition
(``tests.mlp_train_ref.forward_backward`` on the cases of tests/mlp_train_wide_ref.py): every output within the recorded float32
deviation, untouched guard tails around every output and an exactly sized workspace, exact zeros, the bias column on both sides of a
step of the padded width, bit-identical repeats and reuse, a non-default stream, argument validation and the autograd wrapper - the
structure of tests/test_gpu_mlp_train.py."""
import ctypes

import numpy as np
import pytest

from tests import mlp_train_ref, mlp_train_wide_ref as ref

pytestmark = pytest.mark.gpu

# The kernels are allowed MARGIN (the project's factor: tests/test_gpu_mlp_train.py) times the deviation a correct float32 evaluation shows
# on the same cases (ref.F32_DEVIATION_WIDE, scale-normalised per output).
MARGIN = 4.0
SENTINEL = 0x7FC0DEAD      # a NaN with a payload: the guard tails' pattern, as float32 bits
GUARD = 64                 # elements before and after every output and the workspace
H = ref.H
deviation = mlp_train_ref.normalised_deviation


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


def _device_case(shape, wset, m, dev, x=None):
    import torch

    x0, g = ref.inputs(shape, m)
    t = lambda a: torch.from_numpy(np.array(a)).to(dev)
    return [t(p) for p in ref.weights(shape, wset)], t(x0 if x is None else x), t(g)


def _run_guarded(shape, wset, m, grad_out=None, x=None, params=None):
    """The two C entries on guarded outputs and a workspace of exactly workspace_bytes: the dict of ``ref.OUTPUTS`` as float32 numpy.
    The tails are checked after the forward and again after the backward."""
    import torch

    from skyjo_rl_amd import _lib

    L = _lib.load()
    dev = torch.device("cuda", 0)
    D, O = shape
    params0, x, g = _device_case(shape, wset, m, dev, x)
    params = params0 if params is None else [torch.from_numpy(np.array(p)).to(dev) for p in params]
    if grad_out is not None:
        g = grad_out
    nbytes = int(L.skyjo_vec_mlp_train_wide_workspace_bytes(D, O, m))
    assert nbytes == ref.workspace_bytes(D, O, m) and nbytes > 0
    out, ws = _guarded(m * O, dev), _guarded(nbytes // 4, dev)
    grads = [_guarded(p.numel(), dev) for p in params]
    bufs = [out, ws] + grads
    stream = torch.cuda.current_stream().cuda_stream
    rc = L.skyjo_vec_mlp_train_wide_forward(D, O, _ptrs(params), x.data_ptr(), m, out[1].data_ptr(), ws[1].data_ptr(), nbytes, stream)
    assert rc == 0, L.skyjo_vec_last_error()
    _tails_intact(bufs)
    assert all(bool((gr[1].view(torch.int32) == SENTINEL).all()) for gr in grads), "the forward wrote a gradient"
    bits = lambda t: t.view(torch.int32)
    assert not bool((bits(out[1]) == SENTINEL).any()) and not bool((bits(ws[1][:2 * m * H]) == SENTINEL).any())
    assert bool((bits(ws[1][2 * m * H:]) == SENTINEL).all()), "the forward wrote beyond h1 and h2"
    rc = L.skyjo_vec_mlp_train_wide_backward(D, O, _ptrs(params), x.data_ptr(), g.data_ptr(), m, _ptrs([gr[1] for gr in grads]),
                                             ws[1].data_ptr(), nbytes, stream)
    assert rc == 0, L.skyjo_vec_last_error()
    _tails_intact(bufs)
    assert not any(bool((bits(gr[1]) == SENTINEL).any()) for gr in grads), "a gradient has elements the kernels did not write"
    assert not bool((bits(ws[1][2 * m * H:4 * m * H]) == SENTINEL).any())
    res = {"out": out[1].view(m, O), "h1": ws[1][:m * H].view(m, H), "h2": ws[1][m * H:2 * m * H].view(m, H)}
    res.update({k: gr[1].view(p.shape) for k, gr, p in zip(ref.PARAMS, grads, params)})
    return {k: v.cpu().numpy() for k, v in res.items()}


@pytest.mark.parametrize("m", ref.ROW_COUNTS_WIDE)
@pytest.mark.parametrize("wset", ref.WEIGHT_SETS)
@pytest.mark.parametrize("shape", ref.SHAPES_WIDE)
def test_kernel_against_definition(shape, wset, m):
    want = ref.reference(shape, wset, m)
    got = _run_guarded(shape, wset, m)
    devs = {k: deviation(got[k], want[k]) for k in ref.OUTPUTS}
    print(f"shape={shape} set={wset} m={m}: " + " ".join("%s %.3e" % kv for kv in devs.items()))
    for k in ref.OUTPUTS:
        assert got[k].shape == want[k].shape
        assert devs[k] <= MARGIN * ref.F32_DEVIATION_WIDE[wset][k], (k, devs[k], ref.F32_DEVIATION_WIDE[wset][k])
    if shape[1] == 26:  # a column of grad_out that is zero in every row: exactly zero rows of dW3 and entries of db3
        assert (got["w3"][list(ref.ZERO_COLUMNS)] == 0.0).all() and (got["b3"][list(ref.ZERO_COLUMNS)] == 0.0).all()
    if wset == "S":     # the saved activation of a saturated unit is +-1 exactly
        assert (np.abs(got["h1"]) == 1.0).mean() > 0.2


def test_zero_grad_out_gives_exact_zeros():
    import torch

    shape, m = (163, 26), 257
    got = _run_guarded(shape, "A", m, grad_out=torch.zeros((m, shape[1]), dtype=torch.float32, device="cuda:0"))
    for k in ref.PARAMS:
        assert (got[k] == 0.0).all(), k


@pytest.mark.parametrize("shape", [(39, 26), (40, 1)], ids=["no_zero_padding_column", "seven_zero_padding_columns"])
def test_zero_column_of_x_and_the_bias_column(shape):
    """A column of x that is zero in every row gives an exactly zero column of dW1; and with b1 far from zero - so that a bias read from
    another padded column, or db1 taken from one, shows at once - w1 and b1 stay within the bound on both sides of a step of K."""
    m, zero_cols = 257, (0, 17, shape[0] - 1)
    x = np.array(ref.inputs(shape, m)[0])
    x[:, list(zero_cols)] = 0.0
    params = [np.array(p) for p in ref.weights(shape, "A")]
    params[1] = (params[1] + np.float32(0.75) * np.where(np.arange(H) % 2 == 0, 1, -1)).astype(np.float32)
    want = mlp_train_ref.forward_backward(params, x, ref.inputs(shape, m)[1])
    got = _run_guarded(shape, "A", m, x=x, params=params)
    assert (got["w1"][:, list(zero_cols)] == 0.0).all() and (got["w1"] != 0.0).any()
    for k in ref.OUTPUTS:
        d = deviation(got[k], want[k])
        print(f"shape={shape} {k}: {d:.3e} (bound {MARGIN * ref.F32_DEVIATION_WIDE['A'][k]:.3e})")
        assert d <= MARGIN * ref.F32_DEVIATION_WIDE["A"][k], (k, d)


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
    """forward and backward through a branch: clones of out and of the six .grad, as int32 bits."""
    import torch

    out = br.forward(x).clone()
    br.backward(g)
    assert all(p.grad is gr for p, gr in zip(seq.parameters(), br.grads))
    return [t.clone().view(torch.int32) for t in [out] + list(br.grads)]


def test_deterministic_and_reusable():
    import torch

    from skyjo_rl_amd.learner import NativeWideBranch

    dev = torch.device("cuda", 0)
    shape = (67, 26)
    seq = _seq(shape, "A", dev)
    t = lambda a: torch.from_numpy(np.array(a)).to(dev)
    (xa, ga), (xb, gb) = ([t(a) for a in ref.inputs(shape, m)] for m in (1025, 33))
    fresh_a = _branch_bits(NativeWideBranch(seq, 1025), seq, xa, ga)
    fresh_b = _branch_bits(NativeWideBranch(seq, 33), seq, xb, gb)
    br = NativeWideBranch(seq, 1025)
    assert br.max_rows == 1025 and br.workspace.numel() * 4 == ref.workspace_bytes(67, 26, 1025)
    first = _branch_bits(br, seq, xa, ga)
    again = _branch_bits(br, seq, xa, ga)
    small = _branch_bits(br, seq, xb, gb)            # fewer rows, chunks and tiles in the same workspace ...
    back = _branch_bits(br, seq, xa, ga)             # ... and the large batch again: stale partials or tail rows would show
    for got, want in ((first, fresh_a), (again, fresh_a), (small, fresh_b), (back, fresh_a)):
        assert all(torch.equal(a, b) for a, b in zip(got, want))
    out = br.forward(xb)
    assert out.data_ptr() == br.out.data_ptr() and out.shape == (33, 26)


def test_non_default_stream():
    import torch

    from skyjo_rl_amd.learner import NativeWideBranch

    dev = torch.device("cuda", 0)
    shape = (43, 26)
    seq = _seq(shape, "A", dev)
    x, g = (torch.from_numpy(np.array(a)).to(dev) for a in ref.inputs(shape, 1025))
    want = _branch_bits(NativeWideBranch(seq, 1025), seq, x, g)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    br = NativeWideBranch(seq, 1025)
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
    from skyjo_rl_amd.learner import NativeBranch, NativeWideBranch, native_branch

    L = _lib.load()
    dev = torch.device("cuda", 0)
    shape, m = (43, 26), 65
    D, O = shape
    params, x, g = _device_case(shape, "A", m, dev)
    nbytes = int(L.skyjo_vec_mlp_train_wide_workspace_bytes(D, O, m))
    assert nbytes == ref.workspace_bytes(D, O, m)
    fill = lambda n: torch.full((n,), SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)
    out, ws, grads = fill(m * O), fill(nbytes // 4 + 4), [fill(p.numel()) for p in params]
    for bad in ((31, O, m), (164, O, m), (0, O, m), (D, 0, m), (D, 33, m), (D, O, 0), (D, O, -1)):
        assert L.skyjo_vec_mlp_train_wide_workspace_bytes(*bad) == 0 and ref.workspace_bytes(*bad) == 0
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
    bad_f += [ch(fwd, 0, 31), ch(fwd, 0, 164), ch(fwd, 0, 0), ch(fwd, 1, 0), ch(fwd, 1, 33), ch(fwd, 4, 0), ch(fwd, 4, -1),
              ch(fwd, 7, nbytes - 1), ch(fwd, 7, 0), ch(fwd, 2, shifted(2)), ch(fwd, 2, shifted(4)), ch(fwd, 6, vp(ws) + 4)]
    bad_b = [ch(bwd, k, None) for k in (2, 3, 4, 6, 7)] + [ch(bwd, 2, with_null(params, i)) for i in range(6)]
    bad_b += [ch(bwd, 6, with_null(grads, i)) for i in range(6)]
    bad_b += [ch(bwd, 0, 31), ch(bwd, 0, 164), ch(bwd, 0, 0), ch(bwd, 1, 0), ch(bwd, 1, 33), ch(bwd, 5, 0), ch(bwd, 5, -1),
              ch(bwd, 8, nbytes - 1), ch(bwd, 8, 0), ch(bwd, 2, shifted(2)), ch(bwd, 2, shifted(4)), ch(bwd, 7, vp(ws) + 4)]
    for args in bad_f:
        assert L.skyjo_vec_mlp_train_wide_forward(*args) == -1, args
        assert b"skyjo_vec_mlp_train_wide_forward" in L.skyjo_vec_last_error()
    for args in bad_b:
        assert L.skyjo_vec_mlp_train_wide_backward(*args) == -1, args
        assert b"skyjo_vec_mlp_train_wide_backward" in L.skyjo_vec_last_error()

    # NativeWideBranch: ValueError before any launch
    seq = _seq(shape, "A", dev)
    br = NativeWideBranch(seq, m)
    br.out.view(torch.int32).fill_(SENTINEL), br.workspace.view(torch.int32).fill_(SENTINEL)
    for gr in br.grads:
        gr.view(torch.int32).fill_(SENTINEL)
    with pytest.raises(ValueError):
        br.backward(g)                                                   # no forward yet
    for bad_x in (x.double(), x.cpu(), x[:, :42], x.t().contiguous().t(), torch.cat([x, x]), x[:0], x.reshape(-1)):
        with pytest.raises(ValueError):
            br.forward(bad_x)
    for args in ((seq, 0), (seq[:3], m), (_seq(shape, "A", dev).double(), m), (_seq(shape, "A", dev).cpu(), m)):
        with pytest.raises(ValueError):
            NativeWideBranch(*args)
    with pytest.raises(ValueError, match="32..163 inputs"):              # its own range, in its own words
        NativeWideBranch(_seq((31, 26), "A", dev), m)
    with pytest.raises(ValueError, match="1..31 inputs"):
        NativeBranch(seq, m)
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
    # native_branch: the class that fits layer 1's width
    assert type(native_branch(_seq((31, 26), "A", dev), m)) is NativeBranch
    assert type(native_branch(_seq((32, 26), "A", dev), m)) is NativeWideBranch
    assert type(native_branch(_seq((163, 32), "A", dev), m)) is NativeWideBranch
    # and the good calls are good
    assert L.skyjo_vec_mlp_train_wide_forward(*fwd) == 0 and L.skyjo_vec_mlp_train_wide_backward(*bwd) == 0
    torch.cuda.synchronize()


def test_autograd_function():
    import torch

    from skyjo_rl_amd.learner import NativeWideBranch

    dev = torch.device("cuda", 0)
    shape, m = (43, 26), 257
    seq = _seq(shape, "A", dev)
    x, g = (torch.from_numpy(np.array(a)).to(dev) for a in ref.inputs(shape, m))
    c = g * m                                         # the incoming gradient of out in (out * c).sum()
    br = NativeWideBranch(seq, m)
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
