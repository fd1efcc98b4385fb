"""numpy float64 restatement of one branch's training forward and backward (include/skyjo_vec.h: skyjo_vec_mlp_train_forward /
_backward) - Linear(D, 256) - tanh - Linear(256, 256) - tanh - Linear(256, O) - and the seeded inputs of
tests/test_mlp_train_ref.py and tests/test_gpu_mlp_train.py.  Written from the documents; it shares no code with the library.  Not
collected: a helper."""
import functools

import numpy as np

from tests import mlp_pack_ref

H = 256
SHAPES = mlp_pack_ref.SHAPES                  # (obs_dim, out_dim): (31, 26), (31, 1), (17, 26), (1, 32)
TILE_ROWS, CHUNK_ROWS = 64, 256               # learner.TRAIN_TILE_ROWS / TRAIN_CHUNK_ROWS (tests/test_mlp_train_ref.py compares them)
ROW_COUNTS = tuple(sorted({1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1025, 4097} |
                          {n + d for n in (TILE_ROWS, CHUNK_ROWS) for d in (-1, 0, 1)}))
WEIGHT_SETS = ("A", "S")
SATURATE = 8.0                                # set S: w1 of set A times this
FLOAT_X_CASE = ((17, 26), 257)                # the one (shape, rows) whose x is not integer-valued
ZERO_COLUMNS = (3, 11, 25)                    # columns of grad_out that are 0 in every row of a 26-wide shape
PARAMS = ("w1", "b1", "w2", "b2", "w3", "b3")
OUTPUTS = ("out", "h1", "h2") + PARAMS        # what a case is compared on; the gradients under the parameters' names

# The largest deviation of torch's float32 evaluation on the CPU from the float64 restatement, per output and weight set, each
# divided by the output's float64 max-abs in its case, over every shape x row count (``float32_deviation``).  torch's matmul
# splits its sums by the number of threads, so the figures were measured with 1, 2, 4 and 8 threads and the largest taken (only w1
# and w3 moved: w3 of set A 1.58e-06 with one thread, 6.3e-07 with eight), rounded up to two digits; ``float32_deviation`` itself
# runs with one thread so that tests/test_mlp_train_ref.py, which asserts that a fresh measurement does not exceed them and that
# none is 0, sees the same sums everywhere.  tests/test_gpu_mlp_train.py allows the kernels MARGIN = 4 times these.
F32_DEVIATION = {
    "A": {"out": 9.5e-07, "h1": 2.2e-06, "h2": 9.9e-07, "w1": 1.3e-06, "b1": 8.5e-07, "w2": 1.3e-06, "b2": 5.6e-07, "w3": 1.6e-06, "b3": 2.3e-06},
    "S": {"out": 9.6e-07, "h1": 1.3e-05, "h2": 1.2e-06, "w1": 3.3e-06, "b1": 3.0e-06, "w2": 3.4e-06, "b2": 8.6e-07, "w3": 1.4e-06, "b3": 2.3e-06},
}


@functools.lru_cache(maxsize=None)
def weights(shape, wset):
    """(w1, b1, w2, b2, w3, b3) float32 in nn.Linear layout.  Set A: torch's default initialisation under a seed; set S: A with w1
    times SATURATE, so that on integer-valued x a good share of layer 1 saturates (tanh = +-1 exactly in float32: 1 - h^2 = 0)."""
    import torch

    obs_dim, out_dim = shape
    gen_state = torch.random.get_rng_state()
    torch.manual_seed(4000 + 100 * obs_dim + out_dim)
    lins = [torch.nn.Linear(obs_dim, H), torch.nn.Linear(H, H), torch.nn.Linear(H, out_dim)]
    torch.random.set_rng_state(gen_state)
    p = [t.detach().numpy().copy() for lin in lins for t in (lin.weight, lin.bias)]
    if wset == "S":
        p[0] = (p[0] * np.float32(SATURATE)).astype(np.float32)
    assert wset in WEIGHT_SETS
    for t in p:
        t.setflags(write=False)
    return tuple(p)


@functools.lru_cache(maxsize=None)
def inputs(shape, m):
    """(x float32 [m][obs_dim], grad_out float32 [m][out_dim]).  x: the values of observation bytes, -2 .. 12 (FLOAT_X_CASE: normal
    floats); grad_out: normal / m with every fifth row all zero (rows 4, 9, ...) and, 26 wide, the ZERO_COLUMNS zero in every row -
    what the loss head gives for clipped rows and masked actions."""
    obs_dim, out_dim = shape
    rng = np.random.default_rng(7000 + 100000 * obs_dim + 1000 * out_dim + m)
    if (shape, m) == FLOAT_X_CASE:
        x = rng.normal(0.0, 3.0, (m, obs_dim)).astype(np.float32)
    else:
        x = rng.integers(-2, 13, (m, obs_dim)).astype(np.float32)
    g = (rng.normal(0.0, 1.0, (m, out_dim)) / m).astype(np.float32)
    g[4::5] = 0.0
    if out_dim == 26:
        g[:, list(ZERO_COLUMNS)] = 0.0
    x.setflags(write=False), g.setflags(write=False)
    return x, g


def forward_backward(params, x, g):
    """The definition in float64: {"out", "h1", "h2", and the gradients "w1" .. "b3"} of sum(out * g)."""
    w1, b1, w2, b2, w3, b3 = (np.asarray(p, dtype=np.float64) for p in params)
    x, g = np.asarray(x, dtype=np.float64), np.asarray(g, dtype=np.float64)
    h1 = np.tanh(x @ w1.T + b1)
    h2 = np.tanh(h1 @ w2.T + b2)
    out = h2 @ w3.T + b3
    dz2 = (g @ w3) * (1.0 - h2 * h2)
    dz1 = (dz2 @ w2) * (1.0 - h1 * h1)
    return {"out": out, "h1": h1, "h2": h2, "w3": g.T @ h2, "b3": g.sum(axis=0), "w2": dz2.T @ h1, "b2": dz2.sum(axis=0),
            "w1": dz1.T @ x, "b1": dz1.sum(axis=0)}


@functools.lru_cache(maxsize=None)
def reference(shape, wset, m):
    """``forward_backward`` of the case, computed once and shared (do not write to it)."""
    x, g = inputs(shape, m)
    return forward_backward(weights(shape, wset), x, g)


def torch_forward_backward(params, x, g, dtype):
    """The same through torch's nn.functional and autograd on the CPU in ``dtype``: the dict of ``forward_backward`` as float64 numpy."""
    import torch

    p = [torch.from_numpy(np.array(t)).to(dtype).requires_grad_() for t in params]
    xt, gt = torch.from_numpy(np.array(x)).to(dtype), torch.from_numpy(np.array(g)).to(dtype)
    h1 = torch.tanh(torch.nn.functional.linear(xt, p[0], p[1]))
    h2 = torch.tanh(torch.nn.functional.linear(h1, p[2], p[3]))
    out = torch.nn.functional.linear(h2, p[4], p[5])
    grads = torch.autograd.grad(out, p, gt)
    res = {"out": out, "h1": h1, "h2": h2}
    res.update(zip(PARAMS, grads))
    return {k: v.detach().double().numpy() for k, v in res.items()}


def normalised_deviation(got, want):
    """max |got - want| / max |want|; 0 where both are all zero."""
    d, s = float(np.abs(np.asarray(got, dtype=np.float64) - want).max()), float(np.abs(want).max())
    return d / s if s > 0.0 else (0.0 if d == 0.0 else float("inf"))


def float32_deviation():
    """{weight set: {output: the largest ``normalised_deviation`` of torch float32 on the CPU from the restatement}} over every
    shape x row count: what a correct float32 evaluation may be off by."""
    import torch

    dev = {ws: dict.fromkeys(OUTPUTS, 0.0) for ws in WEIGHT_SETS}
    threads = torch.get_num_threads()
    torch.set_num_threads(1)  # (see F32_DEVIATION)
    try:
        for ws in WEIGHT_SETS:
            for shape in SHAPES:
                for m in ROW_COUNTS:
                    x, g = inputs(shape, m)
                    want = reference(shape, ws, m)
                    got = torch_forward_backward(weights(shape, ws), x, g, torch.float32)
                    for k in OUTPUTS:
                        dev[ws][k] = max(dev[ws][k], normalised_deviation(got[k], want[k]))
    finally:
        torch.set_num_threads(threads)
    return dev
