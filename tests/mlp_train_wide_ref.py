"""The wide training branches' cases (include/skyjo_vec.h: skyjo_vec_mlp_train_wide_forward / _backward; 32 <= obs_dim <= 163): the
shapes, row counts and seeded inputs of tests/test_mlp_train_wide_ref.py and tests/test_gpu_mlp_train_wide.py, a numpy restatement of the
padded-width rule and the workspace size, and the float32 deviation the GPU test bounds the kernels with.  The float64 definition is
``tests.mlp_train_ref.forward_backward`` - imported, not restated - and the weight sets are ``tests.mlp_train_ref.weights``.  Written
from the documents; it shares no code with the library.  Not collected: a helper."""
import functools

import numpy as np

from tests import mlp_train_ref

H = mlp_train_ref.H
TILE_ROWS, CHUNK_ROWS = mlp_train_ref.TILE_ROWS, mlp_train_ref.CHUNK_ROWS
# (obs_dim, out_dim): the first wide width; a padded width with no zero column (39 -> 40); both sides of a step of K (39, 40); the
# direct observation at 2, 4 and 12 players (43, 67, 163); every out_dim class (26, 1, 32)
SHAPES_WIDE = ((32, 26), (39, 26), (40, 1), (43, 26), (67, 26), (67, 1), (163, 26), (163, 32))
ROW_COUNTS_WIDE = (1, 2, 63, 64, 65, 255, 256, 257, 1025)   # both sides of the tile and the chunk, and more than four chunks
WEIGHT_SETS = mlp_train_ref.WEIGHT_SETS                      # A: torch's default init under a seed; S: w1 of A times 8
FLOAT_X_CASE_WIDE = ((43, 26), 257)                          # the one (shape, rows) whose x is not integer-valued
ZERO_COLUMNS = mlp_train_ref.ZERO_COLUMNS
PARAMS, OUTPUTS = mlp_train_ref.PARAMS, mlp_train_ref.OUTPUTS
MIN_OBS, MAX_OBS = 32, 163
PART_FIXED = H * H + 32 * H + H + 32                         # 74 016: dW2, dW3 (padded to 32 rows), db2, db3 (padded to 32)

# What a correct float32 evaluation is off by: the largest ``mlp_train_ref.normalised_deviation`` from the float64 definition per weight
# set and output over every SHAPES_WIDE x ROW_COUNTS_WIDE case, the larger of two measurements, rounded up to two digits:
#   (a) torch's float32 on the CPU of the machine this was written on, with 1, 2, 4 and 8 threads (``torch_float32_deviation``) - torch's
#       matmul splits its sums by thread count and differs from host to host, so NO test asserts on it;
#   (b) ``float32_deviation``: the host-independent evaluation of ``numpy_float32`` - every product and every addition a float32 array
#       operation of its own, k ascending, tanh taken in float64 and rounded once.  tests/test_mlp_train_wide_ref.py measures (b) afresh
#       and asserts that it does not exceed these and is not 0.
# tests/test_gpu_mlp_train_wide.py allows the kernels MARGIN = 4 times these.
F32_DEVIATION_WIDE = {
    "A": {"out": 8.7e-07, "h1": 3.9e-06, "h2": 1.1e-06, "w1": 1.4e-06, "b1": 1.6e-06, "w2": 1.5e-06, "b2": 1.5e-06, "w3": 1.5e-06, "b3": 1.8e-06},
    "S": {"out": 1.7e-06, "h1": 3.1e-05, "h2": 3.0e-06, "w1": 7.3e-06, "b1": 7.6e-06, "w2": 6.1e-06, "b2": 2.0e-06, "w3": 1.6e-06, "b3": 1.8e-06},
}


def padded_width(obs_dim):
    """K = 8 (obs_dim // 8 + 1): layer 1's width with the bias column - a multiple of 8 with at least one free column."""
    return 8 * (obs_dim // 8 + 1)


def part_floats(obs_dim):
    """A chunk's partial record: dW2 [256][256], dW1 [256][K], dW3 [32][256], db2 [256], db3 [32]."""
    return PART_FIXED + H * padded_width(obs_dim)


def workspace_bytes(obs_dim, out_dim, m):
    """skyjo_vec_mlp_train_wide_workspace_bytes: h1, h2, dz2, dz1 [m][256] and a record per chunk of 256 rows; 0 for invalid arguments."""
    if not (MIN_OBS <= obs_dim <= MAX_OBS and 1 <= out_dim <= 32 and 1 <= m <= 1 << 30):
        return 0
    return 4 * (4 * m * H + -(-m // CHUNK_ROWS) * part_floats(obs_dim))


def padded_x(x):
    """x [m][D] as layer 1 takes it: [m][K], zeros in columns [D, K - 1) and a 1 in column K - 1 (against b1 in W1's column K - 1)."""
    m, d = x.shape
    k = padded_width(d)
    out = np.zeros((m, k), dtype=x.dtype)
    out[:, :d] = x
    out[:, k - 1] = 1
    return out


weights = mlp_train_ref.weights


@functools.lru_cache(maxsize=None)
def inputs(shape, m):
    """(x float32 [m][obs_dim], grad_out float32 [m][out_dim]), made as ``mlp_train_ref.inputs`` makes them: x the values of observation
    bytes, -2 .. 12 (FLOAT_X_CASE_WIDE: normal floats); grad_out normal / m with every fifth row all zero (rows 4, 9, ...) and, 26 wide,
    the ZERO_COLUMNS zero in every row."""
    obs_dim, out_dim = shape
    rng = np.random.default_rng(7000 + 100000 * obs_dim + 1000 * out_dim + m)
    if (shape, m) == FLOAT_X_CASE_WIDE:
        x = rng.normal(0.0, 3.0, (m, obs_dim)).astype(np.float32)
    else:
        x = rng.integers(-2, 13, (m, obs_dim)).astype(np.float32)
    g = (rng.normal(0.0, 1.0, (m, out_dim)) / m).astype(np.float32)
    g[4::5] = 0.0
    if out_dim == 26:
        g[:, list(ZERO_COLUMNS)] = 0.0
    x.setflags(write=False), g.setflags(write=False)
    return x, g


@functools.lru_cache(maxsize=None)
def reference(shape, wset, m):
    """``mlp_train_ref.forward_backward`` of the case, computed once and shared (do not write to it)."""
    x, g = inputs(shape, m)
    return mlp_train_ref.forward_backward(weights(shape, wset), x, g)


def _chain(a, b):
    """a [m][K] times b [n][K] transposed, float32: one chain per output over k ascending, the product and the addition separate float32
    array operations (no fused multiply-add, no blocking: the same bits on every host)."""
    acc = np.zeros((a.shape[0], b.shape[0]), dtype=np.float32)
    for k in range(a.shape[1]):
        acc = acc + a[:, k:k + 1] * b[None, :, k]
    return acc


def _tanh(z):
    return np.tanh(z.astype(np.float64)).astype(np.float32)


def numpy_float32(params, x, g):
    """The definition evaluated in float32 by ``_chain``: the dict of ``forward_backward`` as float32 numpy.  The bias joins the finished
    sum; the weight gradients' chains run over the rows, ascending, and so do the bias gradients' sums."""
    w1, b1, w2, b2, w3, b3 = (np.asarray(p, dtype=np.float32) for p in params)
    x, g = np.asarray(x, dtype=np.float32), np.asarray(g, dtype=np.float32)
    one = np.float32(1.0)
    h1 = _tanh(_chain(x, w1) + b1)
    h2 = _tanh(_chain(h1, w2) + b2)
    out = _chain(h2, w3) + b3
    dz2 = _chain(g, np.ascontiguousarray(w3.T)) * (one - h2 * h2)
    dz1 = _chain(dz2, np.ascontiguousarray(w2.T)) * (one - h1 * h1)
    t = lambda a: np.ascontiguousarray(a.T)
    ones = np.ones((1, x.shape[0]), dtype=np.float32)
    return {"out": out, "h1": h1, "h2": h2, "w3": _chain(t(g), t(h2)), "b3": _chain(ones, t(g))[0], "w2": _chain(t(dz2), t(h1)),
            "b2": _chain(ones, t(dz2))[0], "w1": _chain(t(dz1), t(x)), "b1": _chain(ones, t(dz1))[0]}


def float32_deviation():
    """(b) of F32_DEVIATION_WIDE: {weight set: {output: the largest normalised deviation of ``numpy_float32`` from the definition}}."""
    dev = {ws: dict.fromkeys(OUTPUTS, 0.0) for ws in WEIGHT_SETS}
    for ws in WEIGHT_SETS:
        for shape in SHAPES_WIDE:
            for m in ROW_COUNTS_WIDE:
                x, g = inputs(shape, m)
                want, got = reference(shape, ws, m), numpy_float32(weights(shape, ws), x, g)
                for k in OUTPUTS:
                    dev[ws][k] = max(dev[ws][k], mlp_train_ref.normalised_deviation(got[k], want[k]))
    return dev


def torch_float32_deviation(threads=1):
    """(a) of F32_DEVIATION_WIDE with ``threads`` threads: torch's float32 on this host's CPU.  A report: it differs between hosts."""
    import torch

    dev = {ws: dict.fromkeys(OUTPUTS, 0.0) for ws in WEIGHT_SETS}
    before = torch.get_num_threads()
    torch.set_num_threads(threads)
    try:
        for ws in WEIGHT_SETS:
            for shape in SHAPES_WIDE:
                for m in ROW_COUNTS_WIDE:
                    x, g = inputs(shape, m)
                    got = mlp_train_ref.torch_forward_backward(weights(shape, ws), x, g, torch.float32)
                    want = reference(shape, ws, m)
                    for k in OUTPUTS:
                        dev[ws][k] = max(dev[ws][k], mlp_train_ref.normalised_deviation(got[k], want[k]))
    finally:
        torch.set_num_threads(before)
    return dev
