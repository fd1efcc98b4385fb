"""tests/mlp_pack_ref.py, the numpy restatement of the packed net that tests/test_gpu_mlp_update.py compares the kernels with, checked
on its own: pack and its inverse agree about where every weight lies, hi + lo carry 16 significant bits, padding is zero, the Adam
inputs do separate float32 from float64 - and the ABI has the four entry points."""
import ctypes
import os
import re

import numpy as np
import pytest

from . import mlp_pack_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _coded(obs_dim, out_dim, by):
    """Weights that are small integers over S (so that the stored S * w is the integer to a rounding): the row, or the column."""
    code = lambda shape: (np.indices(shape)[by] % 251 + 1).astype(np.float32)
    w1, w2, w3 = code((256, obs_dim)), code((256, 256)), code((out_dim, 256))
    b1, b2, b3 = (np.arange(256) % 251 + 1).astype(np.float32), np.arange(256, dtype=np.float32), np.arange(out_dim, dtype=np.float32)
    return w1, b1, w2, b2, w3, b3


@pytest.mark.parametrize("obs_dim,out_dim", ref.SHAPES)
@pytest.mark.parametrize("by", [0, 1])
def test_pack_then_unpack_returns_every_weight_once(obs_dim, out_dim, by):
    w1, b1, w2, b2, w3, b3 = _coded(obs_dim, out_dim, by)
    scaled = [a / ref.SCALE for a in (w1, b1, w2, b2)]
    u = ref.unpack(ref.pack(scaled[0], scaled[1], scaled[2], scaled[3], w3, b3, "fp32"), "fp32")
    value = lambda name: ref.bf16_value(u[name]).astype(np.float64) + ref.bf16_value(u[name + "l"]).astype(np.float64)
    assert np.array_equal(np.rint(value("w1")[:, :obs_dim]), w1) and np.array_equal(np.rint(value("w1")[:, 31]), b1)
    assert np.array_equal(np.rint(value("w2")), w2)
    assert np.array_equal(value("w3")[:out_dim], w3)  # (layer 3 is not scaled: small integers are exact in bf16)
    assert np.array_equal(np.rint(u["b2"]), b2) and np.array_equal(u["b3"][:out_dim], b3)


@pytest.mark.parametrize("obs_dim,out_dim", ref.SHAPES)
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_unpacked_halves_are_the_rounded_weights_and_padding_is_zero(obs_dim, out_dim, precision):
    W = ref.weights_b(obs_dim, out_dim)
    v1, v2, v3 = ref.tables(*W)
    blob = ref.pack(*W, precision=precision)
    assert blob.size == (332800 if precision == "fp32" else 168960)
    u = ref.unpack(blob, precision)
    fold = np.float32(1.0 if precision == "fp32" else -2.0)
    assert np.array_equal(u["w1"], ref.bf16(v1)) and np.array_equal(u["w2"], ref.bf16(fold * v2)) and np.array_equal(u["w3"], ref.bf16(fold * v3))
    # padding: k in [obs_dim, 31) of layer 1 and the rows >= out_dim of layer 3 (weights and bias) are zero
    assert not ref.bf16_value(u["w1"][:, obs_dim:31]).any() and not ref.bf16_value(u["w3"][out_dim:]).any() and not u["b3"][out_dim:].any()
    if precision == "fp32":
        assert not u["w1l"][:, obs_dim:31].any() and not u["w3l"][out_dim:].any()
        for name, v in (("w1", v1), ("w2", v2), ("w3", v3)):
            got = ref.bf16_value(u[name]).astype(np.float64) + ref.bf16_value(u[name + "l"]).astype(np.float64)
            v = v.astype(np.float64)
            normal = np.abs(v) >= 2.0 ** -100  # (below, the low half is a float32 subnormal with fewer bits)
            assert np.all(np.abs(got - v)[normal] <= 2.0 ** -16 * np.abs(v)[normal])
            assert np.all(np.abs(got - v)[~normal] <= 2.0 ** -126)
        assert np.array_equal(u["b2"], ref.SCALE * W[3]) and np.array_equal(u["b3"][:out_dim], W[5])
    else:
        want = (ref.SCALE * W[3]).astype(np.float64) + ref.bf16_value(ref.bf16(v2)).astype(np.float64).sum(1)
        assert np.allclose(u["b2"], want, rtol=1e-5, atol=1e-30)


def test_weight_set_b_holds_what_it_promises():
    for obs_dim, out_dim in ref.SHAPES:
        W = ref.weights_b(obs_dim, out_dim)
        v1, v2, v3 = ref.tables(*W)
        for i, (w, stored) in enumerate(zip(W, (v1[:, :obs_dim], v1[:, 31], v2, ref.SCALE * W[3], W[4], W[5]))):
            if w.size < 24:
                continue  # (b3 of the value branch is one number)
            bits = np.ascontiguousarray(stored).view(np.uint32).reshape(-1)
            tie = (bits & 0xFFFF) == 0x8000
            assert (tie & ((bits >> 16) & 1 == 0)).any() and (tie & ((bits >> 16) & 1 == 1)).any(), i   # rounds down / up to even
            assert (((bits & 0xFFFF) == 0) & (bits << 1 != 0)).any(), i                                   # a zero low half
            wb = w.view(np.uint32).reshape(-1)
            assert (wb == 0).any() and (wb == 0x80000000).any(), i                                        # +0 and -0
            assert ((wb & 0x7F800000 == 0) & (wb << 1 != 0)).any(), i                                      # a float32 subnormal
            assert (w > 0).any() and (w < 0).any() and np.isfinite(w).all()
            mag = np.abs(w[w != 0])
            assert mag.min() <= 1e-30 and mag.max() >= 1e4


def test_adam_inputs_separate_float32_from_float64():
    """The ratio test of tests/test_gpu_mlp_update.py needs d_torch > 0: torch.optim.Adam in float32 on the CPU is not the float64
    rule to the last bit on these inputs - except for the tensor whose gradient is zero, which does not move at all."""
    d = adam_reference(31, 26)["d_torch"]
    for i in range(6):
        for what in ("p", "exp_avg", "exp_avg_sq"):
            assert (d[what][i] == 0.0) == (i == ref.ADAM_ZERO_TENSOR), (i, what, d[what][i])


_ADAM = {}


def adam_reference(obs_dim, out_dim):
    """ADAM_STEPS steps of the policy branch from default init (seed 0) on ``ref.adam_grads``: the float64 rule and torch.optim.Adam
    (float32, CPU, foreach=False).  Computed once per shape and shared: {"start", "p64", "m64", "v64", "torch": (p, m, v), "d_torch"}."""
    key = (obs_dim, out_dim)
    if key in _ADAM:
        return _ADAM[key]
    import torch

    from skyjo_rl_amd.action_mask_model import ActionMaskModel

    torch.manual_seed(0)
    seq = ActionMaskModel(obs_dim=obs_dim, num_outputs=out_dim).policy
    params = list(seq.parameters())
    start = [p.detach().numpy().copy() for p in params]
    shapes = [p.shape for p in start]
    p64 = [p.astype(np.float64) for p in start]
    m64, v64 = [np.zeros_like(p) for p in p64], [np.zeros_like(p) for p in p64]
    opt = torch.optim.Adam(params, foreach=False, **ref.ADAM_HYPER)
    for t in range(1, ref.ADAM_STEPS + 1):
        grads = ref.adam_grads(shapes, t)
        for i, g in enumerate(grads):
            p64[i], m64[i], v64[i] = ref.adam_ref(p64[i], g, m64[i], v64[i], t=t, **ref.ADAM_HYPER)
            params[i].grad = torch.from_numpy(g.copy())
        opt.step()
    tp = [p.detach().numpy() for p in params]
    tm = [opt.state[p]["exp_avg"].numpy() for p in params]
    tv = [opt.state[p]["exp_avg_sq"].numpy() for p in params]
    dist = lambda a, b: [float(np.abs(x.astype(np.float64) - y).max()) for x, y in zip(a, b)]
    _ADAM[key] = {"start": start, "p64": p64, "m64": m64, "v64": v64, "torch": (tp, tm, tv),
                  "d_torch": {"p": dist(tp, p64), "exp_avg": dist(tm, m64), "exp_avg_sq": dist(tv, v64)}}
    return _ADAM[key]


def test_abi_has_the_in_place_update():
    """include/skyjo_vec.h declares the four entry points (and the state size), the library exports them, the ctypes table has them."""
    from skyjo_rl_amd import _lib, build

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "skyjo_vec.h")).read(), flags=re.S)
    lib = ctypes.CDLL(build.build())
    for name, res, nargs in (("skyjo_vec_mlp_update", "int", 8), ("skyjo_vec_mlp_adam_step", "int", 11), ("skyjo_vec_mlp_adam_state_bytes", "int64_t", 1),
                             ("skyjo_vec_mlp_packed_bytes", "int64_t", 1), ("skyjo_vec_mlp_export", "int", 4)):
        assert re.search(r"\b%s\s+%s\s*\(" % (res, name), text), name
        assert hasattr(lib, name), name
        r, args = _lib.SIGNATURES[name]
        assert r is (ctypes.c_int if res == "int" else ctypes.c_int64) and len(args) == nargs
    args = _lib.SIGNATURES["skyjo_vec_mlp_adam_step"][1]
    assert all(a is ctypes.c_float for a in args[5:9]) and args[4] is ctypes.c_int64 and args[9] is ctypes.c_int64
