"""tests/grad_clip_ref.py against torch.nn.utils.clip_grad_norm_ on the CPU, and the two entry points' place in the signature table.
No GPU."""
import numpy as np
import pytest

from tests import grad_clip_ref as ref
from tests import mlp_pack_ref

F32 = np.float32


@pytest.mark.parametrize("obs_dim", sorted({d for d, _ in mlp_pack_ref.SHAPES}))
def test_norm_and_coefficient_are_torchs_in_float64(obs_dim):
    """A policy (D, 26) beside a value branch (D, 1), the twelve tensors: the norm clip_grad_norm_ returns and the gradients it leaves."""
    import torch

    grads = ref.pair_grads(obs_dim)
    want = ref.norm(grads)
    for max_norm in (0.5 * want, 2.0 * want):
        params = [torch.zeros(g.shape, dtype=torch.float64, requires_grad=True) for g in grads]
        for p, g in zip(params, grads):
            p.grad = torch.from_numpy(g).double()
        total = float(torch.nn.utils.clip_grad_norm_(params, max_norm))
        assert abs(total - want) <= 1e-12 * want
        c = ref.coef64(want, max_norm)
        assert (c < 1.0) == (max_norm < want)
        for p, g in zip(params, grads):
            np.testing.assert_allclose(p.grad.numpy(), g.astype(np.float64) * c, rtol=1e-12, atol=0.0)


def _torch_coef(norm32, max_norm):
    """clip_grad_norm_'s two lines on a float32 norm (``total_norm`` there is a float32 tensor, ``max_norm`` a Python float)."""
    import torch

    total_norm = torch.tensor(norm32, dtype=torch.float32)
    clip_coef = float(max_norm) / (total_norm + 1e-6)
    return torch.clamp(clip_coef, max=1.0).numpy()


SPECIAL = [(0.0, 1.0), (float("nan"), 1.0), (float("inf"), 1.0), (0.0, 3e38), (1e-30, 1e-30), (3.7, float("inf")), (1e30, 1e30)]
# norms just below and above max_norm, and above the point where norm + 1e-6 passes it
SPECIAL += [(float(x), m) for m in (1.0, 3.7, 40.0) for x in (np.nextafter(F32(m), F32(0)), F32(m), np.nextafter(F32(m), F32(np.inf)),
                                                               F32(F32(m) - F32(1e-6)), np.nextafter(F32(F32(m) - F32(1e-6)), F32(0)))]


def test_coef32_has_torchs_bits():
    for n, m in SPECIAL:
        got, want = ref.coef32(F32(n), m), _torch_coef(F32(n), m)
        assert (np.isnan(got) and np.isnan(want)) or ref.bits(got) == ref.bits(want), (n, m, got, want)
    assert np.isnan(ref.coef32(F32("nan"), 1.0)) and ref.coef32(F32("inf"), 1.0) == 0.0 and ref.coef32(F32(0), 1.0) == 1.0
    # a sweep: the one division max_norm / (norm + 1e-6) differs from torch's reciprocal-and-multiply in the last bit on about a
    # quarter of these
    rng = np.random.default_rng(5)
    norms = (10.0 ** rng.uniform(-3, 3, 2000)).astype(F32)
    for m in (3.7, 40.0, 0.01):
        import torch

        want = torch.clamp(m / (torch.from_numpy(norms) + 1e-6), max=1.0).numpy()
        got = np.array([ref.coef32(n, m) for n in norms], dtype=F32)
        assert got.tobytes() == want.tobytes(), m
        with np.errstate(all="ignore"):
            one_division = np.minimum(F32(m) / (norms + F32(1e-6)), F32(1.0)).astype(F32)
        assert one_division.tobytes() != want.tobytes()


def test_coef32_is_what_clip_grad_norm_multiplies_by():
    """Through the function itself: a one-element gradient x has the norm |x| exactly and leaves as x * coef, one float32 multiply."""
    import torch

    rng = np.random.default_rng(6)
    for x in (10.0 ** rng.uniform(-2, 2, 200)).astype(F32):
        p = torch.zeros((1,), dtype=torch.float32, requires_grad=True)
        p.grad = torch.tensor([x], dtype=torch.float32)
        total = torch.nn.utils.clip_grad_norm_([p], 3.7)
        assert ref.bits(total.numpy()) == ref.bits(x)
        assert ref.bits(p.grad.numpy()[0]) == ref.bits(F32(x * ref.coef32(x, 3.7))), x


def test_cases_cover_what_they_say():
    cases = ref.cases()
    assert len(cases["d_32_segments"]["views"]) == 32 and len(cases["a_pair_17"]["views"]) == 12
    starts = {(s % 4, c) for s, c in cases["b_unaligned"]["views"]}
    assert starts == {(o, c) for o in (1, 2, 3) for c in ref.UNALIGNED_COUNTS}
    assert {s % 4 for s, _ in cases["a_pair_17"]["views"][6:]} == {2}
    for name, case in cases.items():
        flat, views = case["flat"], case["views"]
        covered = np.zeros(flat.size, dtype=bool)
        for s, c in views:
            assert 0 <= s and s + c <= flat.size and not covered[s:s + c].any(), name
            covered[s:s + c] = True
        assert np.isnan(flat[~covered]).all() and (~covered).sum() >= 8, name  # the filler: a read outside a view shows
    tensors = lambda case: [case["flat"][s:s + c] for s, c in case["views"]]
    with np.errstate(all="ignore"):
        f32_sum = lambda case: sum(np.sum(np.square(t), dtype=F32) for t in tensors(case))
        assert np.isinf(f32_sum(cases["f_huge"])) and np.isfinite(F32(ref.norm(tensors(cases["f_huge"]))))
        assert f32_sum(cases["f_tiny"]) == 0.0 and F32(ref.norm(tensors(cases["f_tiny"]))) > np.finfo(F32).tiny
    assert np.isnan(ref.norm(tensors(cases["g_nan"]))) and np.isposinf(ref.norm(tensors(cases["h_inf"])))
    assert ref.norm(tensors(cases["e_zeros"])) == 0.0


def test_entry_points_are_in_the_signature_table():
    from skyjo_rl_amd import _lib

    assert len(_lib.SIGNATURES["skyjo_vec_grad_norm"][1]) == 6
    assert len(_lib.SIGNATURES["skyjo_vec_mlp_adam_step_clipped"][1]) == 12
    assert len(_lib.SIGNATURES["skyjo_vec_mlp_adam_step"][1]) == 11  # (unchanged)
