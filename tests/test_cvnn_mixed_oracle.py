"""The oracle's explicit-precision restatement of the network step (oracle/cvnn_mixed.py), which
pins the MFMA kernels of csrc/cvnn_mfma.hip, checked on CPU:

* with f32 operands it equals torch autograd of ``_torch_step``'s loss (reference
  gbm_trainer.py:819-835) on the same model — the real-GEMM form of the complex layers
  ([[A, -B], [B, A]] blocks, dA / dB recombination, bias gradients) is the reference's math;
* the bf16 rounding is torch's ``float.bfloat16()`` (round to nearest even), and the bf16 step
  stays within bf16 precision of the f32 one.
"""

from __future__ import annotations

import numpy as np
import pytest
import torch

from oracle.cvnn_mixed import adam_reference, bf16_round, cvnn_step
from spectralmc_amd.cvnn import ComplexLinear, ComplexSequential, modReLU, zReLU
from spectralmc_amd.net import lower
from tests.helpers import make_test_cvnn


def layer_table(model) -> list[tuple[int, ...]]:
    params = list(model.parameters())
    return [(t.in_features, t.out_features, t.activation, t.w_re, t.w_im, t.b_re, t.b_im, t.act_bias)
            for t in lower(model, params)]


def flat_params(model) -> np.ndarray:
    return torch.cat([p.detach().reshape(-1) for p in model.parameters()]).numpy().astype(np.float32)


def torch_grads(model, x: torch.Tensor, targets: torch.Tensor) -> tuple[float, np.ndarray]:
    model.zero_grad(set_to_none=True)
    pr, pi = model(x, torch.zeros_like(x))
    loss = torch.nn.functional.mse_loss(pr, targets.real) + torch.nn.functional.mse_loss(pi, targets.imag)
    loss.backward()
    return float(loss), torch.cat([p.grad.reshape(-1) for p in model.parameters()]).double().numpy()


def zrelu_model(n_in: int, n_out: int) -> torch.nn.Module:
    torch.manual_seed(5)
    return ComplexSequential(ComplexLinear(n_in, 24), zReLU(), ComplexLinear(24, 40), modReLU(40),
                             ComplexLinear(40, n_out))


def inputs(B: int, n_in: int, n_out: int, seed: int = 3) -> tuple[torch.Tensor, torch.Tensor]:
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((B, n_in), generator=g) * 2 - 1
    t = torch.complex(torch.randn((B, n_out), generator=g), torch.randn((B, n_out), generator=g))
    return x, t


@pytest.mark.parametrize("arch", ["c2", "c1", "zrelu"])
def test_f32_restatement_equals_torch_autograd(arch) -> None:
    if arch == "zrelu":
        model, n_in, n_out = zrelu_model(6, 64), 6, 64
    else:
        n_in, n_out = 6, 256
        model = make_test_cvnn(n_inputs=n_in, n_outputs=n_out, seed=123, dtype=torch.float32, device="cpu",
                               hidden_layers=2 if arch == "c2" else 1)
    # modest input scale so that every modReLU / zReLU region is populated
    x, t = inputs(96, n_in, n_out)
    loss_t, g_t = torch_grads(model, x, t)
    loss_o, g_o = cvnn_step(layer_table(model), flat_params(model), x.numpy(), None, t.numpy(), operand="f32")
    assert loss_o == pytest.approx(loss_t, rel=1e-6)
    assert np.linalg.norm(g_o - g_t) / np.linalg.norm(g_t) < 2e-6
    for name, (a, b) in {"max": (np.abs(g_o - g_t).max(), 1e-5 * np.abs(g_t).max())}.items():
        assert a <= b, name


def featured_model() -> torch.nn.Module:
    """Every table feature at once: bias-free layers (-1 offsets), in_features != 6, a zReLU layer, a last-layer
    modReLU, and non-zero ordinary and modReLU biases of both signs (the constructors zero them all)."""
    torch.manual_seed(9)
    model = ComplexSequential(ComplexLinear(5, 24, bias=False), zReLU(), ComplexLinear(24, 40), modReLU(40),
                              ComplexLinear(40, 17, bias=False), modReLU(17))
    g = torch.Generator().manual_seed(10)
    with torch.no_grad():
        for mod in model.modules():
            if isinstance(mod, ComplexLinear) and mod.real_bias is not None:
                mod.real_bias.copy_(torch.randn(mod.real_bias.shape, generator=g) * 0.1)
                mod.imag_bias.copy_(torch.randn(mod.imag_bias.shape, generator=g) * 0.1)
            if isinstance(mod, modReLU):
                mod.bias.copy_(torch.randn(mod.bias.shape, generator=g) * 0.5)
    return model


def featured_case(dtype: torch.dtype):
    model = featured_model().to(dtype)
    g = torch.Generator().manual_seed(4)
    B, n_in, n_out = 37, 5, 17
    x_re = (torch.rand((B, n_in), generator=g) * 2 - 1).to(dtype)
    x_im = (torch.rand((B, n_in), generator=g) * 2 - 1).to(dtype)
    t = torch.complex(torch.randn((B, n_out), generator=g), torch.randn((B, n_out), generator=g))
    t = t.to(torch.complex128 if dtype == torch.float64 else torch.complex64)
    model.zero_grad(set_to_none=True)
    pr, pi = model(x_re, x_im)
    loss = torch.nn.functional.mse_loss(pr, t.real) + torch.nn.functional.mse_loss(pi, t.imag)
    loss.backward()
    flat = torch.cat([p.detach().reshape(-1) for p in model.parameters()]).numpy()
    grads = torch.cat([p.grad.reshape(-1) for p in model.parameters()]).double().numpy()
    sizes = [p.numel() for p in model.parameters()]
    return layer_table(model), flat, x_re.numpy(), x_im.numpy(), t.numpy(), float(loss), grads, sizes


def test_featured_model_populates_every_branch() -> None:
    table, p, x_re, x_im, t, _, g, sizes = featured_case(torch.float64)
    assert [row[5] for row in table] == [-1, table[1][5], -1] and table[1][5] >= 0  # b_re: absent, present, absent
    assert [row[2] for row in table] == [2, 1, 1]
    for row in table:
        if row[2] == 1:
            c = p[row[7]:row[7] + row[1]]
            assert (c > 0).any() and (c < 0).any()
    assert np.abs(x_im).min() > 0
    assert all(np.abs(g[o:o + k]).max() > 0 for o, k in zip(np.cumsum([0] + sizes[:-1]), sizes))


def test_f64_reference_equals_torch_float64_autograd() -> None:
    """operand="f64", the reference that judges the kernels: loss within 1e-12 rel, every gradient element within
    1e-10 of its parameter group's largest magnitude."""
    table, p, x_re, x_im, t, loss_t, g_t, sizes = featured_case(torch.float64)
    assert p.dtype == np.float64
    loss_o, g_o = cvnn_step(table, p, x_re, x_im, t, operand="f64")
    assert g_o.dtype == np.float64
    assert loss_o == pytest.approx(loss_t, rel=1e-12)
    off = 0
    for k in sizes:
        sl = slice(off, off + k)
        assert np.abs(g_o[sl] - g_t[sl]).max() <= 1e-10 * np.abs(g_t[sl]).max(), off
        off += k


def test_f32_restatement_equals_torch_autograd_on_the_featured_model() -> None:
    table, p, x_re, x_im, t, loss_t, g_t, _ = featured_case(torch.float32)
    loss_o, g_o = cvnn_step(table, p, x_re, x_im, t, operand="f32")
    assert g_o.dtype == np.float32
    assert loss_o == pytest.approx(loss_t, rel=1e-6)
    assert np.linalg.norm(g_o - g_t) / np.linalg.norm(g_t) < 2e-6
    assert np.abs(g_o - g_t).max() <= 1e-5 * np.abs(g_t).max()


def test_f32_accumulation_variant_is_a_reordering_only() -> None:
    """accumulate="f32" adds the same products in f32 one after the other: within f32 summation error of the
    exact sums, and not the same numbers."""
    table, p, x_re, x_im, t, _, _, _ = featured_case(torch.float32)
    for operand, tol in (("f32", 2e-6), ("bf16", 2e-2)):
        l0, g0 = cvnn_step(table, p, x_re, x_im, t, operand=operand)
        l1, g1 = cvnn_step(table, p, x_re, x_im, t, operand=operand, accumulate="f32")
        assert l1 == pytest.approx(l0, rel=tol)
        assert 0 < np.linalg.norm(g1.astype(np.float64) - g0) / np.linalg.norm(g0) < tol


@pytest.mark.parametrize("real", [np.float32, np.float64])
@pytest.mark.parametrize("weight_decay", [0.0, 0.01])
def test_adam_reference_equals_torch_adam(real, weight_decay) -> None:
    """adam_reference against torch.optim.Adam in float64 over three steps from non-zero state.  With
    real=float32 the bias corrections alone are f32, which moves the update by at most the f32 rounding of
    1 - b2^t relative to itself (2^-24 / (1 - b2) at t = 1, halved by the square root)."""
    rng = np.random.default_rng(0)
    n = 257
    p = rng.standard_normal(n)
    m = np.zeros(n)
    v = np.zeros(n)
    tp = torch.tensor(p, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([tp], lr=1e-2, weight_decay=weight_decay)
    step = 0.0
    lr, b1, b2, eps = 1e-2, 0.9, 0.999, 1e-8
    for _ in range(3):
        g = rng.standard_normal(n) * 10.0 ** rng.uniform(-4, 1, n)
        tp.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        p_old = p
        p, m, v, gn, step = adam_reference(p, m, v, g, step, lr, b1, b2, eps, weight_decay, real)
        assert gn == pytest.approx(np.linalg.norm(g), rel=1e-14)
        st = opt.state[tp]
        if real is np.float64:
            np.testing.assert_allclose(p, tp.detach().numpy(), rtol=1e-13, atol=0)
            np.testing.assert_allclose(m, st["exp_avg"].numpy(), rtol=1e-13, atol=1e-300)
            np.testing.assert_allclose(v, st["exp_avg_sq"].numpy(), rtol=1e-13, atol=0)
        else:
            # f32 hyper-parameters (0.9f, 0.999f, 0.01f) and f32 bias corrections: 1 - 0.999f^t is off by up
            # to 2^-24 + t * 2^-25 in 1e-3 t, the rest by f32 roundings of the constants
            d, dt = p - p_old, tp.detach().numpy() - p_old
            assert np.abs(d - dt).max() <= 2e-4 * np.abs(dt).max()
    assert step == 3.0


@pytest.mark.parametrize("mutant", ["no_k_term", "dc_counts_dead_units", "imaginary_input_dropped"])
def test_kernel_test_bounds_reject_wrong_gradients(mutant, monkeypatch) -> None:
    """The f32 bound of tests/test_gpu_cvnn_kernels.py (8 x the CPU f32 error per group, floor 2^-21) applied, on
    the CPU, to f32 restatements made wrong the way a kernel could be — modReLU's backward without its
    ``k = -dot c / m^3`` term, its bias gradient summed over dead units too, the imaginary input read as zero:
    each leaves groups outside their bounds, which the zero-bias, real-input cases never could show."""
    import oracle.cvnn_mixed as restatement
    from tests import test_gpu_cvnn_kernels as kernels

    ref = kernels.reference("mixed_333")
    x_im = ref.x_im
    orig = restatement._act_bwd

    def wrong_bwd(act, c, u, v, gr, gi):
        gu, gv, dc = orig(act, c, u, v, gr, gi)
        if act != restatement.ACT_MODRELU:
            return gu, gv, dc
        m = np.sqrt(u * u + v * v + np.float32(1e-9))
        if mutant == "no_k_term":
            on = m + c > 0
            return np.where(on, gr * (m + c) / m, 0), np.where(on, gi * (m + c) / m, 0), dc
        return gu, gv, (gr * u + gi * v) / m

    if mutant == "imaginary_input_dropped":
        x_im = None
    else:
        monkeypatch.setattr(restatement, "_act_bwd", wrong_bwd)
    _, g = cvnn_step(ref.table, ref.params0, ref.x_re, x_im, ref.t, operand="f32")
    outside = [(kind, l) for (kind, l, off, k), e in zip(ref.groups, ref.e_cpu)
               if kernels.group_err(g, ref.g, off, k) > kernels.F32_FACTOR * max(e, kernels.F32_FLOOR)]
    assert outside, mutant
    if mutant == "dc_counts_dead_units":
        assert {kind for kind, _ in outside} == {"modrelu_biases"}


def test_bf16_rounding_is_torch_round_to_nearest_even() -> None:
    g = torch.Generator().manual_seed(0)
    x = torch.cat([torch.randn(4096, generator=g) * 10.0 ** torch.randint(-30, 30, (4096,), generator=g),
                   torch.tensor([0.0, -0.0, 1.0, 1.00390625, 1.005859375, 3.0e38, -3.0e38, 1e-40])])
    want = x.bfloat16().float().numpy()
    np.testing.assert_array_equal(bf16_round(x.numpy()), want)


def test_bf16_step_within_bf16_precision_of_f32() -> None:
    model = make_test_cvnn(n_inputs=6, n_outputs=256, seed=123, dtype=torch.float32, device="cpu", hidden_layers=2)
    x, t = inputs(128, 6, 256)
    table, p = layer_table(model), flat_params(model)
    l32, g32 = cvnn_step(table, p, x.numpy(), None, t.numpy(), operand="f32")
    l16, g16 = cvnn_step(table, p, x.numpy(), None, t.numpy(), operand="bf16")
    assert l16 == pytest.approx(l32, rel=2e-2)
    assert np.linalg.norm(g16 - g32) / np.linalg.norm(g32) < 3e-2
    assert not np.array_equal(g16, g32)
