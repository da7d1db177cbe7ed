"""CPU: tests/loss_ref.py against autograd of the whole function and hand-computed values, and the end-to-end bars of
tests/test_gpu_losses.py: 4 x the error of the reference implementation's own arithmetic (the restatement run in fp32 on the CPU
with autograd, held to backward_from_maps at that run's own maps), the factor and norm of DESIGN.md §9.  The bars are sharp: each
faulty restatement exceeds them on the test's own inputs."""
import functools

import pytest
import torch
import torch.nn.functional as F

import loss_ref as R

F64 = torch.float64
BARS, CPU_FP32, SEED = R.BARS, R.CPU_FP32, R.SEED
SOBEL_BARS, SOBEL_CPU_FP32, SOBEL_SEED, SOBEL_SHAPES = R.SOBEL_BARS, R.SOBEL_CPU_FP32, R.SOBEL_SEED, R.SOBEL_SHAPES


@functools.lru_cache(maxsize=None)
def case(i):
    """inputs, fp64 autograd and the fp64 chain at the fp64 maps of case i, computed once"""
    n, h, w = R.SHAPES[i]
    sd = R.synth_weights(seed=20)
    x, y, g = R.loss_inputs(n, h, w, SEED + i)
    dx, dy, fx, fy = R.autograd_images(sd, x, y, g)
    chain = R.backward_from_maps(sd, fx, fy, g, (h, w))
    return dict(sd=sd, x=x, y=y, g=g, dx=dx, dy=dy, fx=fx, fy=fy, chain=chain, hw=(h, w))


@pytest.mark.parametrize("i", range(3), ids=[str(s) for s in R.SHAPES])
def test_chain_equals_whole_function_autograd(i):
    c = case(i)
    assert float(c["dx"].abs().max()) > 0 and float(c["dy"].abs().max()) > 0
    assert float((c["chain"]["dx"] - c["dx"]).abs().max()) <= 1e-12
    assert float((c["chain"]["dy"] - c["dy"]).abs().max()) <= 1e-12
    for f in c["fx"] + c["fy"]:                                    # the condition the GPU tests assert on the device's maps
        assert 0.2 <= float((f == 0).double().mean()) <= 0.8


def test_per_layer_gradients_and_normalize():
    """g [5][N] weights the layer terms separately, and normalize=True contributes its factor 2"""
    c = case(0)
    g5 = torch.linspace(-1, 1, 10, dtype=F64).view(5, 2)
    x = ((c["x"] + 1) / 2).double().requires_grad_(True)
    _, layers, fx, fy = R.lpips_loss(c["sd"], x, (c["y"] + 1) / 2, normalize=True)
    want = torch.autograd.grad(sum((l * g).sum() for l, g in zip(layers, g5)), x)[0]
    got = R.backward_from_maps(c["sd"], fx, fy, g5, c["hw"], normalize=True)["dx"]
    assert float((got - want).abs().max()) <= 1e-12 and float(want.abs().max()) > 0
    for a, b in zip(fx, c["fx"]):                                  # 2 ((x + 1) / 2) - 1 = x up to rounding: the same maps
        assert float((a.detach() - b).abs().max()) < 1e-12


def test_unit_lin_weights_are_the_unweighted_form():
    c = case(0)
    x = c["x"].double().requires_grad_(True)
    val, _, fx, fy = R.lpips_loss(c["sd"], x, c["y"], lpips=False)
    d = (R.unit_normalize(fx[1], True) - R.unit_normalize(fy[1], True)) ** 2
    assert torch.allclose(R.tail(fx[1], fy[1], torch.ones(192, dtype=F64), True), d.sum(1).flatten(1).mean(1), rtol=1e-13, atol=0)
    want = torch.autograd.grad((val * c["g"].double()).sum(), x)[0]
    got = R.backward_from_maps(c["sd"], fx, fy, c["g"], c["hw"], lpips=False)["dx"]
    assert float((got - want).abs().max()) <= 1e-12


def test_first_maximum_in_raster_order_takes_the_pool_gradient():
    m = torch.ones(1, 1, 3, 3, dtype=F64)
    g = torch.full((1, 1, 1, 1), 2.0, dtype=F64)
    want = torch.zeros(9, dtype=F64)
    want[0] = 2.0
    assert torch.equal(R.pool_grad(m, g).reshape(-1), want)
    assert torch.equal(R.pool_grad(m, g, last=True).reshape(-1), want.flip(0))
    m = torch.tensor([[0., 1, 5, 5, 0], [2, 5, 1, 0, 5], [0, 0, 5, 5, 1], [7, 0, 0, 7, 0], [0, 7, 0, 0, 7]], dtype=F64).view(1, 1, 5, 5)
    g = torch.tensor([[1., 10], [100, 1000]], dtype=F64).view(1, 1, 2, 2)
    want = torch.zeros(5, 5, dtype=F64)
    want[0, 2] = 11.0                   # windows (0, 0) and (0, 1): both first see their 5 at (0, 2)
    want[3, 0] = 100.0                  # window (1, 0): 7 at (3, 0) before (4, 1)
    want[3, 3] = 1000.0                 # window (1, 1): 7 at (3, 3) before (4, 4)
    assert torch.equal(R.pool_grad(m, g)[0, 0], want)
    rnd = torch.rand(2, 3, 9, 11, dtype=F64)
    gp = torch.rand(2, 3, 4, 5, dtype=F64)
    assert torch.equal(R.pool_grad(rnd, gp), R.pool_grad(rnd, gp, last=True))      # without ties the two rules agree
    assert float(R.pool_grad(rnd, gp)[:, :, :, 10:].abs().max()) > 0 and float(R.pool_grad(rnd[:, :, :8], gp[:, :, :3])[:, :, 7].abs().max()) == 0


def test_row_and_column_no_window_reaches_have_zero_gradient():
    """70x146: (70 + 4 - 11) mod 4 = 3 and (146 + 4 - 11) mod 4 = 3, so image row 69 and column 145 lie in no conv1 window; relu1 is
    16x35 and the pool (3, 2) leaves its row 15 uncovered"""
    c = case(2)
    for d in (c["dx"], c["dy"], c["chain"]["dx"], c["chain"]["dy"]):
        assert float(d[:, :, 69].abs().max()) == 0 and float(d[:, :, :, 145].abs().max()) == 0
        assert float(d[:, :, 68].abs().max()) > 0 and float(d[:, :, :, 144].abs().max()) > 0
    assert tuple(c["fx"][0].shape[2:]) == (16, 35)
    assert float(c["chain"]["d_x"][0][:, :, 15].abs().max()) == float(c["chain"]["tail_x"][0][:, :, 15].abs().max()) > 0
    assert torch.equal(c["chain"]["d_x"][0][:, :, 15], c["chain"]["tail_x"][0][:, :, 15])


def test_tail_gradient_gradcheck_and_written_out_form():
    gen = torch.Generator().manual_seed(3)
    fx = torch.rand(2, 8, 2, 2, generator=gen, dtype=F64).requires_grad_(True)
    fy = torch.rand(2, 8, 2, 2, generator=gen, dtype=F64).requires_grad_(True)
    lin = torch.rand(8, generator=gen, dtype=F64)
    assert torch.autograd.gradcheck(lambda a, b: R.tail(a, b, lin, True), (fx, fy), eps=1e-6, atol=1e-8)
    g = torch.tensor([0.7, -1.3], dtype=F64)
    want = torch.autograd.grad((R.tail(fx, fy, lin, True) * g).sum(), (fx, fy))
    assert float((R.tail_grad(fx, fy, lin, g) - want[0]).abs().max()) < 1e-15
    assert float((R.tail_grad(fy, fx, lin, g) - want[1]).abs().max()) < 1e-15
    r, s = R.tail_grad_ref(fx.detach(), fy.detach(), lin, g)
    assert torch.equal(r, R.tail_grad(fx, fy, lin, g).detach()) and bool((s > 0).all())
    dead = torch.zeros(1, 8, 1, 1, dtype=F64)                      # the case NormFix exists for: a dead layer has a finite gradient
    assert float(R.tail_grad(dead, dead, lin, g[:1]).abs().max()) == 0


def test_stage_references_equal_the_chain():
    c = case(1)
    sd, b = c["sd"], c["chain"]
    convs, lins = R.params(sd)
    g = c["g"].double()
    for l in range(5):
        r, _ = R.tail_grad_ref(c["fx"][l], c["fy"][l], lins[l], g)
        assert float((r - b["tail_x"][l]).abs().max()) < 1e-15
    r, s = R.conv_dgrad_ref(b["d_x"][4], convs[4][0], 1, add=b["tail_x"][3], mapv=c["fx"][3])
    assert float((r - b["d_x"][3]).abs().max()) < 1e-15 and float(s.max()) > 0
    r, _ = R.conv_dgrad_ref(b["d_x"][1], convs[1][0], 2)
    assert torch.equal(r, b["pool_x"][0])
    r, _ = R.pool_grad_ref(b["pool_x"][1], c["fx"][1], add=b["tail_x"][1])
    assert float((r - b["d_x"][1]).abs().max()) < 1e-15
    r, _ = R.conv1_dgrad_ref(b["d_x"][0], convs[0][0], c["hw"])
    assert float((r - b["dx"]).abs().max()) < 1e-15


@pytest.mark.parametrize("i", range(3), ids=[str(s) for s in R.SHAPES])
def test_bar_is_four_times_the_fp32_cpu_figure_and_rejects_every_fault(i):
    c = case(i)
    n, h, w = R.SHAPES[i]
    bar = BARS[(n, h, w)]
    d32x, d32y, f32x, f32y = R.autograd_images(c["sd"], c["x"], c["y"], c["g"], dtype=torch.float32)
    lin = R.backward_from_maps(c["sd"], f32x, f32y, c["g"], (h, w))
    fig = max(R.relative_to_max(d32x, lin["dx"]), R.relative_to_max(d32y, lin["dy"]))
    print(f"fp32 CPU figure {n}x{h}x{w}: {fig:.3e} (table {CPU_FP32[(n, h, w)]:.1e}, bar {bar:.2e})")
    assert bar / 16 <= fig <= bar / 2                               # the table is this figure up to the CPU's own summation order
    for fault in R.FAULTS:
        bad = R.backward_from_maps(c["sd"], c["fx"], c["fy"], c["g"], (h, w), fault=fault)
        for s in ("dx", "dy"):
            assert R.relative_to_max(bad[s], c["chain"][s]) > 100 * bar, (fault, s)


# ------------------------------------------------------------------------------------------------ Sobel
def test_sobel_restatement_equals_the_formula_by_hand():
    p = torch.tensor([[0.1, -0.4, 0.9], [0.3, 0.5, -0.7], [-1.0, 0.2, 0.6]], dtype=F64)
    t = torch.tensor([[-0.2, 0.8, 0.0], [0.4, -0.6, 1.0], [0.7, -0.3, 0.1]], dtype=F64)

    def edges(img):
        v = F.pad((img + 1) / 2, (1, 1, 1, 1))
        e = torch.zeros(3, 3, dtype=F64)
        for y in range(3):
            for x in range(3):
                q = v[y:y + 3, x:x + 3]
                gx = (q[0, 2] - q[0, 0]) + 2 * (q[1, 2] - q[1, 0]) + (q[2, 2] - q[2, 0])
                gy = (q[2, 0] - q[0, 0]) + 2 * (q[2, 1] - q[0, 1]) + (q[2, 2] - q[0, 2])
                e[y, x] = (gx * gx + gy * gy + 1e-6) ** 0.5
        return e
    want = (edges(p) - edges(t)).abs()
    got = R.sobel_edge_loss(p.view(1, 1, 3, 3), t.view(1, 1, 3, 3), "none")[0, 0]
    assert float((got - want).abs().max()) < 1e-15
    assert abs(float(R.sobel_edge_loss(p.view(1, 1, 3, 3), t.view(1, 1, 3, 3), "mean")) - float(want.mean())) < 1e-15
    assert abs(float(R.sobel_edge_loss(p.view(1, 1, 3, 3), t.view(1, 1, 3, 3), "sum")) - float(want.sum())) < 1e-14
    two = R.sobel_edge_loss(torch.stack([p, t]).view(1, 2, 3, 3), torch.stack([t, t]).view(1, 2, 3, 3), "none")
    assert torch.equal(two[0, 0], got) and float(two[0, 1].abs().max()) == 0                       # per channel


def test_sobel_gradient_is_zero_for_equal_operands_and_flat_images():
    p = torch.rand(1, 2, 5, 6, dtype=F64).requires_grad_(True)
    assert float(torch.autograd.grad(R.sobel_edge_loss(p, p.detach().clone(), "sum"), p)[0].abs().max()) == 0
    flat = torch.full((1, 2, 5, 6), -1.0, dtype=F64, requires_grad=True)                           # 0 after the mapping: gx = gy = 0
    g = torch.autograd.grad(R.sobel_edge_loss(flat, torch.rand(1, 2, 5, 6, dtype=F64), "mean"), flat)[0]
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) == 0


@pytest.mark.parametrize("shape", SOBEL_SHAPES[1:], ids=[str(s) for s in SOBEL_SHAPES[1:]])
def test_sobel_bar_is_four_times_the_fp32_cpu_figure(shape):
    p, t = R.sobel_inputs(shape, SOBEL_SEED)
    p64, t64 = p.double().requires_grad_(True), t.double().requires_grad_(True)
    ref = torch.autograd.grad(R.sobel_edge_loss(p64, t64, "mean"), (p64, t64))
    p32, t32 = p.clone().requires_grad_(True), t.clone().requires_grad_(True)
    got = torch.autograd.grad(R.sobel_edge_loss(p32, t32, "mean"), (p32, t32))
    fig = max(R.relative_to_max(a, b) for a, b in zip(got, ref))
    print(f"Sobel fp32 CPU figure {shape}: {fig:.3e} (table {SOBEL_CPU_FP32[shape]:.1e})")
    assert float(ref[0].abs().max()) > 0 and SOBEL_BARS[shape] / 16 <= fig <= SOBEL_BARS[shape] / 2
    # the bar is sharp: a gradient that misses the 1/2 of the [-1, 1] -> [0, 1] mapping exceeds it
    assert R.relative_to_max(2 * ref[0], ref[0]) > 100 * SOBEL_BARS[shape]
