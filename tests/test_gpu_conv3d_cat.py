"""The two-source dense stencil (pcs_conv3d_cat*, pcs_amd.voxel.conv3d_cat / Conv3dCat) on MI355X:
bit-identical to the single-source layer on torch.cat([xa, xb], -1) in the output, both input
gradients, dW and db, which makes the fp64 check the claim tests/test_gpu_conv3d.py already makes
for that layer at these channel counts (the same tolerances, no new number).

Grids: (5, 6, 9) has partial 4 x 4 x 8 blocks on every axis and more than one block; (3, 2, 4) is
smaller than one block.  Channels: (32, 32, 32) a 64-channel slice straddling the sources; (64, 64,
64) whole slices; (32, 64, 64) and (64, 32, 96) the 32-channel slices of Cin = 96; (96, 32, 64) a
straddle inside the second slice and an input-gradient tile straddling dXA | dXB."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
B = 2
GRIDS = [(5, 6, 9), (3, 2, 4)]
CHANNELS = [(32, 32, 32), (64, 64, 64), (32, 64, 64), (96, 32, 64), (64, 32, 96)]


def _operands(grid, ca, cb, cout, seed=0):
    g = torch.Generator().manual_seed(seed)
    xa = torch.randn(B, *grid, ca, generator=g).to(torch.bfloat16)
    xb = torch.randn(B, *grid, cb, generator=g).to(torch.bfloat16)
    w = (torch.randn(cout, ca + cb, 3, 3, 3, generator=g) * 0.05).to(torch.bfloat16).float()   # bf16-exact fp32 master
    b = torch.randn(cout, generator=g) * 0.1
    dy = torch.randn(B, *grid, cout, generator=g).to(torch.bfloat16).float()                   # bf16-exact
    return xa, xb, w, b, dy


def _run(fn, xs, w, b, dy, out_dtype):
    """(y, input gradients, dW, db) of fn(*xs, w, b) on the device."""
    xs = [x.to(DEV).requires_grad_() for x in xs]
    wd = w.to(DEV).requires_grad_()
    bd = b.to(DEV).requires_grad_() if b is not None else None
    y = fn(*xs, wd, bd, out_dtype)
    y.backward(dy.to(DEV).to(y.dtype))
    torch.cuda.synchronize()
    return y.detach(), [x.grad for x in xs], wd.grad, None if bd is None else bd.grad


def _rel(a, b):
    return float((a.double().cpu() - b).abs().max() / b.abs().max().clamp_min(1e-30))


@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("ca,cb,cout", CHANNELS)
@pytest.mark.parametrize("grid", GRIDS)
def test_bit_identical_to_the_concatenated_layer(grid, ca, cb, cout, out_dtype, with_bias):
    import pcs_amd.voxel as V
    xa, xb, w, b, dy = _operands(grid, ca, cb, cout)
    b = b if with_bias else None
    y, (dxa, dxb), dw, db = _run(lambda a, c, w_, b_, dt: V.conv3d_cat(a, c, w_, b_, dt), [xa, xb], w, b, dy, out_dtype)
    yr, (dxr,), dwr, dbr = _run(lambda x, w_, b_, dt: V.conv3d(x, w_, b_, 1, 1, dt), [torch.cat([xa, xb], -1)], w, b, dy,
                                out_dtype)
    assert y.dtype == out_dtype and tuple(y.shape) == (B, *grid, cout)
    assert torch.equal(y, yr)
    assert dxa.dtype == torch.bfloat16 and tuple(dxa.shape) == tuple(xa.shape) and tuple(dxb.shape) == tuple(xb.shape)
    assert torch.equal(dxa, dxr[..., :ca]) and torch.equal(dxb, dxr[..., ca:])
    assert torch.equal(dw, dwr)
    if with_bias:
        assert torch.equal(db, dbr)
    assert y.abs().max() > 0 and dxa.abs().max() > 0 and dxb.abs().max() > 0 and dw.abs().max() > 0


@pytest.mark.parametrize("ca,cb,cout", CHANNELS)
def test_matches_torch_fp64(ca, cb, cout):
    """tests/test_gpu_conv3d.py's bounds for the single-source layer: 1e-5 for the fp32 output, dW and
    db (fp32 summation of exact products), 8e-3 for what is stored in bf16."""
    import pcs_amd.voxel as V
    grid = GRIDS[0]
    xa, xb, w, b, dy = _operands(grid, ca, cb, cout, seed=1)
    xr = torch.cat([xa, xb], -1).permute(0, 4, 1, 2, 3).double().requires_grad_()
    wr, br = w.double().requires_grad_(), b.double().requires_grad_()
    yr = F.conv3d(xr, wr, br, padding=1)
    yr.backward(dy.permute(0, 4, 1, 2, 3).double())
    cat = lambda a, c, w_, b_, dt: V.conv3d_cat(a, c, w_, b_, dt)   # noqa: E731
    y, (dxa, dxb), dw, db = _run(cat, [xa, xb], w, b, dy, torch.float32)
    yb = _run(cat, [xa, xb], w, b, dy, torch.bfloat16)[0]
    ref = yr.detach().permute(0, 2, 3, 4, 1)
    assert _rel(y, ref) < 1e-5
    assert _rel(yb.float(), ref) < 8e-3
    assert _rel(dw, wr.grad) < 1e-5
    assert _rel(db, br.grad) < 1e-5
    dx = torch.cat([dxa, dxb], -1).float().permute(0, 4, 1, 2, 3)
    assert _rel(dx, xr.grad) < 8e-3


def test_one_sided_gradients():
    """An input that needs no gradient gets None, and the other one's is unchanged."""
    import pcs_amd.voxel as V
    xa, xb, w, b, dy = _operands(GRIDS[0], 32, 64, 64, seed=2)
    cat = lambda a, c, w_, b_, dt: V.conv3d_cat(a, c, w_, b_, dt)   # noqa: E731
    _, (dxa, dxb), dw, _ = _run(cat, [xa, xb], w, b, dy, torch.bfloat16)
    for keep in (0, 1):
        xs = [xa.to(DEV), xb.to(DEV)]
        xs[keep].requires_grad_()
        wd = w.to(DEV).requires_grad_()
        V.conv3d_cat(xs[0], xs[1], wd, None).backward(dy.to(DEV).bfloat16())
        assert xs[1 - keep].grad is None
        assert torch.equal(xs[keep].grad, (dxa, dxb)[keep]) and torch.equal(wd.grad, dw)


def test_fallback_off_the_multiple_of_32():
    """Widths (24, 40) -> 48 have no two-source path: torch.cat + the single-source layer."""
    import pcs_amd.voxel as V
    xa, xb, w, b, dy = _operands(GRIDS[0], 24, 40, 48, seed=3)
    y, (dxa, dxb), dw, db = _run(lambda a, c, w_, b_, dt: V.conv3d_cat(a, c, w_, b_, dt), [xa, xb], w, b, dy,
                                 torch.float32)
    yr, (dxr,), dwr, dbr = _run(lambda x, w_, b_, dt: V.conv3d(x, w_, b_, 1, 1, dt), [torch.cat([xa, xb], -1)], w, b, dy,
                                torch.float32)
    assert torch.equal(y, yr) and torch.equal(dw, dwr) and torch.equal(db, dbr)
    assert torch.equal(dxa, dxr[..., :24]) and torch.equal(dxb, dxr[..., 24:])


def test_module_and_reproducibility():
    """Conv3dCat carries nn.Conv3d(ca + cb, cout, 3, padding=1)'s parameters (state dicts load into
    Conv3d(ca + cb, cout) and back), refuses other widths than its own, and two runs are bitwise equal."""
    import pcs_amd
    import pcs_amd.voxel as V
    torch.manual_seed(0)
    m = pcs_amd.Conv3dCat(32, 64, 64).to(DEV)
    ref = torch.nn.Conv3d(96, 64, 3, padding=1)
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == [(k, tuple(v.shape)) for k, v in ref.state_dict().items()]
    single = V.Conv3d(96, 64).to(DEV)
    single.load_state_dict(m.state_dict())
    m.load_state_dict(single.state_dict())
    assert V.Conv3dCat(32, 32, 32, bias=False).bias is None
    xa, xb, _, _, dy = _operands(GRIDS[0], 32, 64, 64, seed=4)
    runs = []
    for _ in range(2):
        a, c = xa.to(DEV).requires_grad_(), xb.to(DEV).requires_grad_()
        m.zero_grad(set_to_none=True)
        y = m(a, c)
        y.backward(dy.to(DEV).bfloat16())
        runs.append((y.detach().clone(), a.grad.clone(), c.grad.clone(), m.weight.grad.clone(), m.bias.grad.clone()))
    torch.cuda.synchronize()
    assert all(torch.equal(p, q) for p, q in zip(*runs))
    assert torch.equal(runs[0][0], single(torch.cat([xa, xb], -1).to(DEV)))
    with pytest.raises(ValueError, match="Conv3dCat"):
        m(xb.to(DEV), xa.to(DEV))
    with pytest.raises(ValueError, match="grid"):
        V.conv3d_cat(xa.to(DEV), xb.to(DEV)[:, :4], m.weight)
