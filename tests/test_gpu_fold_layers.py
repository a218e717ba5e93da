"""fold.conv_bn on MI355X: every convolution of the two voxel U-Nets with its eval-mode BatchNorm
(+ residual) (+ ReLU) folded into the store (include/pcs_fold.h; the EpiAffine epilogue of
csrc/conv3d.hip).  Build-defined, not reference parity.

For every conv kind, relu in {0, 1}, residual in {None, given} and out_dtype in {bf16, fp32}:
  1. bit identity: conv_bn(...) has the bit pattern of bn.eval()(conv(..., out_dtype=fp32), residual=...,
     out_dtype=out_dtype), the existing convolution with an fp32 output followed by the existing eval
     apply pass (no tolerance; NaNs count);
  2. against fp64: F.conv3d / conv_transpose3d (dense) or the numpy statements of oracle/sparse_oracle.py
     and tests/sparse_stride_refs.py (sparse), then scale * y + shift (+ R), then ReLU, all in fp64;
     max|a - b| / max|b| < 1e-5 with an fp32 output (tests/test_gpu_sparse.py's bound for these
     convolutions) and < 2^-8 with a bf16 output (one bf16 rounding is at most 2^-9 of the element, which
     is at most max|b|; doubled);
  3. the unfused bf16 output of the convolution on the same inputs is torch.equal before and after.
Sparse: grid 16, 2 scenes, occupancy 0.3 (V is no multiple of 64), on the pair-list and on the tile-gather
route, selected as tests/test_gpu_sparse.py selects them.  Dense: 2 x 6 x 6 x 10 for the stencil (partial
4 x 4 x 8 blocks on every axis), 2 x 8 x 8 x 8 for the k = 2, s = 2 layers.  (Cin, Cout) in (32, 32),
(64, 64), (64, 128): the 32-channel tiles, 32- and 64-deep k-steps, two column blocks; the two-source
layers at CA = CB = 32 and 64.  Then NaN / inf propagation and the errors."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sparse_oracle as so
import sparse_stride_refs as sr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
BOX = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
GRID = 16
CHANNELS = [(32, 32), (64, 64), (64, 128)]
CAT_CHANNELS = [32, 64]
EPS = 1e-5

_LEVELS = {}


def _levels():
    """(sv, link) of the one sparse geometry, built once (the pair lists are cached on them)."""
    if not _LEVELS:
        from pcs_amd.data import jittered_clouds, ragged_collate
        from pcs_amd.sparse import coarsen, sparse_voxels
        from pcs_amd.voxel import voxelize
        clouds = jittered_clouds(21, 2, grid=GRID, occupancy=0.3, per_voxel=3)
        rb = ragged_collate([(torch.from_numpy(p), torch.from_numpy(l)) for p, l in clouds])
        sv = sparse_voxels(rb, voxelize(rb, GRID, *BOX), *BOX)
        svc, link = coarsen(sv)
        assert sv.num_voxels % 64 != 0 and link.coarse % 64 != 0
        _LEVELS["sv"], _LEVELS["link"] = sv, link
    return _LEVELS["sv"], _LEVELS["link"]


@pytest.fixture
def route(request, monkeypatch):
    """The form of the sparse gathers: the tile-gather kernel or the per-tap pair lists
    (tests/test_gpu_sparse.py's switch)."""
    import pcs_amd.sparse as S
    monkeypatch.setattr(S, "PAIR_TAPS_MAX", 0.0 if request.param == "gather" else 27.0)
    return request.param


def _bn(cls, c, relu, g):
    """gamma random with both signs, running_mean ~ N(0, 0.5), running_var ~ U(0.5, 2)."""
    bn = cls(c, relu=relu).to(DEV)
    with torch.no_grad():
        gamma = (0.5 + torch.rand(c, generator=g)) * (torch.randint(0, 2, (c,), generator=g) * 2 - 1)
        assert (gamma > 0).any() and (gamma < 0).any()
        bn.weight.copy_(gamma)
        bn.bias.copy_(torch.randn(c, generator=g) * 0.3)
        bn.running_mean.copy_(torch.randn(c, generator=g) * 0.5)
        bn.running_var.copy_(0.5 + 1.5 * torch.rand(c, generator=g))
    return bn


def _set_params(conv, g):
    """bf16-exact weights (the kernels read them in bf16) and a bias."""
    with torch.no_grad():
        conv.weight.copy_((torch.randn(conv.weight.shape, generator=g) * 0.05).to(torch.bfloat16).float())
        conv.bias.copy_(torch.randn(conv.bias.shape, generator=g) * 0.1)
    return conv.to(DEV)


def _dense_ref(x, w, b, stride, padding, transposed):
    xd = x.double().permute(0, 4, 1, 2, 3)
    fn = F.conv_transpose3d if transposed else F.conv3d
    return fn(xd, w.double(), b.double(), stride=stride, padding=padding).permute(0, 2, 3, 4, 1).contiguous()


def _case(kind, cin, cout, seed):
    """(conv, inputs on the device, tail of the conv's arguments, the BatchNorm class, fp64 conv output)."""
    from pcs_amd import sparse as S
    from pcs_amd import voxel as V
    from pcs_amd.sparse_norm import SparseBatchNorm
    from pcs_amd.voxel_unet import VoxelBatchNorm
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *shape: torch.randn(*shape, generator=g).to(torch.bfloat16)   # noqa: E731
    if kind in ("subm", "subm_cat", "down", "up"):
        sv, link = _levels()
        nbr = sv.nbr.cpu().numpy()
        if kind == "subm":
            conv, xs, tail = _set_params(S.SubMConv3d(cin, cout), g), [rnd(sv.num_voxels, cin)], (sv,)
            ref = so.submanifold_conv(xs[0].double().numpy(), conv.weight.detach().cpu().numpy(),
                                      conv.bias.detach().cpu().numpy(), nbr)
        elif kind == "subm_cat":
            conv, tail = _set_params(S.SubMConv3dCat(cin, cin, cout), g), (sv,)
            xs = [rnd(sv.num_voxels, cin), rnd(sv.num_voxels, cin)]
            ref = so.submanifold_conv(torch.cat(xs, 1).double().numpy(), conv.weight.detach().cpu().numpy(),
                                      conv.bias.detach().cpu().numpy(), nbr)
        elif kind == "down":
            conv, xs, tail = _set_params(S.SparseDownConv3d(cin, cout), g), [rnd(link.fine, cin)], (link,)
            ref = sr.down_conv(xs[0].double().numpy(), conv.weight.detach().cpu().numpy(),
                               conv.bias.detach().cpu().numpy(), link.child.cpu().numpy())
        else:
            conv, xs, tail = _set_params(S.SparseUpConv3d(cin, cout), g), [rnd(link.coarse, cin)], (link,)
            ref = sr.up_conv(xs[0].double().numpy(), conv.weight.detach().cpu().numpy(),
                             conv.bias.detach().cpu().numpy(), link.parent.cpu().numpy(), link.tap.cpu().numpy())
        return conv, [x.to(DEV) for x in xs], tail, SparseBatchNorm, torch.from_numpy(np.asarray(ref, np.float64))
    if kind == "conv3d_stencil":
        conv, xs = _set_params(V.Conv3d(cin, cout), g), [rnd(2, 6, 6, 10, cin)]
        ref = _dense_ref(xs[0], conv.weight.detach().cpu(), conv.bias.detach().cpu(), 1, 1, False)
    elif kind == "conv3d_down":
        conv, xs = _set_params(V.Conv3d(cin, cout, 2, 2, 0), g), [rnd(2, 8, 8, 8, cin)]
        ref = _dense_ref(xs[0], conv.weight.detach().cpu(), conv.bias.detach().cpu(), 2, 0, False)
    elif kind == "conv_transpose3d":
        conv, xs = _set_params(V.ConvTranspose3d(cin, cout), g), [rnd(2, 8, 8, 8, cin)]
        ref = _dense_ref(xs[0], conv.weight.detach().cpu(), conv.bias.detach().cpu(), 2, 0, True)
    else:
        assert kind == "conv3d_cat"
        conv, xs = _set_params(V.Conv3dCat(cin, cin, cout), g), [rnd(2, 6, 6, 10, cin), rnd(2, 6, 6, 10, cin)]
        ref = _dense_ref(torch.cat(xs, -1), conv.weight.detach().cpu(), conv.bias.detach().cpu(), 1, 1, False)
    return conv, [x.to(DEV) for x in xs], (), VoxelBatchNorm, ref


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _unfused(conv, bn, xs, tail, residual, out_dtype):
    """The existing two-kernel composition with an fp32 intermediate."""
    was = bn.training
    bn.eval()
    with torch.no_grad():
        y = bn(conv(*xs, *tail, out_dtype=torch.float32), residual=residual, out_dtype=out_dtype)
    bn.train(was)
    return y


def _check_layer(kind, cin, cout):
    from pcs_amd.fold import conv_bn
    conv, xs, tail, bn_cls, ref = _case(kind, cin, cout, seed=cin * 1000 + cout)
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        plain = conv(*xs, *tail)                                   # the unfused bf16 output, before
    assert plain.dtype == torch.bfloat16 and tuple(plain.shape) == tuple(ref.shape)
    worst = {}
    for relu in (False, True):
        bn = _bn(bn_cls, cout, relu, g)
        scale = bn.weight.detach().double().cpu() / torch.sqrt(bn.running_var.double().cpu() + EPS)
        shift = bn.bias.detach().double().cpu() - bn.running_mean.double().cpu() * scale
        for out_dtype in (torch.bfloat16, torch.float32):
            res = torch.randn(ref.shape, generator=g).to(out_dtype)
            for residual in (None, res.to(DEV)):
                bn.train()                                         # conv_bn reads the running buffers whatever the mode
                y = conv_bn(conv, bn, *xs, *tail, residual=residual, out_dtype=out_dtype)
                assert bn.training and y.dtype == out_dtype and not y.requires_grad and tuple(y.shape) == tuple(ref.shape)
                want = _unfused(conv, bn, xs, tail, residual, out_dtype)
                key = (kind, cin, cout, relu, residual is not None, out_dtype)
                assert torch.equal(_bits(y), _bits(want)), (key, int((_bits(y) != _bits(want)).sum()))
                r64 = ref * scale + shift
                if residual is not None:
                    r64 = r64 + res.double()
                if relu:
                    r64 = torch.relu(r64)
                err = float((y.double().cpu() - r64).abs().max() / r64.abs().max())
                worst[out_dtype] = max(worst.get(out_dtype, 0.0), err)
                assert err < (1e-5 if out_dtype == torch.float32 else 2.0 ** -8), (key, err)
    print(f"{kind} {cin}->{cout}: norm-relative error vs fp64: fp32 out {worst[torch.float32]:.3e}, "
          f"bf16 out {worst[torch.bfloat16]:.3e}")
    with torch.no_grad():
        assert torch.equal(conv(*xs, *tail), plain)                # ... and after


@pytest.mark.parametrize("route", ["gather", "pairs"], indirect=True)
@pytest.mark.parametrize("cin,cout", CHANNELS)
@pytest.mark.parametrize("kind", ["subm", "down"])
def test_sparse_layers(kind, cin, cout, route):
    sv, link = _levels()
    assert (sv if kind == "subm" else link).use_pairs() == (route == "pairs")
    _check_layer(kind, cin, cout)


@pytest.mark.parametrize("cin,cout", CHANNELS)
def test_sparse_up_layer(cin, cout):
    _check_layer("up", cin, cout)                                  # one pair per output row: pcs_sparse_conv_rows_affine


@pytest.mark.parametrize("route", ["gather", "pairs"], indirect=True)
@pytest.mark.parametrize("c", CAT_CHANNELS)
def test_sparse_two_source_layer(c, route):
    assert _levels()[0].use_pairs() == (route == "pairs")
    _check_layer("subm_cat", c, c)                                 # 32: no two-source path, torch.cat + the padded layer


@pytest.mark.parametrize("cin,cout", CHANNELS)
@pytest.mark.parametrize("kind", ["conv3d_stencil", "conv3d_down", "conv_transpose3d"])
def test_dense_layers(kind, cin, cout):
    _check_layer(kind, cin, cout)


@pytest.mark.parametrize("c", [16] + CAT_CHANNELS)
def test_dense_two_source_layer(c):
    _check_layer("conv3d_cat", c, c)                               # 16: no two-source path, torch.cat + the padded layer


@pytest.mark.parametrize("route", ["gather", "pairs"], indirect=True)
@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float32])
def test_nan_and_inf_propagate_as_in_the_composition(out_dtype, route):
    """One input element NaN and one inf (SubMConv3d 64 -> 64, ReLU, a residual): the output has the
    composition's bit pattern, NaN / inf sit in rows that read a poisoned voxel and nowhere else, and every
    other row is finite and identical to the clean run."""
    from pcs_amd.fold import conv_bn
    from pcs_amd.sparse_norm import SparseBatchNorm
    conv, xs, tail, _, _ = _case("subm", 64, 64, seed=3)
    sv = tail[0]
    g = torch.Generator().manual_seed(11)
    bn = _bn(SparseBatchNorm, 64, True, g)
    res = torch.randn(sv.num_voxels, 64, generator=g).to(out_dtype).to(DEV)
    clean = conv_bn(conv, bn, xs[0], sv, residual=res, out_dtype=out_dtype)
    assert torch.isfinite(clean).all()
    r_nan, r_inf = 5, sv.num_voxels - 7
    x = xs[0].clone()
    x[r_nan, 3], x[r_inf, 40] = float("nan"), float("inf")
    y = conv_bn(conv, bn, x, sv, residual=res, out_dtype=out_dtype)
    want = _unfused(conv, bn, [x], tail, res, out_dtype)
    assert torch.equal(_bits(y), _bits(want))
    touched = ((sv.nbr == r_nan) | (sv.nbr == r_inf)).any(1)
    assert touched[r_nan] and touched[r_inf] and not touched.all()
    assert torch.isnan(y[r_nan]).all()                             # NaN times any weight, through the ReLU
    assert not torch.isfinite(y[r_inf]).all() and torch.isfinite(y[~touched]).all()
    assert torch.equal(torch.isnan(y), torch.isnan(want)) and torch.equal(torch.isinf(y), torch.isinf(want))
    assert torch.equal(_bits(y[~touched]), _bits(clean[~touched]))


def test_nan_propagates_through_the_dense_stencil():
    from pcs_amd.fold import conv_bn
    from pcs_amd.voxel_unet import VoxelBatchNorm
    conv, xs, tail, _, _ = _case("conv3d_stencil", 64, 64, seed=4)
    g = torch.Generator().manual_seed(12)
    bn = _bn(VoxelBatchNorm, 64, True, g)
    res = torch.randn(2, 6, 6, 10, 64, generator=g).to(torch.bfloat16).to(DEV)
    clean = conv_bn(conv, bn, xs[0], residual=res)
    x = xs[0].clone()
    x[0, 0, 0, 0, 5], x[1, 5, 5, 9, 60] = float("nan"), float("inf")
    y = conv_bn(conv, bn, x, residual=res)
    want = _unfused(conv, bn, [x], tail, res, torch.bfloat16)
    assert torch.equal(_bits(y), _bits(want))
    touched = torch.zeros(2, 6, 6, 10, dtype=torch.bool, device=DEV)
    touched[0, :2, :2, :2] = True
    touched[1, 4:, 4:, 8:] = True
    assert torch.isnan(y[0, 0, 0, 0]).all() and torch.isnan(y[0, 1, 1, 1]).all()
    assert not torch.isfinite(y[1, 5, 5, 9]).all() and torch.isfinite(y[~touched]).all()
    assert torch.equal(_bits(y[~touched]), _bits(clean[~touched]))


def test_errors():
    from pcs_amd.fold import conv_bn
    from pcs_amd.sparse import SubMConv3d
    from pcs_amd.sparse_norm import SparseBatchNorm
    from pcs_amd.voxel import Conv3d
    from pcs_amd.voxel_unet import VoxelBatchNorm
    sv, link = _levels()
    V = sv.num_voxels
    conv, bn = SubMConv3d(64, 64).to(DEV), SparseBatchNorm(64, relu=True).to(DEV)
    x = torch.randn(V, 64, device=DEV).to(torch.bfloat16)
    assert not conv_bn(conv, bn, x, sv).requires_grad              # the parameters require grad; the output never does
    with pytest.raises(RuntimeError, match="inference only"):
        conv_bn(conv, bn, x.clone().requires_grad_(), sv)
    with pytest.raises(RuntimeError, match="inference only"):
        conv_bn(conv, bn, x, sv, residual=x.clone().requires_grad_())
    with torch.no_grad():                                          # no graph is asked for
        assert not conv_bn(conv, bn, x.clone().requires_grad_(), sv).requires_grad
    with pytest.raises(ValueError, match="residual"):
        conv_bn(conv, bn, x, sv, residual=x.float())               # not in out_dtype
    with pytest.raises(ValueError, match="residual"):
        conv_bn(conv, bn, x, sv, residual=x[:-1])
    with pytest.raises(ValueError, match="residual"):
        conv_bn(conv, bn, x, sv, residual=x, out_dtype=torch.float32)
    with pytest.raises(ValueError, match="128 channels, the convolution 64"):
        conv_bn(conv, SparseBatchNorm(128).to(DEV), x, sv)
    with pytest.raises(TypeError):
        conv_bn(conv, torch.nn.BatchNorm1d(64).to(DEV), x, sv)
    with pytest.raises(TypeError):
        conv_bn(torch.nn.Conv3d(64, 64, 3).to(DEV), bn, x, sv)
    with pytest.raises(TypeError, match="takes 2 inputs"):
        conv_bn(conv, bn, x)
    with pytest.raises(ValueError):
        conv_bn(conv, bn, x.float(), sv)
    with pytest.raises(ValueError):
        conv_bn(conv, bn, x, sv, out_dtype=torch.float16)
    dconv, dbn = Conv3d(32, 32).to(DEV), VoxelBatchNorm(32, relu=True).to(DEV)
    xd = torch.randn(1, 4, 4, 8, 32, device=DEV).to(torch.bfloat16)
    with pytest.raises(ValueError, match="residual"):
        conv_bn(dconv, dbn, xd, residual=xd.view(-1, 32))
    with pytest.raises(ValueError, match="64 channels, the convolution 32"):
        conv_bn(dconv, VoxelBatchNorm(64).to(DEV), xd)
    with pytest.raises(RuntimeError, match="inference only"):
        conv_bn(dconv, dbn, xd.clone().requires_grad_())
