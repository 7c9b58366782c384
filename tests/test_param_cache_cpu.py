"""ptt_amd.param_cache on the CPU: when a ParamCache rebuilds and when ops.param_generation moves, the conv + BatchNorm fold
against its formula (bitwise) and against the stock eval-mode unit (float64), and the shared index tables."""
import pytest
import torch
import torch.nn as nn

from ptt_amd import ops
from ptt_amd.models.backbones_3d.pointnet2 import pytorch_utils as pt_utils
from ptt_amd.param_cache import FoldedLayer, ParamCache, fold_conv_bn, index_table

CPU = torch.device('cpu')


def _counted(cache, tensors, device=CPU):
    """-> (value, builds, generations moved) of one cache.get."""
    calls = []
    g0 = ops.param_generation
    value = cache.get(tensors, device, lambda: calls.append(1) or object())
    return value, len(calls), ops.param_generation - g0


def test_param_cache_rebuilds_once_per_change_and_not_otherwise():
    a, b = torch.zeros(4), torch.ones(3)
    cache = ParamCache()
    assert not cache.held()
    v0, builds, moved = _counted(cache, [a, b])
    assert (builds, moved) == (1, 1) and cache.held()
    v1, builds, moved = _counted(cache, [a, b])                 # a repeated get: nothing is built, nothing moves
    assert (builds, moved) == (0, 0) and v1 is v0

    b.add_(0.0)                                                 # an in-place write: the version counter moves
    v2, builds, moved = _counted(cache, [a, b])
    assert (builds, moved) == (1, 1) and v2 is not v1
    assert _counted(cache, [a, b])[1:] == (0, 0)

    version = a._version
    a.data = a.data.clone()                                     # new storage, same version
    assert a._version == version
    v3, builds, moved = _counted(cache, [a, b])
    assert (builds, moved) == (1, 1) and v3 is not v2
    assert _counted(cache, [a, b])[1:] == (0, 0)

    v4, builds, moved = _counted(cache, [a, b], torch.device('meta'))      # asked for another device
    assert (builds, moved) == (1, 1) and v4 is not v3
    assert _counted(cache, [a, b], torch.device('meta'))[1:] == (0, 0)


def test_param_cache_builds_without_autograd():
    w = torch.ones(3, requires_grad=True)
    assert not ParamCache().get([w], CPU, lambda: w * 2).requires_grad


def test_param_cache_drop_moves_the_generation_only_when_an_entry_was_held():
    cache = ParamCache()
    g0 = ops.param_generation
    cache.drop()
    assert ops.param_generation == g0
    cache.get([torch.zeros(1)], CPU, lambda: 1)
    g1 = ops.param_generation
    assert g1 == g0 + 1
    cache.drop()
    assert ops.param_generation == g1 + 1 and not cache.held()
    cache.drop()
    assert ops.param_generation == g1 + 1


def test_param_cache_is_not_part_of_the_state_dict():
    seq = pt_utils.Seq(4).conv1d(8, bn=True)
    assert all('cache' not in k for k in seq.state_dict())
    assert [n for n, _ in seq.named_modules() if 'cache' in n] == []


def test_folded_layer_field_order_is_what_the_ops_entry_points_unpack():
    assert FoldedLayer._fields == ('wpacked', 'scale', 'shift', 'cin', 'cout', 'relu')


def _unit(kind, cin=8, cout=16, seed=0):
    """One Conv2d unit of pytorch_utils with non-trivial BatchNorm statistics."""
    torch.manual_seed(seed)
    bn = kind.startswith('bn')
    unit = pt_utils.Conv2d(cin, cout, bn=bn, bias=(kind == 'bias'))
    if kind == 'bn+bias':                                       # the builders never make it; a loaded module may
        unit.conv = nn.Conv2d(cin, cout, kernel_size=1, bias=True)
    with torch.no_grad():
        if unit.conv.bias is not None:
            unit.conv.bias.uniform_(-0.5, 0.5)
        if bn:
            b = unit.normlayer.bn
            b.weight.uniform_(0.5, 1.5)
            b.bias.normal_(0, 0.3)
            b.running_mean.normal_(0, 0.5)
            b.running_var.uniform_(0.3, 2.0)
    return unit.eval()


@pytest.mark.parametrize("kind", ["bn+bias", "bn", "bias", "none"])
def test_fold_conv_bn_is_the_formula_bit_for_bit(kind):
    unit = _unit(kind)
    with torch.no_grad():
        scale, shift = fold_conv_bn(unit)
        bias = unit.conv.bias
        if kind.startswith('bn'):
            bn = unit.normlayer.bn
            want_scale = (bn.weight / torch.sqrt(bn.running_var + bn.eps)).float().contiguous()
            want_shift = (bn.bias - bn.running_mean * want_scale).float().contiguous()
            if bias is not None:
                want_shift = (want_shift + bias * want_scale).contiguous()
        else:
            want_scale, want_shift = None, (None if bias is None else bias.detach().float().contiguous())
    for got, want in ((scale, want_scale), (shift, want_shift)):
        if want is None:
            assert got is None
        else:
            assert got.dtype == torch.float32 and got.is_contiguous() and not got.requires_grad
            assert torch.equal(got, want)


@pytest.mark.parametrize("kind", ["bn+bias", "bn", "bias", "none"])
def test_fold_conv_bn_matches_the_stock_eval_unit_in_float64(kind):
    """conv(x) * scale + shift against the unit itself, both in float64. Both sides start from the same convolution output
    y = W x (the same rounded number); the unit then takes ((y + b) - mean) / sqrt(var + eps) * gamma + beta, the fold
    y * scale + shift: a handful of roundings each, every one relative to an intermediate no larger than
    m = (|y| + |b| + |mean|) * |scale| + |beta|. The bound is eps(float64) * K * max(m), K the reduction length of the
    convolution (8 here: 'a few ulps')."""
    cin = 8
    unit = _unit(kind, cin=cin).double()
    x = torch.randn(2, cin, 5, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        scale, shift = fold_conv_bn(unit, dtype=torch.float64)
        y = nn.functional.conv2d(x, unit.conv.weight)
        got = y
        if scale is not None:
            got = got * scale.view(1, -1, 1, 1)
        if shift is not None:
            got = got + shift.view(1, -1, 1, 1)
        ref = nn.Sequential(*[m for n, m in unit.named_children() if n != 'activation'])(x)
        zero = torch.zeros(unit.conv.weight.shape[0], dtype=torch.float64)
        b = unit.conv.bias.abs() if unit.conv.bias is not None else zero
        bn = unit.normlayer.bn if hasattr(unit, 'normlayer') else None
        mean, beta = (bn.running_mean.abs(), bn.bias.abs()) if bn is not None else (zero, zero)
        s = scale.abs() if scale is not None else zero + 1
        m = (y.abs() + (b + mean).view(1, -1, 1, 1)) * s.view(1, -1, 1, 1) + beta.view(1, -1, 1, 1)
    tol = torch.finfo(torch.float64).eps * cin * float(m.max())
    err = float((got - ref).abs().max())
    print("fold_conv_bn[%s]: max |fold - unit| = %.3g, bound %.3g" % (kind, err, tol))
    assert err <= tol


def test_index_table_is_built_once_per_shape_and_moves_no_generation():
    g0 = ops.param_generation
    t = index_table(3, 5, CPU, torch.int64)
    assert t.dtype == torch.int64 and torch.equal(t, torch.arange(5).repeat(3, 1))
    assert index_table(3, 5, CPU, torch.int64) is t
    assert index_table(3, 5, CPU, torch.int32) is not t and index_table(2, 5, CPU, torch.int64) is not t
    assert index_table(3, 5, CPU, torch.int32).dtype == torch.int32
    assert ops.param_generation == g0
