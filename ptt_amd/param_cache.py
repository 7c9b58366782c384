"""The eval-mode parameter caches of the modules that run on the hand-written kernels: ONE implementation of the two rules a
captured graph (ops.StateWatch) relies on —
  * a cache is rebuilt when (data_ptr, _version) of a tensor it was built from moves, or when it is asked for another device;
  * every rebuild and every drop moves ops.param_generation (ops.publish_params / ops.drop_params), because the buffers a
    captured graph addresses are being replaced or freed —
plus the one conv + BatchNorm fold and the one per-shape index table.
"""
from collections import namedtuple

import torch

from . import ops

# One folded layer as ops.sa_fused_forward, ops.rows_mlp and ops.xcorr_fused unpack it. A second packing of the same layer (the
# weights without the BatchNorm scale, a rotated first layer, ...) gets a name of its own at the site that needs it.
FoldedLayer = namedtuple('FoldedLayer', 'wpacked scale shift cin cout relu')


class ParamCache(object):
    """What a module built from its parameters and buffers for the kernels, and what it was built from. A plain attribute
    of its owner: not a submodule, parameter or buffer (state_dict() keys stay the reference's)."""
    __slots__ = ('_key', '_value')

    def __init__(self):
        self._key = self._value = None

    def held(self):
        return self._key is not None

    def get(self, tensors, device, build):
        """build()'s result (called under no_grad) as of the current state of `tensors`, made for `device`."""
        key = (str(device), *[(t.data_ptr(), t._version) for t in tensors])
        if key != self._key:
            with torch.no_grad():
                value = build()
            ops.publish_params(device)
            self._key, self._value = key, value
        return self._value

    def drop(self):
        if self._key is not None:       # nothing held: no graph can address it, param_generation stays
            ops.drop_params()
            self._key = self._value = None


class DropsCachesOnModeChange(object):
    """Mixin (ahead of nn.Module in the bases) for the owner of a ParamCache that folds BatchNorm running statistics: a
    train-mode forward may move them through raw pointers (no _version bump), so train() / eval() drop what was folded."""

    def train(self, mode=True):
        for cache in vars(self).values():
            if isinstance(cache, ParamCache):
                cache.drop()
        return super().train(mode)


def conv_bn_tensors(units):
    """The tensors a fold of `units` (conv units of pytorch_utils) reads, for ParamCache.get."""
    tensors = []
    for unit in units:
        tensors.append(unit.conv.weight)
        if unit.conv.bias is not None:
            tensors.append(unit.conv.bias)
        if hasattr(unit, 'normlayer'):
            bn = unit.normlayer.bn
            tensors += [bn.weight, bn.bias, bn.running_mean, bn.running_var]
            if bn.num_batches_tracked is not None:
                tensors.append(bn.num_batches_tracked)     # bumped by every train-mode forward
    return tensors


def fold_conv_bn(unit, dtype=torch.float32):
    """(scale | None, shift | None) with which conv [+ bias] [+ eval-mode BatchNorm] of one conv unit of pytorch_utils is
    (W x) * scale + shift: scale = gamma / sqrt(var + eps), shift = beta - mean * scale (+ bias * scale). dtype: float32 is
    what the kernels read and every caller takes; float64 exists for the CPU test that checks the fold against a float64 unit."""
    scale = shift = None
    if hasattr(unit, 'normlayer'):
        bn = unit.normlayer.bn
        scale = (bn.weight / torch.sqrt(bn.running_var + bn.eps)).to(dtype).contiguous()
        shift = (bn.bias - bn.running_mean * scale).to(dtype).contiguous()
        if unit.conv.bias is not None:
            shift = (shift + unit.conv.bias * scale).contiguous()
    elif unit.conv.bias is not None:
        shift = unit.conv.bias.detach().to(dtype).contiguous()
    return scale, shift


_index_tables = {}


def index_table(B, n, device, dtype):
    """arange(n).repeat(B, 1): the (B, n) table of 'the first n points' that sequence sampling returns. Built once per shape
    and shared by every caller (they only read it); the cache only grows, so param_generation stays."""
    key = (B, int(n), str(device), dtype)
    table = _index_tables.get(key)
    if table is None:
        table = _index_tables[key] = torch.arange(n, dtype=dtype, device=device).repeat(B, 1)
        ops.publish_params(device, replaced=False)
    return table
