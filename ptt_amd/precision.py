"""Choosing the arithmetic of the fused pair kernel for a whole model: 'fp32' (default) or 'bf16x2' (TransformerBlock.precision)."""
import torch

from .models.transformer_block.variants import PRECISIONS, TransformerBlock


def set_precision(model, precision):
    """Sets `precision` on every TransformerBlock below `model` (itself included) -> how many it set. ValueError for a value
    that is neither 'fp32' nor 'bf16x2' (nothing is changed then).

    One parameter of each such block gets its _version bumped, so every ops.StateWatch and ParamCache that saw the block in
    the old mode sees a change: TrackCore.ready, TrackletRunner and GraphedHotPath re-capture their graphs instead of replaying
    the other arithmetic. The parameter's values are not touched."""
    if precision not in PRECISIONS:
        raise ValueError("set_precision: precision must be one of %s, got %r" % (", ".join(map(repr, PRECISIONS)), precision))
    n = 0
    for m in model.modules():
        if isinstance(m, TransformerBlock):
            m.precision = precision
            torch.autograd.graph.increment_version(m.fc1.weight)
            n += 1
    return n
