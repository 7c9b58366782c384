"""Choosing the arithmetic of the fused kernels for a whole model: 'fp32' (default) or 'bf16x2' (TransformerBlock.precision,
PointnetSAModuleVotes.precision, CosineSimAug.precision)."""
import torch

from .models.backbones_3d.pointnet2.pointnet2_modules import PointnetSAModuleVotes
from .models.backbones_3d.pointnet2_backbone import PointNet2BackboneLight
from .models.similarity_modules.p2b_xcoor import CosineSimAug
from .models.transformer_block.variants import PRECISIONS, TransformerBlock

SCOPES = ('transformer', 'sa', 'similarity')


def set_precision(model, precision, scope=('transformer',)):
    """Sets `precision` on every module below `model` (itself included) that `scope` names -> how many it set. scope is a
    collection of 'transformer' (every TransformerBlock: the default, alone), 'sa' (the SA levels of every
    PointNet2BackboneLight — the modules SA_CONFIG.PRECISION configures — and `model` itself when it is a PointnetSAModuleVotes:
    the split-bf16 stream kernel of the dense SA1 / SA2 levels; the box head's vote aggregation, 257 -> 256 -> 256 -> 256 on 16
    neighbours, has no second arithmetic and is left alone) and 'similarity' (every CosineSimAug, `model` itself included — the
    modules SIMILARITY_MODULE.PRECISION configures: the split-bf16 kernel of the batched pair MLP). ValueError for a value that
    is neither 'fp32' nor 'bf16x2' and for an unknown scope name (nothing is changed then).

    One parameter of each module that is set gets its _version bumped (fc1.weight of a TransformerBlock,
    mlp_module[0].conv.weight of an SA module, mlp[0].conv.weight of a CosineSimAug), so every ops.StateWatch and ParamCache
    that saw the module in the old mode sees a change: TrackCore.ready, TrackletRunner and GraphedHotPath re-capture their
    graphs instead of replaying the other arithmetic. The parameter's values are not touched."""
    if precision not in PRECISIONS:
        raise ValueError("set_precision: precision must be one of %s, got %r" % (", ".join(map(repr, PRECISIONS)), precision))
    scope = (scope,) if isinstance(scope, str) else tuple(scope)
    for name in scope:
        if name not in SCOPES:
            raise ValueError("set_precision: scope must name some of %s, got %r" % (", ".join(map(repr, SCOPES)), name))
    levels = []
    if 'sa' in scope:
        levels = [model] if isinstance(model, PointnetSAModuleVotes) else []
        for m in model.modules():
            if isinstance(m, PointNet2BackboneLight):
                levels += [sa for sa in m.SA_modules if isinstance(sa, PointnetSAModuleVotes)]
    n = 0
    for m in model.modules():
        if 'transformer' in scope and isinstance(m, TransformerBlock):
            m.precision = precision
            torch.autograd.graph.increment_version(m.fc1.weight)
            n += 1
        if 'similarity' in scope and isinstance(m, CosineSimAug):
            m.precision = precision
            torch.autograd.graph.increment_version(m.mlp[0].conv.weight)
            n += 1
    for m in levels:
        m.precision = precision
        torch.autograd.graph.increment_version(m.mlp_module[0].conv.weight)
        n += 1
    return n
