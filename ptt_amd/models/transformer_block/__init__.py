"""Mirror of ptt/models/transformer_block/__init__.py: registry + build_transformer (:7-27)."""
from .multitransformer import MulTransformerBlock
from .variants import TransformerBlock, TransformerBlockSTD

__all__ = {
    'MulTransformerBlock': MulTransformerBlock,
    'TransformerBlock': TransformerBlock,
    'TransformerBlockSTD': TransformerBlockSTD,
}

_NOT_ON_HOT_PATH = ('TransformerBlockALL', 'TransformerBlockBackbone', 'TransformerBlockCosine',
                    'TransformerBlockMLP', 'TransformerBlockOffset', 'CrossAttentionBlock')


def build_transformer(model_cfg):
    """model_cfg: NAME, DIM_INPUT, DIM_MODEL, KNN, N_HEADS, N_LAYERS (MulTransformerBlock reads heads / layers; the other
    variants swallow them in **kwargs exactly as in the reference, transformer_block/__init__.py:20-27)."""
    name = model_cfg.NAME
    if name not in __all__:
        if name in _NOT_ON_HOT_PATH:
            raise NotImplementedError(
                "%s exists in the reference but is selected by no shipped config (SURVEY.md §2 row 5/6); "
                "only TransformerBlock / TransformerBlockSTD / MulTransformerBlock are provided" % name)
        raise KeyError(name)
    # optional PRECISION: 'fp32' (absent) or 'bf16x2', the split-bf16 pair kernel of TransformerBlock (its only user)
    precision = model_cfg.get('PRECISION', 'fp32') if hasattr(model_cfg, 'get') else getattr(model_cfg, 'PRECISION', 'fp32')
    if precision != 'fp32' and name != 'TransformerBlock':
        raise ValueError("TRANSFORMER_BLOCK.PRECISION = %r: only TransformerBlock has another arithmetic than 'fp32' (%s runs in fp32)"
                         % (precision, name))
    block = __all__[name](d_points=model_cfg.DIM_INPUT, d_model=model_cfg.DIM_MODEL, k=model_cfg.KNN,
                          heads=model_cfg.N_HEADS, layers=model_cfg.N_LAYERS)
    if name == 'TransformerBlock':
        block.precision = precision     # validated by the attribute: anything but 'fp32' / 'bf16x2' is a ValueError
    return block
