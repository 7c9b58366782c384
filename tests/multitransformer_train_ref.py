"""Shared by tests/golden/make_golden_g20.py and the MulTransformerBlock training tests: which blocks G20 records, from which seeds,
and how a gradient is sampled, so the fixture script and the tests index the same entries."""
import numpy as np

BLOCKS = ((1, 1), (2, 1), (8, 1), (4, 2))      # (heads, layers)
B, N = 2, 64
MAX_SAMPLE = 640                               # values kept per gradient (the issue allows up to 4096; this keeps the file < 1 MiB)


def train_seed(heads, layers):
    return 2000 + 10 * heads + layers


def sample(a):
    """The fixed strided sample of an array: flat[::ceil(numel / MAX_SAMPLE)]."""
    flat = np.asarray(a).reshape(-1)
    return flat[::max(1, -(-flat.size // MAX_SAMPLE))]


def split(names, shapes, g):
    """{name: its slice of the concatenated sample g} for gradients of the given shapes."""
    out, off = {}, 0
    for n, s in zip(names, shapes):
        size = int(np.prod(s))
        cnt = len(range(0, size, max(1, -(-size // MAX_SAMPLE))))
        out[n] = g[off:off + cnt]
        off += cnt
    assert off == len(g), (off, len(g))
    return out
