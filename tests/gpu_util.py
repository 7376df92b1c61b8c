import numpy as np
import pytest


@pytest.fixture(scope="module")
def ctx():
    from inverted_index_2_amd import Context
    c = Context(0)
    yield c
    c.close()


class path_delta:
    """with path_delta(ctx) as d: ...  - afterwards d holds what the calls inside launched: {path name: count} of the kernel
    paths whose counters moved (Context.paths())."""

    def __init__(self, ctx):
        self.ctx, self.d = ctx, {}

    def __enter__(self):
        self.before = self.ctx.paths()
        return self.d

    def __exit__(self, *exc):
        after = self.ctx.paths()
        self.d.update({k: after[k] - self.before[k] for k in after if after[k] != self.before[k]})


def blocks_of(l):
    """DV1 blocks of a list of ids (256 postings each, the last one may be short)."""
    return (len(l) + 255) // 256


def sorted_unique(rng, n, universe):
    if n == 0:
        return np.empty(0, np.uint32)
    if n > universe // 2:
        v = np.flatnonzero(rng.random(universe) < n / universe)
    else:
        v = np.unique(rng.integers(0, universe, int(n * 1.1) + 8, dtype=np.int64))[:n]
    return v.astype(np.uint32)
