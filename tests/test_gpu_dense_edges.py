"""GPU: the dense two-list AND family - k_intersect_dense for two and three lists, the two-kernel k_and2 split, k_and2_fused marking,
reading a dense form at one and at two tiles a wave, k_dense_form_build, k_and2_words - and the streaming OR on pairs of lists that
end at doc 0xFFFFFFFF or lie across 0x80000000 (tests/dense_edge_cases.py: the existing case tables, moved), against plain numpy:
np.intersect1d / np.union1d / np.setdiff1d and packed bits, bit for bit.  Every call starts from an output full of 0xDEADBEEF,
finds nothing written behind its result and shows the path its mode names; every option goes back to its default.  A tombstone
bitmap that reaches the last doc id is 512 MiB: each is made once."""
import pytest

from tests import dense_edge_cases as de
from tests.gpu_util import ctx  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("edge", de.EDGES, ids=lambda e: e.name)
def test_the_family_on_a_shifted_case(ctx, edge):
    x, y, sets, _ = edge.data()
    t = edge.third()
    seg = ctx.encode_lists([x, y, t])
    tombs = [(r, ctx.tombstones(r)) for r in sets]
    try:
        took = de.run_family(ctx, (x, y, t), [(seg, 0), (seg, 1)], (seg, 2), tombs=tombs, union_path=de.stream_pacer([x, y]))
        print(edge.name, took)
        assert seg.dense_form(2, words=False) is None                      # the third list: no kernel of the family caches it
        assert all(len(v) == (1 + len(sets) if m.tombstones else 1) for m in de.MODES for v in [took[m.name]])
    finally:
        seg.free()
        for _, tomb in tombs:
            tomb.free()
