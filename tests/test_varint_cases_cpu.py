"""CPU: the varint layouts of tests/varint_cases.py are what they claim to be before they reach a GPU - the matrix round-trips
through the oracle codec and through a LEB128 loop written here, and cells_of(), which reads nothing but the encoded bytes,
finds every wanted cell in the matrix, in every case of VARINT_CASES (or, per consumer, in its cases together: see the module's
docstring) and in the lists of the count and merge tests."""
import functools

import numpy as np
import pytest

from inverted_index_2_amd.engine import path_names
from oracle import oracle as orc
from tests import merge_cases as mc
from tests import path_cases as pc
from tests import varint_cases as vc


def leb128_decode(payload, skip, blk_off, n_postings):
    """The segment's lists, decoded byte by byte (independent of the oracle's C code)."""
    payload, first, byte_off = bytes(payload), skip["first_doc"].tolist(), skip["byte_off"].tolist()
    out, post_off = [], [0]
    for l in range(len(blk_off) - 1):
        for b in range(int(blk_off[l]), int(blk_off[l + 1])):
            doc, gap, shift = first[b], 0, 0
            out.append(doc)
            for byte in payload[byte_off[b]:byte_off[b + 1]]:
                gap |= (byte & 0x7F) << shift
                shift += 7
                if byte < 0x80:
                    doc, gap, shift = doc + gap, 0, 0
                    out.append(doc)
            assert shift == 0, "a block ends inside a varint"
        post_off.append(len(out))
    assert len(out) == n_postings and max(out) < 1 << 32
    return np.array(post_off, np.uint64), np.array(out, np.uint32)


def encoded(lists):
    off, vals = vc.csr(lists)
    return (off, vals) + tuple(orc.dv1_encode(off, vals))


def test_ids_from_widths_gives_exactly_the_widths():
    rng = np.random.default_rng(1)
    widths = rng.integers(1, 5, 400)
    ids = vc.ids_from_widths(9, widths, rng)
    gaps = np.diff(ids.astype(np.int64))
    assert ids[0] == 9 and np.array_equal(vc.varint_len(gaps), widths)
    for w in (2, 3, 4, 5):                                  # every 7-bit group of a wide gap is non-zero, the top one is 1
        g = np.diff(vc.ids_from_widths(0, [w] * 7, rng).astype(np.int64))
        assert np.all(g >> (7 * (w - 1)) == 1) and all(np.all((g >> (7 * k)) & 127) for k in range(w - 1))
    with pytest.raises(AssertionError):
        vc.ids_from_widths(0, [5] * 16, rng)               # sixteen five-byte gaps leave the id space


def test_the_fullest_block_is_found_by_search():
    widths, counts = vc.fullest_block()
    assert counts == (14, 241, 0) and int(widths.sum()) == 1034 > 4 * 256      # 14 * 2^28 + 241 * 2^21 < 2^32: five chunks


def test_matrix_roundtrips_through_both_decoders():
    lists, _ = vc.matrix_segment()
    off, vals, blk_off, skip, payload = encoded(lists)
    po, ids = leb128_decode(payload, skip, blk_off, vals.size)
    assert np.array_equal(po, off) and np.array_equal(ids, vals)
    po2, ids2 = orc.dv1_decode(blk_off, skip, payload, vals.size)
    assert np.array_equal(po2, off) and np.array_equal(ids2, vals)


def test_matrix_holds_every_wanted_cell():
    lists, is_matrix = vc.matrix_segment()
    _, _, blk_off, skip, payload = encoded(lists)
    cells = vc.cells_of(payload, skip, blk_off, [i for i, m in enumerate(is_matrix) if m])
    wanted = vc.wanted_cells()
    assert len(wanted) == sum(16 + 2 * (w + 1) for w in vc.WIDTHS)
    assert wanted <= cells, sorted(wanted - cells)
    for w in vc.WIDTHS:                                     # spelled out: dword phases, piece phases, both chunk boundaries
        v = [c for c in cells if c[0] == "v" and c[1] == w]
        assert {c[2] for c in v} == {0, 1, 2, 3} and {c[3] for c in v} == set(range(16))
        assert {c[4] for c in v} >= {(B, k) for B in vc.CHUNKS for k in range(w + 1)}
    assert {c[1] for c in cells if c[0] == "start"} == set(range(16))
    assert {c[1] for c in cells if c[0] == "tail"} == {1, 2, 3}
    assert ("cont4",) in cells and ("cont4_piece",) in cells
    # the further layouts: payload sizes, short blocks, the fullest block
    by_name = {n: ids for n, ids in vc.matrix()}
    size = lambda ids: int(vc.varint_len(np.diff(ids.astype(np.int64))).sum())
    for nbytes in (255, 256, 257, 511, 512, 513):
        assert size(by_name[f"payload_{nbytes}"]) == nbytes and by_name[f"payload_{nbytes}"].size == 256
    assert size(by_name["payload_255_short_block"]) == 255 and by_name["payload_255_short_block"].size == 200
    assert size(by_name["fullest"]) == 1034 and by_name["one_posting"].size == 1
    for n in (2, 3, 4, 5):
        for w in vc.WIDTHS:
            ids = by_name[f"short_{n}_last_w{w}"]
            assert ids.size == n and vc.varint_len(int(ids[-1]) - int(ids[-2])) == w


def test_partner_holds_the_ids_around_a_planted_varint_and_decoys_outside_the_list():
    c, marks = vc.carrier45(1, 0)
    p = vc.partner(c, marks)
    assert np.all(np.isin(c[marks], p)) and np.all(np.isin(c[np.array(marks) - 1], p))
    decoys = np.setdiff1d(p, c)
    assert decoys.size >= 4 * len(marks)
    i = marks[0]
    prev, gap = int(c[i - 1]), int(c[i]) - int(c[i - 1])
    w = int(vc.varint_len(gap))
    top = gap >> (7 * (w - 1))
    assert prev + gap - (top << 7 * (w - 1)) + (top << 7 * (w - 2)) in decoys.tolist()      # the last byte shifted 7 bits too few


# ---- the cases -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_cells(name):
    lists = vc.BY_NAME[name].lists()
    _, _, blk_off, skip, payload = encoded(lists)
    return vc.cells_of(payload, skip, blk_off)


def test_cases_are_well_formed():
    names = set(path_names())
    for case in vc.VARINT_CASES:
        assert set(case.options) <= set(pc.DEFAULTS), case.name
        assert set(case.expect) <= names and all(isinstance(v, int) and v > 0 for v in case.expect.values()), case.name
        assert case.need in ("w23", "dense", "w45") and case.layouts() == ["one", "two"], case.name
    consumers = {c.consumer for c in vc.VARINT_CASES}
    assert set(vc.WIDE_CONSUMERS) <= consumers
    assert consumers >= {"and.and2_fused", "and.and2_split", "and.dense2", "and.dense3", "and.dense4", "or.stream2", "or.stream3", "or.stream4",
                         "or.tiles", "or.tiles_wide"}
    for case in vc.VARINT_CASES:                            # the consumer a case names is a path it expects (or a group of them)
        assert any(k == case.consumer or k.startswith(case.consumer + ".") for k in case.expect), case.name


@pytest.mark.parametrize("case", vc.VARINT_CASES, ids=lambda c: c.name)
def test_case_carries_its_cells(case):
    cells = case_cells(case.name)
    if case.need == "w23":
        assert vc.W23 <= cells, sorted(vc.W23 - cells)
    elif case.need == "dense":
        assert vc.dense_ok(cells)
        # a full block of 256 bytes and a short one of 255 with continuation bytes: the lengths at which only the continuation
        # term of the streaming kernels' private fast-path tests (len > 256 || any, len != 255 || any) sends a block to the decoder
        assert ("len", 255) in cells and ("len", 256) in cells
        assert not any(c[0] == "v" and c[1] >= 4 for c in cells)
    else:
        assert cells & vc.W45


@pytest.mark.parametrize("consumer", vc.WIDE_CONSUMERS)
def test_consumer_carries_every_wide_cell(consumer):
    cells = set()
    for case in vc.VARINT_CASES:
        if case.consumer == consumer:
            cells |= case_cells(case.name)
    assert vc.W45 <= cells, sorted(vc.W45 - cells)
    assert vc.W23 <= cells and ("cont4",) in cells and ("cont4_piece",) in cells


def test_the_sixteen_byte_probes_are_reached_and_meet_every_cell():
    """decode_rows16_any runs for a probed list only with PROBE_MIN_BLOCKS of its blocks in the driver block's doc range
    (intersect.hip: `NFIX == 0u && bh - bl >= 16u`): counted here from the lists, as k_isect_partition counts them, for the
    driver block of every id that ends a planted varint."""
    assert {c.name for c in vc.VARINT_CASES if c.consumer == "and.tiles_sub"} == set(vc.PROBED_CASES)
    cells = set()
    for name, (seed, j) in vc.PROBED_CASES.items():
        case = vc.BY_NAME[name]
        carrier, driver = case.lists()
        c2, d2, marks = vc.probe_pair(seed, j, driver.size)
        assert carrier is c2 and driver is d2 and case.call == ("intersect", [0, 1])
        assert 2 <= -(-driver.size // 256) < -(-carrier.size // 256)                            # the partner drives, more than one block
        assert np.all(np.isin(carrier[list(marks)], driver))                                    # every planted varint's id is a candidate
        assert min(vc.probed_blocks(driver, carrier, carrier[list(marks)])) >= vc.PROBE_MIN_BLOCKS
        _, _, blk_off, skip, payload = encoded([carrier])
        cells |= vc.cells_of(payload, skip, blk_off)
    assert vc.W23 <= cells and vc.W45 <= cells and ("cont4_piece",) in cells
    # the 64-list split drivers: the carrier is the longest list, one of the lists 2 .. 63 the combined pass probes
    assert len(vc.COMBINED_PROBE_CASES) >= 2
    for name in vc.COMBINED_PROBE_CASES:
        lists = vc.BY_NAME[name].lists()
        assert len(lists) == 64 and max(range(64), key=lambda i: -(-lists[i].size // 256)) == 0
    assert any(("cont4_piece",) in case_cells(name) for name in vc.COMBINED_PROBE_CASES)


@pytest.mark.parametrize("case", vc.VARINT_CASES, ids=lambda c: c.name)
def test_reference_is_not_trivial(case):
    lists = case.lists()
    for l in lists:
        assert l.dtype == np.uint32 and l.size and np.all(l[1:] > l[:-1])
    plain = pc.reference(case, lists)
    for (op, operands), res in zip(pc.operands(case, lists), plain):
        assert res.dtype == np.uint64 and res.size > 0
        if op == "or":
            assert res.size > max(o.size for o in operands)
        else:
            assert res.size < min(o.size for o in operands)
    if case.tomb:
        removed = pc.removed_ids(case, lists)
        for res, left in zip(plain, pc.reference(case, lists, removed)):
            assert 0 < left.size < res.size


def test_count_lists_carry_every_cell():
    lists, ids = vc.count_lists()
    _, _, blk_off, skip, payload = encoded(lists)
    cells = vc.cells_of(payload, skip, blk_off)
    assert vc.W23 <= cells and vc.W45 <= cells
    hits = [int(np.count_nonzero(np.isin(l, ids))) for l in lists]
    assert all(0 < h < l.size for h, l in zip(hits, lists)) and np.setdiff1d(ids, np.concatenate(lists)).size > 100


@pytest.mark.parametrize("case", vc.MERGE_CASES, ids=lambda c: c.name)
def test_merge_segments_carry_every_cell(case):
    segs = case.segs()
    cells = set()
    for off, vals in segs:
        blk_off, skip, payload = orc.dv1_encode(off, vals)
        cells |= vc.cells_of(payload, skip, blk_off)
    assert vc.W23 <= cells and vc.W45 <= cells, sorted((vc.W23 | vc.W45) - cells)
    n_in = sum(v.size for _, v in segs)
    p = case.plan()
    if "small_terms" in case.name:
        assert n_in <= 8192 and len(segs[0][0]) - 1 <= 512           # ii2_merge_small takes them
    else:
        assert {"small", "large", "range"} <= p.branches              # batches of small terms and range tiles
        # the blocks the tile bounds cut in two - what the plan kernels' own decoders walk - hold gaps of every width
        T = len(segs[0][0]) - 1
        cut = set()
        for t in np.flatnonzero(p.large & ~p.bitmap):
            cut |= vc.straddled_widths(case, int(t))
        assert cut == {1, 2, 3, 4, 5} and 5 in vc.straddled_widths(case, T - 1)
    removed = case.removed()
    w_off, w_vals, _ = orc.merge_segments([o for o, _ in segs], [v for _, v in segs], removed)
    r_off, r_vals = mc.reference(segs, removed)
    assert np.array_equal(w_off, r_off) and np.array_equal(w_vals.astype(np.uint64), r_vals) and 0 < w_vals.size < n_in
